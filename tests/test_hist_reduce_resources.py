"""The integer reduce of the real-space histograms (psa_amd/csrc/hist_reduce.hip; the one kernel behind psa_van_hove_self,
psa_pair_histogram and psa_angle_histogram) as the compiler builds it for gfx950 (hipcc cross-compiles here), from the
compiler's resource remarks and the assembly: no scratch and no spilled registers; within 128 registers; no global atomic
of any kind, no float LDS atomic, no 64-bit LDS atomic and no 32-bit integer LDS add (that one belongs to the histogram
kernels alone); the Makefile lists the file and the shared geometry header; msd.hip, pair.hip and angle.hip hold no
reduce and no displacement chain of their own."""
import re

import pytest

from kernel_build import SRC, device_compile

KERNELS = ("hist_reduce_kernel",)


def test_makefile_lists_the_sources():
    mk = (SRC / "Makefile").read_text()
    srcs = next(ln for ln in mk.splitlines() if ln.startswith("SRCS"))
    assert " hist_reduce.hip" in srcs and " api_realspace.hip" in srcs
    assert re.search(r"for f in [^;]*\bhist_reduce\b[^;]*; do", mk)           # the asm list
    assert "min_image.h" in mk and (SRC / "min_image.h").is_file()            # the shared header is a prerequisite
    assert all((SRC / f).is_file() for f in srcs.split(":=")[1].split())


def test_one_reduce_and_one_chain():
    for f in ("msd.hip", "pair.hip", "angle.hip"):
        text = re.sub(r"//[^\n]*", "", (SRC / f).read_text())                 # the code without its comments
        assert '#include "min_image.h"' in text and "rintf(" not in text and "floorf(" not in text, f
        assert not re.search(r"\w+_reduce_kernel", text.replace("msd_moments_reduce_kernel", "")), f
    assert len(re.findall(r"__global__", (SRC / "hist_reduce.hip").read_text())) == 1


@pytest.fixture(scope="module")
def compiled():
    c = device_compile("hist_reduce.hip")
    print(c.usage)
    return c.usage, c.asm


def test_hist_reduce_resources(compiled):
    usage, asm = compiled
    assert len(usage) == len(KERNELS) and all(any(k in name for name in usage) for k in KERNELS)
    for name, u in usage.items():
        assert u["ScratchSize [bytes/lane]"] == 0 and u["VGPRs Spill"] == 0 and u["SGPRs Spill"] == 0, (name, u)
        assert u["VGPRs"] + u["AGPRs"] <= 128, (name, u)
        assert u["LDS Size [bytes/block]"] == 8 * 32 * 8                       # eight strands of 32 uint64 sums
    assert "scratch_" not in asm


def test_atomics(compiled):
    usage, asm = compiled
    assert "global_atomic" not in asm and "flat_atomic" not in asm and "buffer_atomic" not in asm
    assert not re.search(r"ds_\w*(add|sub|min|max)\w*_f(16|32|64)|ds_pk_add", asm)   # no float LDS atomic
    assert "cmpswap" not in asm and "cmpst" not in asm
    assert "ds_add_u32" not in asm and "ds_add_rtn" not in asm and "ds_add_u64" not in asm
