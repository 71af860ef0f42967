"""The self-overlap kernels (psa_amd/csrc/overlap.hip) as the compiler builds them for gfx950 (hipcc cross-compiles here),
from the compiler's resource remarks and the assembly: no scratch and no spilled registers anywhere; every kernel within
128 registers; no atomic of any kind, global or LDS; the count kernel uses no LDS and loads u64 with 8-byte loads;
msd.hip, which now shares msd_unit.h with it, still compiles to its seven kernels; the Makefile lists the sources."""
import re

import pytest

from kernel_build import SRC, device_compile

KERNELS = ("overlap_count_kernel", "overlap_reduce_kernel", "overlap_moments_kernel")
MSD_KERNELS = ("msd_unwrap_count_kernel", "msd_unwrap_scan_kernel", "msd_unwrap_write_kernel", "msd_moments_kernel",
               "msd_moments_reduce_kernel", "msd_moments_finish_kernel", "msd_hist_kernel")


def test_makefile_lists_the_sources():
    mk = (SRC / "Makefile").read_text()
    srcs = next(ln for ln in mk.splitlines() if ln.startswith("SRCS"))
    assert " overlap.hip" in srcs and " api_overlap.hip" in srcs
    assert re.search(r"for f in [^;]*\boverlap\b[^;]*; do", mk)               # the asm list
    assert all((SRC / f).is_file() for f in srcs.split(":=")[1].split())
    rule = next(ln for ln in mk.splitlines() if ln.startswith("$(BUILD)/%.o"))
    assert "msd_unit.h" in rule and (SRC / "msd_unit.h").is_file()


@pytest.fixture(scope="module")
def compiled():
    c = device_compile("overlap.hip")
    print(c.usage)
    return c.usage, c.asm


def _body(asm, name):
    body = asm[asm.index(name + ":"):]
    return body[:body.index("s_endpgm")]


def test_overlap_kernels_resources(compiled):
    usage, asm = compiled
    assert len(usage) == len(KERNELS) and all(any(k in name for name in usage) for k in KERNELS)
    for name, u in usage.items():
        assert u["ScratchSize [bytes/lane]"] == 0 and u["VGPRs Spill"] == 0 and u["SGPRs Spill"] == 0, (name, u)
        assert u["VGPRs"] + u["AGPRs"] <= 128, (name, u)
    assert "scratch_" not in asm
    name, u = next((k, v) for k, v in usage.items() if "overlap_count_kernel" in k)
    assert u["LDS Size [bytes/block]"] == 0
    body = _body(asm, name)
    assert body.count("global_load_dwordx2") + 2 * body.count("global_load_dwordx4") >= 27   # (the origin + eight lags) x 3 components
    assert "ds_" not in body and "s_barrier" not in body


def test_no_atomics(compiled):
    usage, asm = compiled
    assert "atomic" not in asm and "cmpswap" not in asm and "cmpst" not in asm
    assert not re.search(r"\bds_\w*(add|sub|inc|dec|min|max|and|or|xor|wrxchg)\w*", asm)
    for name in usage:
        body = _body(asm, name)
        assert ("ds_write" in body or "ds_read" in body) == ("overlap_moments_kernel" in name), name


def test_msd_still_compiles_to_its_seven_kernels():
    usage = device_compile("msd.hip").usage
    assert len(usage) == len(MSD_KERNELS) and all(any(k in name for name in usage) for k in MSD_KERNELS)
    text = (SRC / "msd.hip").read_text()
    assert '#include "msd_unit.h"' in text and "struct MsdUnit" not in text and "struct MsdChunk" not in text
    assert '#include "msd_unit.h"' in (SRC / "overlap.hip").read_text()
