"""The displacement kernels (psa_amd/csrc/msd.hip) as the compiler builds them for gfx950 (hipcc cross-compiles here), from
the compiler's resource remarks and the assembly: no scratch and no spilled registers anywhere; every kernel within 128
registers; the LDS of the moments and histogram kernels lets at least two workgroups share a compute unit; the moments
kernel's inner loop -- the block with the float64 accumulation of four origins -- reads LDS and loads nothing from
global memory; no global atomic of any kind, no float LDS atomic, and the 32-bit integer LDS add in the histogram kernel
alone; the Makefile lists the sources."""
import re

import pytest

from kernel_build import SRC, device_compile
from psa_amd import _hip

LDS_PER_CU = 160 * 1024
KERNELS = ("msd_unwrap_count_kernel", "msd_unwrap_scan_kernel", "msd_unwrap_write_kernel", "msd_moments_kernel",
           "msd_moments_reduce_kernel", "msd_moments_finish_kernel", "msd_hist_kernel")          # the integer reduce: test_hist_reduce_resources.py


def test_makefile_lists_the_sources():
    mk = (SRC / "Makefile").read_text()
    srcs = next(ln for ln in mk.splitlines() if ln.startswith("SRCS"))
    assert " msd.hip" in srcs and " api_msd.hip" in srcs
    assert re.search(r"for f in [^;]*\bmsd\b[^;]*; do", mk)                   # the asm list
    assert all((SRC / f).is_file() for f in srcs.split(":=")[1].split())


@pytest.fixture(scope="module")
def compiled():
    c = device_compile("msd.hip")
    print(c.usage)
    return c.usage, c.asm


def _body(asm, name):
    body = asm[asm.index(name + ":"):]
    return body[:body.index("s_endpgm")]


def test_msd_kernels_resources(compiled):
    usage, asm = compiled
    assert len(usage) == len(KERNELS) and all(any(k in name for name in usage) for k in KERNELS)
    for name, u in usage.items():
        assert u["ScratchSize [bytes/lane]"] == 0 and u["VGPRs Spill"] == 0 and u["SGPRs Spill"] == 0, (name, u)
        assert u["VGPRs"] + u["AGPRs"] <= 128, (name, u)
    assert "scratch_" not in asm
    name, u = next((k, v) for k, v in usage.items() if "msd_moments_kernel" in k)
    assert u["LDS Size [bytes/block]"] == 3 * (_hip.MSD_WINDOW + _hip.MSD_ORIGINS) * 4 and 2 * u["LDS Size [bytes/block]"] <= LDS_PER_CU
    name, u = next((k, v) for k, v in usage.items() if "msd_hist_kernel" in k)
    assert (_hip.MSD_MAX_BINS + 1) * 4 <= u["LDS Size [bytes/block]"] <= (_hip.MSD_MAX_BINS + 4) * 4
    assert 2 * u["LDS Size [bytes/block]"] <= LDS_PER_CU


def test_moments_inner_loop(compiled):
    usage, asm = compiled
    name = next(k for k in usage if "msd_moments_kernel" in k)
    blocks = re.split(r"\n\.LBB\d+_\d+:", _body(asm, name))
    f64 = [b.count("v_add_f64") + b.count("v_fma_f64") for b in blocks]
    inner = blocks[f64.index(max(f64))]
    print(f"the inner loop: {max(f64)} float64 adds, {len(re.findall(r'ds_read', inner))} LDS reads, "
          f"{inner.count('v_cvt_f64_f32')} conversions")
    assert max(f64) >= 16                                                     # four origins x four sums
    assert "global_load" not in inner and "flat_load" not in inner and "buffer_load" not in inner and "s_load" not in inner
    assert "ds_read" in inner and "s_barrier" not in inner and "ds_write" not in inner
    assert re.search(r"s_cbranch_\w+ \.LBB", inner)                           # it is a loop's body


def test_atomics(compiled):
    usage, asm = compiled
    assert "global_atomic" not in asm and "flat_atomic" not in asm and "buffer_atomic" not in asm
    assert not re.search(r"ds_\w*(add|sub|min|max)\w*_f(16|32|64)|ds_pk_add", asm)   # no float LDS atomic
    assert "cmpswap" not in asm and "cmpst" not in asm
    for name in usage:
        adds = _body(asm, name).count("ds_add_u32")
        assert (adds >= 1) == ("msd_hist_kernel" in name), (name, adds)
        assert "ds_add_rtn" not in _body(asm, name) and "ds_add_u64" not in _body(asm, name)
