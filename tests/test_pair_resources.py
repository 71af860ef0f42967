"""The pair kernels (psa_amd/csrc/pair.hip) as the compiler builds them for gfx950 (hipcc cross-compiles here), from the
compiler's resource remarks and the assembly: no scratch and no spilled registers anywhere; every kernel within 128
registers; the LDS of the histogram kernel lets at least two workgroups share a compute unit; the inner pair loop -- the
block with the most square roots -- reads LDS and loads nothing from global memory; no global atomic of any kind, no
float LDS atomic, and the 32-bit integer LDS add in the histogram kernel alone; the Makefile lists the sources."""
import re

import pytest

from kernel_build import SRC, device_compile
from psa_amd import _hip

LDS_PER_CU = 160 * 1024
KERNELS = ("pair_frac_kernel", "pair_hist_kernel")          # the integer reduce: test_hist_reduce_resources.py


def test_makefile_lists_the_sources():
    mk = (SRC / "Makefile").read_text()
    srcs = next(ln for ln in mk.splitlines() if ln.startswith("SRCS"))
    assert " pair.hip" in srcs and " api_pair.hip" in srcs
    assert re.search(r"for f in [^;]*\bpair\b[^;]*; do", mk)                  # the asm list
    assert all((SRC / f).is_file() for f in srcs.split(":=")[1].split())


def test_exported_constants():
    head = (SRC / "psa_ctx.h").read_text()
    for name in ("PAIR_TILE", "PAIR_MAX_BINS", "PAIR_MAX_LAGS", "PAIR_MAX_SPECIES"):
        assert int(re.search(rf"constexpr int {name} = (\d+);", head).group(1)) == getattr(_hip, name)
    assert (_hip.PAIR_MAX_BINS, _hip.PAIR_MAX_LAGS, _hip.PAIR_MAX_SPECIES) == (1024, 64, 8) and _hip.PAIR_TILE % 64 == 0


@pytest.fixture(scope="module")
def compiled():
    c = device_compile("pair.hip")
    print(c.usage)
    return c.usage, c.asm


def _body(asm, name):
    body = asm[asm.index(name + ":"):]
    return body[:body.index("s_endpgm")]


def test_pair_kernels_resources(compiled):
    usage, asm = compiled
    assert len(usage) == len(KERNELS) and all(any(k in name for name in usage) for k in KERNELS)
    for name, u in usage.items():
        assert u["ScratchSize [bytes/lane]"] == 0 and u["VGPRs Spill"] == 0 and u["SGPRs Spill"] == 0, (name, u)
        assert u["VGPRs"] + u["AGPRs"] <= 128, (name, u)
    assert "scratch_" not in asm
    name, u = next((k, v) for k, v in usage.items() if "pair_hist_kernel" in k)
    least = (_hip.PAIR_MAX_BINS + 1) * 4 + 3 * _hip.PAIR_TILE * 4          # one histogram and the staged tile
    assert least <= u["LDS Size [bytes/block]"] and 2 * u["LDS Size [bytes/block]"] <= LDS_PER_CU


def test_inner_pair_loop(compiled):
    usage, asm = compiled
    name = next(k for k in usage if "pair_hist_kernel" in k)
    blocks = re.split(r"\n\.LBB\d+_\d+:", _body(asm, name))
    roots = [b.count("v_sqrt_f32") + b.count("v_rsq_f32") for b in blocks]
    inner = blocks[roots.index(max(roots))]
    valu = len(re.findall(r"\n\s+v_", inner))
    print(f"the inner loop: {max(roots)} roots, {valu} VALU instructions, {len(re.findall(r'ds_read', inner))} LDS reads, "
          f"{inner.count('ds_add_u32')} LDS adds")
    assert max(roots) >= 4 and inner.count("ds_add_u32") >= 4                  # four beta-atoms per pass
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
        assert (adds >= 1) == ("pair_hist_kernel" in name), (name, adds)
        assert "ds_add_rtn" not in _body(asm, name) and "ds_add_u64" not in _body(asm, name)
