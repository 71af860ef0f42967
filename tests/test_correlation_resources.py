"""The time-correlation kernels (psa_amd/csrc/correlation.hip) as the compiler builds them for gfx950 (hipcc cross-compiles
here), from the compiler's resource remarks and the assembly: no scratch and no spilled registers, at most 128 VGPRs, no
LDS; the back-transform's inner blocks hold float64 FMAs -- in the columns form CORR_LAGS of them per load of the power,
fed from scalar registers --; no atomics; the Makefile lists the sources."""
import re

import pytest

from kernel_build import SRC, device_compile

CORR_LAGS = 8


def test_makefile_lists_the_sources():
    mk = (SRC / "Makefile").read_text()
    srcs = next(ln for ln in mk.splitlines() if ln.startswith("SRCS"))
    assert " correlation.hip" in srcs and " api_correlation.hip" in srcs
    assert re.search(r"for f in [^;]*\bcorrelation\b[^;]*; do", mk)          # the asm list
    assert all((SRC / f).is_file() for f in srcs.split(":=")[1].split())
    text = (SRC / "psa_ctx.h").read_text()
    assert f"constexpr int CORR_LAGS = {CORR_LAGS};" in text


@pytest.fixture(scope="module")
def compiled():
    c = device_compile("correlation.hip")
    print(c.usage)
    return c.usage, c.asm


def test_correlation_kernels_resources(compiled):
    usage, asm = compiled
    # padding with and without the copy; the back-transform's two layouts for float64 and float32 input
    assert len(usage) == 6
    assert sum("correlation_pad_kernel" in k for k in usage) == 2
    assert sum("correlation_transform_cols_kernel" in k for k in usage) == 2
    assert sum("correlation_transform_lags_kernel" in k for k in usage) == 2
    for name, u in usage.items():
        assert u["ScratchSize [bytes/lane]"] == 0 and u["VGPRs Spill"] == 0 and u["SGPRs Spill"] == 0, (name, u)
        assert u["VGPRs"] + u["AGPRs"] <= 128 and u["LDS Size [bytes/block]"] == 0, (name, u)
    assert "scratch_" not in asm
    assert "atomic" not in asm and "ds_add" not in asm                        # no atomics anywhere


def _body(asm, name):
    body = asm[asm.index(name + ":"):]
    return body[:body.index("s_endpgm")]


def _fma64(block):
    return block.count("v_fma_f64") + block.count("v_fmac_f64")


def test_back_transform_inner_blocks(compiled):
    usage, asm = compiled
    for name in usage:
        if "transform" not in name:
            assert _fma64(_body(asm, name)) == 0, name                        # the padding pass does no arithmetic
            continue
        blocks = re.split(r"\n\.LBB\d+_\d+:", _body(asm, name))
        loops = [b for b in blocks if _fma64(b) and ("global_load" in b or "s_load" in b)]
        assert loops, name
        for b in loops:
            print(f"{name}: an inner block with {_fma64(b)} float64 FMAs, {b.count('global_load')} vector loads")
            assert "v_fma_f32" not in b and "v_fmac_f32" not in b, name       # nothing of the sum in float32
            assert "global_store" not in b, name
        if "cols_kernel" in name:
            # one load of the power feeds CORR_LAGS FMAs whose table entries sit in scalar registers
            best = max(loops, key=_fma64)
            assert _fma64(best) % CORR_LAGS == 0 and _fma64(best) // CORR_LAGS == best.count("global_load"), name
            assert len(re.findall(r"v_fmac?_f64\S* v\[\d+:\d+\], s\[\d+:\d+\]", best)) == _fma64(best), name
