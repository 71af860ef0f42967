"""The covariance kernels (psa_amd/csrc/covariance.hip) as the compiler builds them for gfx950 (hipcc cross-compiles
here), from the compiler's resource remarks and the assembly: the six instantiations of covariance_kernel (1 .. 6 row
blocks of 16, n = 3B <= 96) and the float64 finishing pass -- no scratch, no spilled registers, the LDS image as planned
(16 NB rows x 66 complex values, the two weight rows of a tile and the row starts) and at most 80 KiB per workgroup, so
that two workgroups share a compute unit's 160 KiB, the products on the fp32 matrix cores, and the hot loop a plain MFMA
stream: the accumulators are the MFMA's own registers (4 per tile pair, at most one more tile's worth in AGPRs) and the block that holds the
MFMAs has no branch but its own back edge and does not copy the accumulators."""
import re

import pytest

from kernel_build import SRC, device_compile


def test_makefile_lists_the_sources():
    mk = (SRC / "Makefile").read_text()
    srcs = next(ln for ln in mk.splitlines() if ln.startswith("SRCS"))
    assert " covariance.hip" in srcs and " api_covariance.hip" in srcs
    assert re.search(r"for f in [^;]*\bcovariance\b[^;]*; do", mk)            # the asm list
    assert all((SRC / f).is_file() for f in srcs.split(":=")[1].split())


@pytest.fixture(scope="module")
def compiled():
    """(resource remarks per kernel, assembly) of covariance.hip, compiled once"""
    c = device_compile("covariance.hip")
    print(c.usage)
    return c.usage, c.asm


def test_covariance_kernels_resources(compiled):
    usage, asm = compiled
    assert len(usage) == 7
    for nb in range(1, 7):
        name, u = next((k, v) for k, v in usage.items() if f"covariance_kernelILi{nb}EE" in k)
        assert u["ScratchSize [bytes/lane]"] == 0 and u["VGPRs Spill"] == 0 and u["SGPRs Spill"] == 0, (name, u)
        assert u["Occupancy [waves/SIMD]"] >= 1 and u["VGPRs"] + u["AGPRs"] <= 512, (name, u)
        assert u["LDS Size [bytes/block]"] == 16 * nb * 66 * 8 + 2 * 64 * 4 + 16 * nb * 8, (name, u)
        assert u["LDS Size [bytes/block]"] <= 80 * 1024, (name, u)
        assert 0 <= u["AGPRs"] - 4 * (nb * (nb + 1) // 2) <= 4, (name, u)     # the accumulators, one more tile at the most
        body = asm[asm.index(name + ":"):]
        body = body[:body.index("s_endpgm")]
        hot = [b for b in re.split(r"\n\.LBB\d+_\d+:", body) if "v_mfma_f32_16x16x4" in b]
        assert len(hot) == 1, (name, len(hot))                                # one loop holds every MFMA
        loop = hot[0].split("s_cbranch")[0]                                   # up to the back edge
        assert loop.count("v_mfma_f32_16x16x4") == 2 * 2 * (nb * (nb + 1) // 2), name     # two steps x two terms per pair
        # no accumulator is copied around the MFMAs (the register allocator swaps one tile's four registers per pass at
        # NB = 3: twelve moves beside 24 MFMAs); none at all in the configuration-3 kernel
        assert loop.count("v_accvgpr_") <= (0 if nb == 2 else 12) and hot[0].count("s_cbranch") == 1, name
    u2 = next(v for k, v in usage.items() if "covariance_kernelILi2EE" in k)
    assert u2["VGPRs"] <= 64 and u2["Occupancy [waves/SIMD]"] >= 4, u2         # configuration 3: n = 24
    name, u = next((k, v) for k, v in usage.items() if "covariance_finish_kernel" in k)
    assert u["ScratchSize [bytes/lane]"] == 0 and u["VGPRs Spill"] == 0 and u["SGPRs Spill"] == 0 and u["LDS Size [bytes/block]"] == 0, (name, u)
    assert "scratch_" not in asm
    assert "v_mfma_f32_16x16x4" in asm and "ds_read_b64" in asm               # fp32 matrix cores, 8-byte operand reads
    assert "global_atomic" not in asm and "ds_add" not in asm                 # no atomics anywhere
