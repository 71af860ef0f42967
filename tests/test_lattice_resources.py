"""The lattice-spectra kernels (psa_amd/csrc/lattice.hip) as the compiler builds them for gfx950 (hipcc cross-compiles
here), from the compiler's resource remarks and the assembly: the projection kernel with and without currents -- no
scratch, no spilled registers, at most 128 VGPRs and four wavefronts per SIMD, an LDS footprint that lets four workgroups
share a compute unit, and one loop that accumulates: it reads LDS and nothing else, and holds no sine and no cosine --,
the shell and finish passes, and no atomics anywhere."""
import re

import pytest

from kernel_build import SRC, device_compile
from psa_amd import _hip

LDS_PER_CU = 160 * 1024


def test_makefile_lists_the_sources():
    mk = (SRC / "Makefile").read_text()
    srcs = next(ln for ln in mk.splitlines() if ln.startswith("SRCS"))
    assert " lattice.hip" in srcs and " api_lattice.hip" in srcs
    assert re.search(r"for f in [^;]*\blattice\b[^;]*; do", mk)               # the asm list
    assert all((SRC / f).is_file() for f in srcs.split(":=")[1].split())


@pytest.fixture(scope="module")
def compiled():
    c = device_compile("lattice.hip")
    print(c.usage)
    return c.usage, c.asm


def test_lattice_kernels_resources(compiled):
    usage, asm = compiled
    assert len(usage) == 5
    # the factor table, the staged (w, w v), the staged (s_hi, s_lo) of three axes, the tile's entries
    lds = _hip.LAT_TABLE * 8 + _hip.LAT_ATOMS * 16 + 3 * _hip.LAT_ATOMS * 8 + (_hip.LAT_MAX_ENTRIES + 1) * 2
    for nc in (1, 4):
        name, u = next((k, v) for k, v in usage.items() if f"lattice_project_kernelILi{nc}EE" in k)
        assert u["ScratchSize [bytes/lane]"] == 0 and u["VGPRs Spill"] == 0 and u["SGPRs Spill"] == 0, (name, u)
        assert u["VGPRs"] + u["AGPRs"] <= 128 and u["Occupancy [waves/SIMD]"] >= 4, (name, u)
        assert u["LDS Size [bytes/block]"] == lds and 2 * lds <= LDS_PER_CU, (name, u)
        assert 4 * lds <= LDS_PER_CU, (name, u)                               # ... and the four that make 4 waves per SIMD
        body = asm[asm.index(name + ":"):]
        body = body[:body.index("s_endpgm")]
        blocks = re.split(r"\n\.LBB\d+_\d+:", body)
        # the accumulating loop: the block that gathers table entries (8-byte LDS reads) and holds the FMAs; nothing else
        # in the kernel reads the table
        hot = [b for b in blocks if b.count("ds_read_b64") >= 3 * _hip.LAT_KS // _hip.LAT_THREADS and "v_fmac_f32" in b]
        assert len(hot) >= 1, name                                            # (the compiler may unroll it: every copy is held)
        for h in hot:
            fmas = h.count("v_fmac_f32") + h.count("v_fma_f32") + h.count("v_pk_fma_f32")
            print(f"NC = {nc}: an accumulating block holds {fmas} FMAs, {h.count('v_mul_f32')} multiplications, "
                  f"{h.count('ds_read')} LDS reads")
            assert fmas >= (2 * nc + 4) * (_hip.LAT_KS // _hip.LAT_THREADS), name  # 2 NC accumulations + two complex products per unit
            assert "v_sin_f32" not in h and "v_cos_f32" not in h, name
            assert "global_load" not in h and "buffer_load" not in h and "flat_load" not in h, name
            assert "ds_write" not in h and "s_barrier" not in h, name
        # the transcendentals sit in the build step: one sine and one cosine per entry
        build = [b for b in blocks if "v_sin_f32" in b]
        assert build and all(b.count("v_sin_f32") == b.count("v_cos_f32") == 1 and "ds_write_b64" in b for b in build), name
        name, u = next((k, v) for k, v in usage.items() if f"lattice_shell_kernelILi{nc}EE" in k)
        assert u["ScratchSize [bytes/lane]"] == 0 and u["VGPRs Spill"] == 0 and u["SGPRs Spill"] == 0, (name, u)
        assert u["VGPRs"] + u["AGPRs"] <= 128 and u["LDS Size [bytes/block]"] == 0, (name, u)
    name, u = next((k, v) for k, v in usage.items() if "lattice_finish_kernel" in k)
    assert u["ScratchSize [bytes/lane]"] == 0 and u["VGPRs Spill"] == 0, (name, u)
    assert "scratch_" not in asm
    assert "atomic" not in asm and "ds_add" not in asm                        # no atomics anywhere
