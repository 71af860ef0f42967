"""The dynamic-spectra kernels (psa_amd/csrc/dynamic.hip) as the compiler builds them for gfx950 (hipcc cross-compiles
here), from the compiler's resource remarks and the assembly: the projection kernel with and without currents, the power
pass of each, and the sine / cosine sweep -- no scratch, no spilled registers, at most 128 VGPRs (four wavefronts per SIMD:
the latency of the transcendentals is covered by the other wavefronts and the lane's second atom), the two LDS images of
a staged tile, the hardware sine and cosine in the one loop that does the work, and no atomics."""
import re

import pytest

from kernel_build import SRC, device_compile
from psa_amd import _hip


def test_makefile_lists_the_sources():
    mk = (SRC / "Makefile").read_text()
    srcs = next(ln for ln in mk.splitlines() if ln.startswith("SRCS"))
    assert " dynamic.hip" in srcs and " api_dynamic.hip" in srcs
    assert re.search(r"for f in [^;]*\bdynamic\b[^;]*; do", mk)               # the asm list
    assert all((SRC / f).is_file() for f in srcs.split(":=")[1].split())


@pytest.fixture(scope="module")
def compiled():
    c = device_compile("dynamic.hip")
    print(c.usage)
    return c.usage, c.asm


def test_dynamic_kernels_resources(compiled):
    usage, asm = compiled
    assert len(usage) == 5
    for nc in (1, 4):
        name, u = next((k, v) for k, v in usage.items() if f"dynamic_project_kernelILi{nc}EE" in k)
        assert u["ScratchSize [bytes/lane]"] == 0 and u["VGPRs Spill"] == 0 and u["SGPRs Spill"] == 0, (name, u)
        assert u["VGPRs"] + u["AGPRs"] <= 128 and u["Occupancy [waves/SIMD]"] >= 4, (name, u)
        # two images of DYN_ATOMS atoms: (x, y, z, w) and, with currents, (w v_x, w v_y, w v_z, 0)
        assert u["LDS Size [bytes/block]"] == 2 * (2 if nc == 4 else 1) * _hip.DYN_ATOMS * 16, (name, u)
        body = asm[asm.index(name + ":"):]
        body = body[:body.index("s_endpgm")]
        hot = [b for b in re.split(r"\n\.LBB\d+_\d+:", body) if "v_sin_f32" in b]
        assert len(hot) == 1, (name, len(hot))                                # one loop holds the transcendentals
        assert hot[0].count("v_sin_f32") == 2 and hot[0].count("v_cos_f32") == 2, name    # two atoms in flight
        assert "global_load" not in hot[0] and "buffer_load" not in hot[0], name          # trajectory data only from LDS
        assert hot[0].count("ds_read") <= 4, name                             # 16-byte reads of the staged atoms
        name, u = next((k, v) for k, v in usage.items() if f"dynamic_power_kernelILi{nc}EE" in k)
        assert u["ScratchSize [bytes/lane]"] == 0 and u["VGPRs Spill"] == 0 and u["SGPRs Spill"] == 0, (name, u)
        assert u["VGPRs"] + u["AGPRs"] <= 128 and u["LDS Size [bytes/block]"] == 0, (name, u)
    name, u = next((k, v) for k, v in usage.items() if "dynamic_sincos_kernel" in k)
    assert u["ScratchSize [bytes/lane]"] == 0 and u["VGPRs Spill"] == 0, (name, u)
    assert "scratch_" not in asm
    assert "global_atomic" not in asm and "ds_add" not in asm and "flat_atomic" not in asm     # no atomics anywhere
