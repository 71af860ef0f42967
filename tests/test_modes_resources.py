"""The contraction kernel of the mode-projected SED (psa_amd/csrc/modes.hip) as the compiler builds it for gfx950 (hipcc
cross-compiles here), from the compiler's resource remarks and the assembly: its four tiles (8, 16, 24, 32 modes per
pass), each without (SUM = false) and with (SUM = true) the running sum over Welch segments -- no scratch, no spilled
registers, within the 128 VGPRs that four wavefronts per SIMD allow, the LDS tile as planned (64 frequencies x
(4 k-vectors x MT + 1) floats: the hand-over tile also holds the running sum, so that four workgroups of the widest tile,
4 x 33024 bytes, still share a compute unit's 160 KiB), the coefficients through uniform loads, and neither instantiation
above the registers or below the occupancy of the separate kernel it replaced."""
import re

import pytest

from kernel_build import SRC, device_compile
LDS_PER_CU = 160 * 1024
# (VGPRs, wavefronts per SIMD) of mode_power_kernel<MT> and mode_welch_kernel<MT> before they became one template
BEFORE = {(8, False): (38, 8), (16, False): (54, 8), (24, False): (66, 6), (32, False): (86, 4),
          (8, True): (54, 8), (16, True): (78, 6), (24, True): (96, 5), (32, True): (94, 4)}


def test_makefile_lists_the_sources():
    mk = (SRC / "Makefile").read_text()
    srcs = next(ln for ln in mk.splitlines() if ln.startswith("SRCS"))
    assert " modes.hip" in srcs and " api_modes.hip" in srcs
    assert re.search(r"for f in [^;]*\bmodes\b[^;]*; do", mk)                 # the asm list
    assert all((SRC / f).is_file() for f in srcs.split(":=")[1].split())


@pytest.fixture(scope="module")
def compiled():
    """(resource remarks per kernel, assembly) of modes.hip, compiled once"""
    c = device_compile("modes.hip")
    print(c.usage)
    return c.usage, c.asm


def _check(compiled, summed):
    usage, asm = compiled
    assert len(usage) == 8 and all("mode_power_kernel" in k for k in usage)
    for mt in (8, 16, 24, 32):
        vgprs, waves = BEFORE[mt, summed]
        name, u = next((k, v) for k, v in usage.items() if f"mode_power_kernelILi{mt}ELb{int(summed)}EE" in k)
        assert u["ScratchSize [bytes/lane]"] == 0 and u["VGPRs Spill"] == 0 and u["SGPRs Spill"] == 0, (name, u)
        assert u["VGPRs"] <= 128 and u["Occupancy [waves/SIMD]"] >= 4, (name, u)
        assert u["LDS Size [bytes/block]"] == 64 * (4 * mt + 1) * 4, (name, u)
        assert 4 * u["LDS Size [bytes/block]"] <= LDS_PER_CU, (name, u)
        assert u["VGPRs"] <= vgprs and u["Occupancy [waves/SIMD]"] >= waves, (name, u)
    assert "scratch_" not in asm
    assert "s_load_dwordx" in asm and "v_fma" in asm                          # coefficients through scalar loads


def test_mode_power_kernels_use_no_scratch(compiled):
    """SUM = false: the former mode_power_kernel<MT>"""
    _check(compiled, False)


def test_mode_power_sum_kernels_resources(compiled):
    """SUM = true: the former mode_welch_kernel<MT>"""
    _check(compiled, True)
