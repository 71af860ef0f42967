"""The density-of-states kernels (psa_amd/csrc/vdos.hip) as the compiler builds them for gfx950 (hipcc cross-compiles
here): no scratch, no spilled registers -- both stream through HBM, and a spill would add traffic to exactly the loop
that is bound by it -- and the gather's LDS tile as planned (192 columns x 65 floats)."""
from kernel_build import device_compile


def test_vdos_kernels_use_no_scratch():
    _, usage, asm = device_compile("vdos.hip")
    kernels = {k: v for k, v in usage.items() if "vdos_" in k and "kernel" in k}
    print(kernels)
    assert any("vdos_gather_kernel" in k for k in kernels) and any("vdos_power_kernel" in k for k in kernels)
    assert len(kernels) == 4
    for name, u in kernels.items():
        assert u["ScratchSize [bytes/lane]"] == 0 and u["VGPRs Spill"] == 0 and u["SGPRs Spill"] == 0, (name, u)
        assert u["VGPRs"] <= 128, (name, u)                      # at least four wavefronts per SIMD
    gather = next(v for k, v in kernels.items() if "vdos_gather_kernel" in k)
    assert gather["LDS Size [bytes/block]"] == 192 * 65 * 4
    assert "scratch_" not in asm
