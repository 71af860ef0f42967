"""The peak kernels (psa_amd/csrc/peaks.hip) as the compiler builds them for gfx950 (hipcc cross-compiles here), from the
compiler's resource remarks alone: no scratch, no spilled registers; peak_find without LDS and light enough for eight
wavefronts per SIMD (it only streams); peak_fit with its planned 4 x 16 KiB of LDS -- one window of at most 4095 floats
per wavefront -- and room for two workgroups per compute unit: 2 x 64 KiB within the 160 KiB of LDS, and two wavefronts
per SIMD, each workgroup placing one on each of the four."""
from kernel_build import device_compile

LDS_PER_CU = 160 * 1024


def test_peak_kernels_resources():
    usage = device_compile("peaks.hip").usage
    print(usage)
    find = next(v for k, v in usage.items() if "peak_find_kernel" in k)
    fit = next(v for k, v in usage.items() if "peak_fit_kernel" in k)
    assert len(usage) == 2
    for u in (find, fit):
        assert u["ScratchSize [bytes/lane]"] == 0 and u["VGPRs Spill"] == 0 and u["SGPRs Spill"] == 0, u
    assert find["LDS Size [bytes/block]"] == 0 and find["Occupancy [waves/SIMD]"] >= 8, find
    assert fit["LDS Size [bytes/block]"] == 4 * 4096 * 4, fit
    assert LDS_PER_CU // fit["LDS Size [bytes/block]"] >= 2 and fit["Occupancy [waves/SIMD]"] >= 2 and fit["VGPRs"] <= 256, fit
