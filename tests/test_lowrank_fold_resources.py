"""Build-time shape of the folded low-rank route's kernels: the folded pair launch (k1_lowrank_fold_kernel,
k1_lowrank_fold.hip) holds 36 accumulator tiles per wavefront in either role with two wavefronts per SIMD -- no scratch, no
spills, at most 256 registers --, its ring is all 160 KiB of LDS, and its body holds role A's eight unrolled stages (one
fold) and role B's four at 36 MFMAs per wavefront each; the two-product instantiations of the loader-wavefront kernel
(k1_planes_lw_kernel<., true>, k1_planes_lw.hip) and the folded table kernel are spill-free."""
import re

from kernel_build import device_compile

KERNEL = "k1_lowrank_fold_kernel"
MFMA = "v_mfma_f32_16x16x32_f16"


def _no_spill(u):
    assert u["ScratchSize [bytes/lane]"] == 0 and u["VGPRs Spill"] == 0 and u["SGPRs Spill"] == 0, u


def test_lowrank_fold_budget():
    _, usage, text = device_compile("k1_lowrank_fold.hip")
    u = next(v for k, v in usage.items() if KERNEL in k)
    print(f"{KERNEL}: {u['VGPRs']} VGPRs, {u['AGPRs']} AGPRs, {u['VGPRs Spill']} spilled, {u['ScratchSize [bytes/lane]']} B scratch "
          f"per lane, {u['LDS Size [bytes/block]']} B LDS")
    _no_spill(u)
    assert u["VGPRs"] + u["AGPRs"] <= 256, u
    assert u["Occupancy [waves/SIMD]"] >= 2, u
    assert u["LDS Size [bytes/block]"] == 160 * 1024, u
    body = text[re.search(rf"^_ZN3psa\d+{KERNEL}\w*:", text, re.M).start():]
    body = body[:body.index("s_endpgm")]
    assert body.count(MFMA) == (8 + 4) * 36


def test_two_product_node_pass_is_spill_free():
    _, usage, text = device_compile("k1_planes_lw.hip")
    two = {k: v for k, v in usage.items() if re.search(r"k1_planes_lw_kernelILb[01]ELb1EE", k)}
    three = {k: v for k, v in usage.items() if re.search(r"k1_planes_lw_kernelILb[01]ELb0EE", k)}
    assert len(two) == 2 and len(three) == 2, list(usage)
    for name, u in two.items():
        print(f"{name}: {u['VGPRs']} VGPRs")
        _no_spill(u)
        assert u["VGPRs"] <= 168 and u["Occupancy [waves/SIMD]"] >= 3, u
    # two MFMAs per chain against three: per unrolled stage 4 row tiles x 3 components
    for name in two:
        body = text[text.index(name + ":"):]
        body = body[:body.index("s_endpgm")]
        other = name.replace("ELb1EE", "ELb0EE")
        ref = text[text.index(other + ":"):]
        ref = ref[:ref.index("s_endpgm")]
        assert body.count(MFMA) * 3 == ref.count(MFMA) * 2 and body.count(MFMA) % 24 == 0, (body.count(MFMA), ref.count(MFMA))


def test_fold_table_kernel_is_spill_free():
    _, usage, _ = device_compile("k1_planes_diff.hip")
    fold = {k: v for k, v in usage.items() if "diff_fold_table_kernel" in k}
    assert len(fold) == 2, list(usage)
    for u in fold.values():
        _no_spill(u)
