"""Build-time shape of the low-rank route's pair launch (k1_lowrank_pair_kernel, k1_lowrank_pair.hip): two wavefronts per
SIMD hold 30 (role A) or 42 (role B) accumulator tiles in registers -- no scratch, no spills, at most 256 VGPRs, no
scratch_ instruction in the kernel's assembly --, the ring is all 160 KiB of LDS, and the body holds role A's 40 unrolled
stages and role B's four at 42 MFMAs per wavefront each."""
import re

from kernel_build import device_compile

KERNEL = "k1_lowrank_pair_kernel"


def test_lowrank_pair_budget():
    _, usage, text = device_compile("k1_lowrank_pair.hip")
    u = next(v for k, v in usage.items() if KERNEL in k)
    scratch, spills, vgprs, lds = u["ScratchSize [bytes/lane]"], u["VGPRs Spill"], u["VGPRs"], u["LDS Size [bytes/block]"]
    print(f"{KERNEL}: {vgprs} VGPRs, {u['AGPRs']} AGPRs, {spills} spilled, {scratch} B scratch per lane, {lds} B LDS")
    assert scratch == 0 and spills == 0 and u["SGPRs Spill"] == 0, (scratch, spills, u["SGPRs Spill"])
    assert vgprs + u["AGPRs"] <= 256, (vgprs, u["AGPRs"])
    assert u["Occupancy [waves/SIMD]"] >= 2, u
    assert lds == 160 * 1024, lds
    body = text[re.search(rf"^_ZN3psa\d+{KERNEL}\w*:", text, re.M).start():]
    body = body[:body.index("s_endpgm")]
    assert "scratch_" not in body
    assert body.count("v_mfma_f32_16x16x32_f16") == (40 + 4) * 42
