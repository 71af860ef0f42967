"""Build-time shape of the 48-node low-rank route's kernels: the 48-node pair launch (k1_lowrank_n48_kernel,
k1_lowrank_n48.hip) holds 33 accumulator tiles per wavefront in either role with two wavefronts per SIMD -- no scratch, no
spills, at most 256 registers --, its ring is all 160 KiB of LDS, and its body holds role A's eight unrolled stages (one
fold) and role B's four at (6 + 5) x 3 = 33 MFMAs per wavefront each; the 48-node table kernels and both instantiations of
the combine are spill-free."""
import re

from kernel_build import device_compile

KERNEL = "k1_lowrank_n48_kernel"
MFMA = "v_mfma_f32_16x16x32_f16"


def _no_spill(u):
    assert u["ScratchSize [bytes/lane]"] == 0 and u["VGPRs Spill"] == 0 and u["SGPRs Spill"] == 0, u


def test_lowrank_n48_budget():
    _, usage, text = device_compile("k1_lowrank_n48.hip")
    u = next(v for k, v in usage.items() if KERNEL in k)
    print(f"{KERNEL}: {u['VGPRs']} VGPRs, {u['AGPRs']} AGPRs, {u['VGPRs Spill']} spilled, {u['ScratchSize [bytes/lane]']} B scratch "
          f"per lane, {u['LDS Size [bytes/block]']} B LDS")
    _no_spill(u)
    assert u["VGPRs"] + u["AGPRs"] <= 256, u
    assert u["Occupancy [waves/SIMD]"] >= 2, u
    assert u["LDS Size [bytes/block]"] == 160 * 1024, u
    body = text[re.search(rf"^_ZN3psa\d+{KERNEL}\w*:", text, re.M).start():]
    body = body[:body.index("s_endpgm")]
    assert body.count(MFMA) == (8 + 4) * 33
    # each role's body on its own: the MFMAs between one role's stores and the other's are one role's unrolled stages,
    # eight of role A (one fold) and four of role B, 33 each
    runs, n = [], 0
    for line in body.splitlines():
        if MFMA in line:
            n += 1
        elif "global_store_dwordx2" in line and n:
            runs.append(n)
            n = 0
    assert n == 0, "MFMAs behind the last store"
    assert sorted(runs) == [4 * 33, 8 * 33], runs


def test_n48_table_kernels_are_spill_free():
    _, usage, _ = device_compile("k1_planes_diff.hip")
    tables = {k: v for k, v in usage.items() if "diff_n48_table_kernel" in k or "node_table_n48_kernel" in k}
    assert len(tables) == 3, list(usage)
    for u in tables.values():
        _no_spill(u)


def test_combine_instantiations_are_spill_free():
    _, usage, text = device_compile("lowrank_combine.hip")
    both = {k: v for k, v in usage.items() if "lowrank_combine_r_kernel" in k}
    assert len(both) == 2 and any("ILi48E" in k for k in both) and any("ILi64E" in k for k in both), list(usage)
    for u in both.values():
        _no_spill(u)
    # one packed FMA per node and row, four rows at a time: 48 against 64
    count = {}
    for name in both:
        body = text[text.index(name + ":"):]
        count[48 if "ILi48E" in name else 64] = body[:body.index("s_endpgm")].count("v_pk_fma_f32")
    assert count[48] * 64 == count[64] * 48, count
