"""Build-time shape of the real-weights low-rank combine (lowrank_combine_r_kernel, lowrank_combine.hip): no scratch
and no spills (its 64 node values per thread live in registers), at most 256 VGPRs, per four rows exactly one
v_pk_fma_f32 per node and row and one ds_read_b128 per four nodes and row, and per output element the phase sequence
of two multiplies and two FMAs -- no second packed FMA per node, no scalar-FMA fallback for the node sum."""
import re

from kernel_build import device_compile

KERNEL = "lowrank_combine_r_kernel"


def test_lowrank_combine_r_budget():
    _, usage, text = device_compile("lowrank_combine.hip")
    u = next(v for k, v in usage.items() if KERNEL in k)
    scratch, spills, vgprs, lds = u["ScratchSize [bytes/lane]"], u["VGPRs Spill"], u["VGPRs"], u["LDS Size [bytes/block]"]
    print(f"{KERNEL}: {vgprs} VGPRs, {spills} spilled, {scratch} B scratch per lane, {lds} B LDS")
    assert scratch == 0 and spills == 0 and vgprs <= 256, (scratch, spills, vgprs)
    assert lds == 64 * 64 * 4 + 64 * 8, lds                     # 64 rows of L and their phases
    body = text[re.search(rf"^_ZN3psa\d+{KERNEL}\w*:", text, re.M).start():]
    body = body[:body.index("s_endpgm")]
    assert "scratch_" not in body
    assert body.count("v_pk_fma_f32") == 4 * 64                 # four rows x 64 nodes, one each
    assert body.count("ds_read_b128") == 4 * 16                 # four rows x 64 nodes / 4
    # the phase: two multiplies and two FMAs per stored element, four stores in the row loop
    n_fma = len(re.findall(r"\bv_(?:fma|fmac)_f32", body))
    n_mul = len(re.findall(r"\bv_mul_f32", body))
    assert n_fma == 8 and n_mul == 8, (n_fma, n_mul)
