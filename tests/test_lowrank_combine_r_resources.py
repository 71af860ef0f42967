"""Build-time shape of the real-weights low-rank combine (lowrank_combine_r_kernel, lowrank_combine.hip): no scratch
and no spills (its 64 node values per thread live in registers), at most 256 VGPRs, per four rows exactly one
v_pk_fma_f32 per node and row and one ds_read_b128 per four nodes and row, and per output element the phase sequence
of two multiplies and two FMAs -- no second packed FMA per node, no scalar-FMA fallback for the node sum."""
import re
import subprocess
from pathlib import Path

import pytest

from test_lowrank_combine_resources import HIPCC, SRC, _flags

KERNEL = "lowrank_combine_r_kernel"


def test_lowrank_combine_r_budget(tmp_path):
    if not Path(HIPCC).exists():
        pytest.skip("no hipcc")
    asm = tmp_path / "k.s"
    res = subprocess.run([HIPCC, *_flags(), "-S", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage",
                          str(SRC / "lowrank_combine.hip"), "-o", str(asm)], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-2000:]
    usage = res.stderr[res.stderr.index(KERNEL):]
    nxt = usage.find("Function Name", 1)
    usage = usage if nxt < 0 else usage[:nxt]
    scratch = int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", usage).group(1))
    spills = int(re.search(r"VGPRs Spill: (\d+)", usage).group(1))
    vgprs = int(re.search(r" VGPRs: (\d+)", usage).group(1))
    lds = int(re.search(r"LDS Size \[bytes/block\]: (\d+)", usage).group(1))
    print(f"{KERNEL}: {vgprs} VGPRs, {spills} spilled, {scratch} B scratch per lane, {lds} B LDS")
    assert scratch == 0 and spills == 0 and vgprs <= 256, (scratch, spills, vgprs)
    assert lds == 64 * 64 * 4 + 64 * 8, lds                     # 64 rows of L and their phases
    text = asm.read_text()
    body = text[re.search(rf"^_ZN3psa\d+{KERNEL}\w*:", text, re.M).start():]
    body = body[:body.index("s_endpgm")]
    assert "scratch_" not in body
    assert body.count("v_pk_fma_f32") == 4 * 64                 # four rows x 64 nodes, one each
    assert body.count("ds_read_b128") == 4 * 16                 # four rows x 64 nodes / 4
    # the phase: two multiplies and two FMAs per stored element, four stores in the row loop
    n_fma = len(re.findall(r"\bv_(?:fma|fmac)_f32", body))
    n_mul = len(re.findall(r"\bv_mul_f32", body))
    assert n_fma == 8 and n_mul == 8, (n_fma, n_mul)
