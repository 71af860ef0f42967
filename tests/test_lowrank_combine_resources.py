"""Build-time shape of the packed low-rank combine (lowrank_combine.hip): no scratch and no spills (its 64 node values
per thread live in registers), at most 256 VGPRs, and per pair of rows exactly two v_pk_fma_f32 per node and row --
the fmaf pairs of the scalar combine, packed, with no scalar-FMA fallback."""
import re
import shutil
import subprocess
from pathlib import Path

import pytest

from conftest import ROOT

HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
SRC = ROOT / "psa_amd" / "csrc"


def _flags():
    text = (SRC / "Makefile").read_text()
    line = next(ln for ln in text.splitlines() if ln.startswith("CXXFLAGS"))
    cont = text.split(line)[1].splitlines()[1]
    raw = (line.split(":=")[1].rstrip("\\") + " " + cont).split()
    return [f.replace("$(ARCH)", "gfx950").replace("$(ROOT)", str(ROOT)) for f in raw if not f.startswith("-W")]


def test_lowrank_combine_budget(tmp_path):
    if not Path(HIPCC).exists():
        pytest.skip("no hipcc")
    asm = tmp_path / "k.s"
    res = subprocess.run([HIPCC, *_flags(), "-S", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage",
                          str(SRC / "lowrank_combine.hip"), "-o", str(asm)], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-2000:]
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", res.stderr)]
    spills = [int(x) for x in re.findall(r"VGPRs Spill: (\d+)", res.stderr)]
    vgprs = [int(x) for x in re.findall(r" VGPRs: (\d+)", res.stderr)]
    assert scratch and all(s == 0 for s in scratch), res.stderr[-1500:]
    assert all(s == 0 for s in spills) and all(v <= 256 for v in vgprs), (spills, vgprs)
    text = asm.read_text()
    assert "scratch_" not in text
    comb = text[text.index("lowrank_combine_v_kernel"):]
    comb = comb[:comb.index("s_endpgm")]
    assert comb.count("v_pk_fma_f32") == 4 * 64 and "v_fma_f32" not in comb
