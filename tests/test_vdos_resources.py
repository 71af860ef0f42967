"""The density-of-states kernels (psa_amd/csrc/vdos.hip) as the compiler builds them for gfx950 (hipcc cross-compiles
here): no scratch, no spilled registers -- both stream through HBM, and a spill would add traffic to exactly the loop
that is bound by it -- and the gather's LDS tile as planned (192 columns x 65 floats)."""
import re
import shutil
import subprocess
from pathlib import Path

import pytest

from conftest import ROOT

HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
SRC = ROOT / "psa_amd" / "csrc"


def _flags():
    line = next(ln for ln in (SRC / "Makefile").read_text().splitlines() if ln.startswith("CXXFLAGS"))
    cont = (SRC / "Makefile").read_text().split(line)[1].splitlines()[1]
    raw = (line.split(":=")[1].rstrip("\\") + " " + cont).split()
    return [f.replace("$(ARCH)", "gfx950").replace("$(ROOT)", str(ROOT)) for f in raw if not f.startswith("-W")]


def test_vdos_kernels_use_no_scratch(tmp_path):
    if not Path(HIPCC).exists():
        pytest.skip("no hipcc")
    res = subprocess.run([HIPCC, *_flags(), "-S", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", str(SRC / "vdos.hip"),
                          "-o", str(tmp_path / "k.s")], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-2000:]
    blocks = re.split(r"remark: [^\n]*Function Name: ", res.stderr)[1:]
    usage = {}
    for b in blocks:
        name = b.split()[0]
        usage[name] = {k: int(v) for k, v in re.findall(r"(ScratchSize \[bytes/lane\]|VGPRs Spill|SGPRs Spill|VGPRs|LDS Size \[bytes/block\]): (\d+)", b)}
    kernels = {k: v for k, v in usage.items() if "vdos_" in k and "kernel" in k}
    print(kernels)
    assert any("vdos_gather_kernel" in k for k in kernels) and any("vdos_power_kernel" in k for k in kernels)
    assert len(kernels) == 4
    for name, u in kernels.items():
        assert u["ScratchSize [bytes/lane]"] == 0 and u["VGPRs Spill"] == 0 and u["SGPRs Spill"] == 0, (name, u)
        assert u["VGPRs"] <= 128, (name, u)                      # at least four wavefronts per SIMD
    gather = next(v for k, v in kernels.items() if "vdos_gather_kernel" in k)
    assert gather["LDS Size [bytes/block]"] == 192 * 65 * 4
    assert "scratch_" not in (tmp_path / "k.s").read_text()
