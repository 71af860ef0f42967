"""The segment-averaging contraction kernel (psa_amd/csrc/modes_welch.hip) as the compiler builds it for gfx950 (hipcc
cross-compiles here), from the compiler's resource remarks alone: its four tiles (8, 16, 24, 32 modes per pass) without
scratch and without spilled registers, within the 128 VGPRs that four wavefronts per SIMD allow, and with the planned LDS
-- the hand-over tile of the parent kernel, 64 frequencies x (4 k-vectors x MT + 1) floats, which also holds the running
sum over the segments, so that four workgroups of the widest tile (4 x 33024 bytes) still share a compute unit's 160 KiB."""
import re
import shutil
import subprocess
from pathlib import Path

import pytest

from conftest import ROOT

HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
SRC = ROOT / "psa_amd" / "csrc"
LDS_PER_CU = 160 * 1024


def _flags():
    line = next(ln for ln in (SRC / "Makefile").read_text().splitlines() if ln.startswith("CXXFLAGS"))
    cont = (SRC / "Makefile").read_text().split(line)[1].splitlines()[1]
    raw = (line.split(":=")[1].rstrip("\\") + " " + cont).split()
    return [f.replace("$(ARCH)", "gfx950").replace("$(ROOT)", str(ROOT)) for f in raw if not f.startswith("-W")]


def test_mode_welch_kernels_resources(tmp_path):
    if not Path(HIPCC).exists():
        pytest.skip("no hipcc")
    res = subprocess.run([HIPCC, *_flags(), "-S", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage",
                          str(SRC / "modes_welch.hip"), "-o", str(tmp_path / "k.s")], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-2000:]
    blocks = re.split(r"remark: [^\n]*Function Name: ", res.stderr)[1:]
    usage = {}
    for b in blocks:
        usage[b.split()[0]] = {k: int(v) for k, v in re.findall(
            r"(ScratchSize \[bytes/lane\]|VGPRs Spill|SGPRs Spill|VGPRs|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\d+)", b)}
    print(usage)
    assert len(usage) == 4 and all("mode_welch_kernel" in k and "mode_power_kernel" not in k for k in usage)
    for mt in (8, 16, 24, 32):
        name, u = next((k, v) for k, v in usage.items() if f"mode_welch_kernelILi{mt}E" in k)
        assert u["ScratchSize [bytes/lane]"] == 0 and u["VGPRs Spill"] == 0 and u["SGPRs Spill"] == 0, (name, u)
        assert u["VGPRs"] <= 128 and u["Occupancy [waves/SIMD]"] >= 4, (name, u)
        assert u["LDS Size [bytes/block]"] == 64 * (4 * mt + 1) * 4, (name, u)
        assert 4 * u["LDS Size [bytes/block]"] <= LDS_PER_CU, (name, u)
