"""The contraction kernel of the mode-projected SED (psa_amd/csrc/modes.hip) as the compiler builds it for gfx950 (hipcc
cross-compiles here): no scratch, no spilled registers in any of its four tiles (8, 16, 24, 32 modes per pass), the
LDS tile as planned (64 frequencies x (4 k-vectors x MT + 1) floats), enough wavefronts per SIMD to hide the row loads,
and the coefficients through uniform loads."""
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


def test_makefile_lists_the_sources():
    mk = (SRC / "Makefile").read_text()
    srcs = next(ln for ln in mk.splitlines() if ln.startswith("SRCS"))
    assert " modes.hip" in srcs and " api_modes.hip" in srcs
    assert re.search(r"for f in [^;]*\bmodes\b[^;]*; do", mk)                 # the asm list


def test_mode_power_kernels_use_no_scratch(tmp_path):
    if not Path(HIPCC).exists():
        pytest.skip("no hipcc")
    res = subprocess.run([HIPCC, *_flags(), "-S", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", str(SRC / "modes.hip"),
                          "-o", str(tmp_path / "k.s")], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-2000:]
    blocks = re.split(r"remark: [^\n]*Function Name: ", res.stderr)[1:]
    usage = {}
    for b in blocks:
        name = b.split()[0]
        usage[name] = {k: int(v) for k, v in re.findall(
            r"(ScratchSize \[bytes/lane\]|VGPRs Spill|SGPRs Spill|VGPRs|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\d+)", b)}
    kernels = {k: v for k, v in usage.items() if "mode_power_kernel" in k}
    print(kernels)
    assert len(kernels) == 4
    for mt in (8, 16, 24, 32):
        name, u = next((k, v) for k, v in kernels.items() if f"mode_power_kernelILi{mt}E" in k)
        assert u["ScratchSize [bytes/lane]"] == 0 and u["VGPRs Spill"] == 0 and u["SGPRs Spill"] == 0, (name, u)
        assert u["VGPRs"] <= 128 and u["Occupancy [waves/SIMD]"] >= 4, (name, u)
        assert u["LDS Size [bytes/block]"] == 64 * (4 * mt + 1) * 4, (name, u)
    asm = (tmp_path / "k.s").read_text()
    assert "scratch_" not in asm
    assert "s_load_dwordx" in asm and "v_fma" in asm                          # coefficients through scalar loads
