"""The peak kernels (psa_amd/csrc/peaks.hip) as the compiler builds them for gfx950 (hipcc cross-compiles here), from the
compiler's resource remarks alone: no scratch, no spilled registers; peak_find without LDS and light enough for eight
wavefronts per SIMD (it only streams); peak_fit with its planned 4 x 16 KiB of LDS -- one window of at most 4095 floats
per wavefront -- and room for two workgroups per compute unit: 2 x 64 KiB within the 160 KiB of LDS, and two wavefronts
per SIMD, each workgroup placing one on each of the four."""
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


def test_peak_kernels_resources(tmp_path):
    if not Path(HIPCC).exists():
        pytest.skip("no hipcc")
    res = subprocess.run([HIPCC, *_flags(), "-S", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", str(SRC / "peaks.hip"),
                          "-o", str(tmp_path / "k.s")], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-2000:]
    blocks = re.split(r"remark: [^\n]*Function Name: ", res.stderr)[1:]
    usage = {}
    for b in blocks:
        usage[b.split()[0]] = {k: int(v) for k, v in re.findall(
            r"(ScratchSize \[bytes/lane\]|VGPRs Spill|SGPRs Spill|VGPRs|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\d+)", b)}
    print(usage)
    find = next(v for k, v in usage.items() if "peak_find_kernel" in k)
    fit = next(v for k, v in usage.items() if "peak_fit_kernel" in k)
    assert len(usage) == 2
    for u in (find, fit):
        assert u["ScratchSize [bytes/lane]"] == 0 and u["VGPRs Spill"] == 0 and u["SGPRs Spill"] == 0, u
    assert find["LDS Size [bytes/block]"] == 0 and find["Occupancy [waves/SIMD]"] >= 8, find
    assert fit["LDS Size [bytes/block]"] == 4 * 4096 * 4, fit
    assert LDS_PER_CU // fit["LDS Size [bytes/block]"] >= 2 and fit["Occupancy [waves/SIMD]"] >= 2 and fit["VGPRs"] <= 256, fit
