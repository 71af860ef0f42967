"""The build-time kernel tests' one compile: a source of psa_amd/csrc device-compiled for gfx950 with the Makefile's
flags (hipcc cross-compiles without a GPU), once per source and process, whichever tests ask for it."""
import functools
import re
import shutil
import subprocess
import tempfile
from pathlib import Path
from typing import NamedTuple

import pytest

from conftest import ROOT

HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
SRC = ROOT / "psa_amd" / "csrc"


def flags():
    """CXXFLAGS of the Makefile (two lines), without its warning options"""
    line = next(ln for ln in (SRC / "Makefile").read_text().splitlines() if ln.startswith("CXXFLAGS"))
    cont = (SRC / "Makefile").read_text().split(line)[1].splitlines()[1]
    raw = (line.split(":=")[1].rstrip("\\") + " " + cont).split()
    return [f.replace("$(ARCH)", "gfx950").replace("$(ROOT)", str(ROOT)) for f in raw if not f.startswith("-W")]


class Compiled(NamedTuple):
    stderr: str      # the compiler's resource remarks as it printed them
    usage: dict      # mangled kernel name -> {remark: value}
    asm: str         # the assembly


@functools.lru_cache(maxsize=None)
def device_compile(source):
    """Compiled of psa_amd/csrc/<source>; skips the calling test when there is no hipcc"""
    if not Path(HIPCC).exists():
        pytest.skip("no hipcc")
    with tempfile.TemporaryDirectory() as tmp:
        out = Path(tmp) / "k.s"
        res = subprocess.run([HIPCC, *flags(), "-S", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", str(SRC / source),
                              "-o", str(out)], capture_output=True, text=True, timeout=600)
        assert res.returncode == 0, res.stderr[-2000:]
        asm = out.read_text()
    usage = {}
    for b in re.split(r"remark: [^\n]*Function Name: ", res.stderr)[1:]:
        usage[b.split()[0]] = {k: int(v) for k, v in re.findall(
            r"(ScratchSize \[bytes/lane\]|VGPRs Spill|SGPRs Spill|VGPRs|AGPRs|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\d+)", b)}
    return Compiled(res.stderr, usage, asm)
