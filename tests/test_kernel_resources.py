"""Register budgets the planes kernels rely on, checked at build time (hipcc cross-compiles gfx950 here): they wait
for their LDS-DMA with a COUNTED `s_waitcnt vmcnt(N)`, and scratch loads / stores are vector-memory operations that
count too -- a kernel that spills a single register inside its loop would read LDS before the data has landed.  The
256-row kernel sits at 250 of the 256 VGPRs two wavefronts per SIMD may have, so a compiler update can tip it."""
import re

import pytest

from kernel_build import device_compile


@pytest.mark.parametrize("source, max_vgprs", [("k1_planes_wide.hip", 256), ("k1_planes_lw.hip", 168), ("k1_planes_diff.hip", 256),
                                               ("k1_planes.hip", 256)])
def test_counted_vmcnt_kernels_use_no_scratch(source, max_vgprs):
    res = device_compile(source)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", res.stderr)]
    spills = [int(x) for x in re.findall(r"VGPRs Spill: (\d+)", res.stderr)]
    vgprs = [int(x) for x in re.findall(r" VGPRs: (\d+)", res.stderr)]
    assert scratch and all(s == 0 for s in scratch), res.stderr[-1500:]
    assert all(s == 0 for s in spills) and all(v <= max_vgprs for v in vgprs), (spills, vgprs)
    assert "scratch_" not in res.asm
