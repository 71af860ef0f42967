"""The bond-angle kernels (psa_amd/csrc/angle.hip) as the compiler builds them for gfx950 (hipcc cross-compiles here), from
the compiler's resource remarks and the assembly: no scratch and no spilled registers anywhere; every kernel within 128
registers; the inner block of the neighbour pass -- the block with the most square roots -- reads LDS and loads nothing
from global memory; no global atomic of any kind, no float LDS atomic, and the 32-bit integer LDS add in the angle pass
alone; the Makefile lists the sources; the exported constants are the header's."""
import re

import pytest

from kernel_build import SRC, device_compile
from psa_amd import _hip

KERNELS = ("angle_neighbours_kernel", "angle_hist_kernel")   # the integer reduce: test_hist_reduce_resources.py


def test_makefile_lists_the_sources():
    mk = (SRC / "Makefile").read_text()
    srcs = next(ln for ln in mk.splitlines() if ln.startswith("SRCS"))
    assert " angle.hip" in srcs and " api_angle.hip" in srcs
    assert re.search(r"for f in [^;]*\bangle\b[^;]*; do", mk)                 # the asm list
    assert all((SRC / f).is_file() for f in srcs.split(":=")[1].split())


def test_makefile_object_rule_names_every_header():
    """an object is rebuilt when any header beside the sources changes: a header the rule leaves out gives stale objects"""
    mk = (SRC / "Makefile").read_text()
    rule = next(ln for ln in mk.splitlines() if ln.startswith("$(BUILD)/%.o:"))
    named = set(rule.split(":", 1)[1].split("|")[0].split())
    headers = sorted(p.name for p in SRC.glob("*.h"))
    assert headers and [h for h in headers if h not in named] == []


def test_exported_constants():
    head = (SRC / "psa_ctx.h").read_text()
    for name in ("ANGLE_MAX_NEIGHBOURS", "ANGLE_MAX_BINS"):
        assert int(re.search(rf"constexpr int {name} = (\d+);", head).group(1)) == getattr(_hip, name)
    assert (_hip.ANGLE_MAX_NEIGHBOURS, _hip.ANGLE_MAX_BINS) == (64, 1024)


@pytest.fixture(scope="module")
def compiled():
    c = device_compile("angle.hip")
    print(c.usage)
    return c.usage, c.asm


def _body(asm, name):
    body = asm[asm.index(name + ":"):]
    return body[:body.index("s_endpgm")]


def test_angle_kernels_resources(compiled):
    usage, asm = compiled
    assert len(usage) == len(KERNELS) and all(any(k in name for name in usage) for k in KERNELS)
    for name, u in usage.items():
        assert u["ScratchSize [bytes/lane]"] == 0 and u["VGPRs Spill"] == 0 and u["SGPRs Spill"] == 0, (name, u)
        assert u["VGPRs"] + u["AGPRs"] <= 128, (name, u)
    assert "scratch_" not in asm


def test_inner_neighbour_loop(compiled):
    usage, asm = compiled
    name = next(k for k in usage if "angle_neighbours_kernel" in k)
    blocks = re.split(r"\n\.LBB\d+_\d+:", _body(asm, name))
    roots = [b.count("v_sqrt_f32") + b.count("v_rsq_f32") for b in blocks]
    inner = blocks[roots.index(max(roots))]
    valu = len(re.findall(r"\n\s+v_", inner))
    print(f"the inner block: {max(roots)} roots, {valu} VALU instructions, {len(re.findall(r'ds_read', inner))} LDS reads")
    assert max(roots) >= 4                                                   # four beta-atoms per pass
    assert "global_load" not in inner and "flat_load" not in inner and "buffer_load" not in inner and "s_load" not in inner
    assert "ds_read" in inner and "s_barrier" not in inner and "ds_write" not in inner and "global_store" not in inner
    assert re.search(r"s_cbranch_\w+ \.LBB", inner)                           # it is a loop's body


def test_atomics(compiled):
    usage, asm = compiled
    assert "global_atomic" not in asm and "flat_atomic" not in asm and "buffer_atomic" not in asm
    assert not re.search(r"ds_\w*(add|sub|min|max)\w*_f(16|32|64)|ds_pk_add", asm)   # no float LDS atomic
    assert "cmpswap" not in asm and "cmpst" not in asm
    for name in usage:
        adds = _body(asm, name).count("ds_add_u32")
        assert (adds >= 1) == ("angle_hist_kernel" in name), (name, adds)
        assert "ds_add_rtn" not in _body(asm, name) and "ds_add_u64" not in _body(asm, name)
