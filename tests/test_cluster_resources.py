"""The four cluster kernels (psa_amd/csrc/cluster.hip) as the compiler builds them for gfx950 (hipcc cross-compiles here), from
the compiler's resource remarks and the assembly: exactly four kernels, no scratch, no spilled vector register, within 128
vector registers; no float atomic of any kind (global, flat, buffer or LDS); the global atomics that are there are the
integer compare-and-swap on `parent` and the integer add on `size`; the Makefile lists the source."""
import re

import pytest

from kernel_build import SRC, device_compile

KERNELS = ("cluster_bonds_kernel", "cluster_hook_kernel", "cluster_flatten_kernel", "cluster_stats_kernel")


def test_makefile_lists_the_source():
    mk = (SRC / "Makefile").read_text()
    srcs = next(ln for ln in mk.splitlines() if ln.startswith("SRCS"))
    assert " cluster.hip" in srcs and re.search(r"for f in [^;]*\bcluster\b[^;]*; do", mk)
    assert all((SRC / f).is_file() for f in srcs.split(":=")[1].split())
    assert (SRC / "cluster.hip").read_text().count("__global__") == 4


@pytest.fixture(scope="module")
def compiled():
    c = device_compile("cluster.hip")
    print(c.usage)
    return c.usage, c.asm


def test_kernel_resources(compiled):
    usage, asm = compiled
    assert len(usage) == 4 and all(sum(k in name for name in usage) == 1 for k in KERNELS)
    for name, u in usage.items():
        assert u["ScratchSize [bytes/lane]"] == 0 and u["VGPRs Spill"] == 0 and u["SGPRs Spill"] == 0, (name, u)
        assert u["VGPRs"] + u["AGPRs"] <= 128, (name, u)
    assert "scratch_" not in asm


def test_atomics(compiled):
    usage, asm = compiled
    # no float atomic: global, flat, buffer or LDS
    assert not re.search(r"(global|flat|buffer)_atomic_\w*(f16|f32|f64|bf16)", asm)
    assert not re.search(r"ds_\w*(add|sub|min|max)\w*_f(16|32|64)|ds_pk_add", asm)
    assert "flat_atomic" not in asm and "buffer_atomic" not in asm
    # the global atomics: the compare-and-swap of the hook pass, the add of the flatten pass, 32-bit integers
    kinds = set(re.findall(r"\b(global_atomic_\w+)", asm))
    assert kinds == {"global_atomic_cmpswap", "global_atomic_add"}, kinds
    assert asm.count("ds_add_u32") >= 3 and "ds_max_u64" in asm
