"""The two local-order kernels (psa_amd/csrc/qlm.hip) as the compiler builds them for gfx950 (hipcc cross-compiles here), from
the compiler's resource remarks and the assembly: exactly two kernels, no scratch, no spilled vector register, within 128
vector registers -- the scalar registers that the second kernel's compiler parks in lanes of vector registers (v_writelane,
never memory) are inside that count, and "no scratch" is what keeps them out of memory; the first kernel parks none --; no
global, flat or buffer atomic, no float LDS atomic, no 64-bit LDS atomic, and the 32-bit integer LDS add that
counts; the Makefile lists the source."""
import re

import pytest

from kernel_build import SRC, device_compile


def test_makefile_lists_the_source():
    mk = (SRC / "Makefile").read_text()
    srcs = next(ln for ln in mk.splitlines() if ln.startswith("SRCS"))
    assert " qlm.hip" in srcs and re.search(r"for f in [^;]*\bqlm\b[^;]*; do", mk)
    assert all((SRC / f).is_file() for f in srcs.split(":=")[1].split())
    assert (SRC / "qlm.hip").read_text().count("__global__") == 2


@pytest.fixture(scope="module")
def compiled():
    c = device_compile("qlm.hip")
    print(c.usage)
    return c.usage, c.asm


def test_kernel_resources(compiled):
    usage, asm = compiled
    assert len(usage) == 2 and sorted(("qlm_sum_kernel" in k) + 2 * ("local_order_kernel" in k) for k in usage) == [1, 2]
    for name, u in usage.items():
        assert u["ScratchSize [bytes/lane]"] == 0 and u["VGPRs Spill"] == 0, u
        assert u["VGPRs"] + u["AGPRs"] <= 128, u
        assert u["SGPRs Spill"] == 0 or "local_order_kernel" in name, u
    assert "scratch_" not in asm


def test_atomics(compiled):
    usage, asm = compiled
    assert "global_atomic" not in asm and "flat_atomic" not in asm and "buffer_atomic" not in asm
    assert not re.search(r"ds_\w*(add|sub|min|max)\w*_f(16|32|64)|ds_pk_add", asm)   # no float LDS atomic
    assert "cmpswap" not in asm and "cmpst" not in asm
    assert asm.count("ds_add_u32") >= 1 and "ds_add_rtn" not in asm and "ds_add_u64" not in asm
    assert not re.search(r"ds_(add|sub|inc|dec|min|max|and|or|xor)\w*_(u|i|b)64", asm)   # no 64-bit LDS atomic of any kind
