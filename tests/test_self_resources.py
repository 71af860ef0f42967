"""The self-spectra kernels (psa_amd/csrc/self.hip) as the compiler builds them for gfx950 (hipcc cross-compiles here), from
the compiler's resource remarks and the assembly: no scratch and no spilled registers anywhere; the series kernel within
128 VGPRs and with an LDS footprint -- the table tab[atom][entry][frame] -- that lets at least two workgroups share a
compute unit; the blocks that store the series read the table and hold no sine and no cosine; the transcendentals sit in
the build step, one sine and one cosine per entry written; no atomics; the lattice kernels still compile from the shared
header."""
import re

import pytest

from kernel_build import SRC, device_compile
from psa_amd import _hip

LDS_PER_CU = 160 * 1024


def test_makefile_lists_the_sources():
    mk = (SRC / "Makefile").read_text()
    srcs = next(ln for ln in mk.splitlines() if ln.startswith("SRCS"))
    assert " self.hip" in srcs and " api_self.hip" in srcs
    assert re.search(r"for f in [^;]*\bself\b[^;]*; do", mk)                  # the asm list
    assert all((SRC / f).is_file() for f in srcs.split(":=")[1].split())
    assert "lattice_math.h" in mk and (SRC / "lattice_math.h").is_file()      # the shared header is a prerequisite
    for f in ("lattice.hip", "self.hip"):
        text = (SRC / f).read_text()
        assert '#include "lattice_math.h"' in text and "lat_entry(const float" not in text


@pytest.fixture(scope="module")
def compiled():
    c = device_compile("self.hip")
    print(c.usage)
    return c.usage, c.asm


def test_self_kernels_resources(compiled):
    usage, asm = compiled
    assert len(usage) == 4                                                    # series, power with and without mirror, reduce
    for name, u in usage.items():
        assert u["ScratchSize [bytes/lane]"] == 0 and u["VGPRs Spill"] == 0 and u["SGPRs Spill"] == 0, (name, u)
    assert "scratch_" not in asm
    assert "atomic" not in asm and "ds_add" not in asm                        # no atomics anywhere
    name, u = next((k, v) for k, v in usage.items() if "self_series_kernel" in k)
    lds = _hip.SELF_ATOMS * _hip.SELF_ENTRIES * _hip.SELF_FRAMES * 8
    assert u["VGPRs"] + u["AGPRs"] <= 128, (name, u)
    assert u["LDS Size [bytes/block]"] == lds and 2 * lds <= LDS_PER_CU, (name, u)
    body = asm[asm.index(name + ":"):]
    body = body[:body.index("s_endpgm")]
    blocks = re.split(r"\n\.LBB\d+_\d+:", body)
    # the blocks that store the series: table reads (8-byte LDS reads), the products, the stores; nothing transcendental
    store = [b for b in blocks if "global_store_dwordx2" in b]
    assert store
    for b in store:
        n = b.count("global_store_dwordx2")
        print(f"a storing block: {n} stores, {b.count('ds_read_b64') + 2 * b.count('ds_read2_b64')} table reads, "
              f"{b.count('v_fma_f32') + b.count('v_fmac_f32') + b.count('v_pk_fma_f32')} FMAs")
        assert "v_sin_f32" not in b and "v_cos_f32" not in b, name
        assert b.count("ds_read_b64") + 2 * b.count("ds_read2_b64") == 3 * n, name
        assert "ds_write" not in b and "s_barrier" not in b, name
    assert "v_sin_f32" not in "".join(store)
    # the build step: one sine and one cosine per entry written (the compiler may unroll it: every copy is held)
    build = [b for b in blocks if "v_sin_f32" in b or "v_cos_f32" in b]
    assert build
    for b in build:
        words = b.count("ds_write_b64") + 2 * b.count("ds_write2_b64") + 2 * b.count("ds_write2st64_b64")
        assert b.count("v_sin_f32") == b.count("v_cos_f32") == words >= 1, name
    assert "s_barrier" not in body                                            # a lane reads only what it wrote
    for key in ("self_power_kernel", "self_reduce_kernel"):
        for name, u in ((k, v) for k, v in usage.items() if key in k):
            assert u["LDS Size [bytes/block]"] == 0 and u["VGPRs"] + u["AGPRs"] <= 128, (name, u)
