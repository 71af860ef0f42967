"""The pair passes of the partial spectra (psa_amd/csrc/partial.hip) as the compiler builds them for gfx950 (hipcc
cross-compiles here), from the compiler's resource remarks only: the power pass and the shell pass, each with and without
currents -- no scratch, no spilled registers, at most 128 VGPRs, no LDS --, and the Makefile's lists."""
import re

import pytest

from kernel_build import SRC, device_compile


def test_makefile_lists_the_sources():
    mk = (SRC / "Makefile").read_text()
    srcs = next(ln for ln in mk.splitlines() if ln.startswith("SRCS"))
    assert " partial.hip" in srcs and " api_partial.hip" in srcs
    assert re.search(r"for f in [^;]*\bpartial\b[^;]*; do", mk)               # the asm list
    assert all((SRC / f).is_file() for f in srcs.split(":=")[1].split())


@pytest.fixture(scope="module")
def usage():
    c = device_compile("partial.hip")
    print(c.usage)
    return c.usage


def test_partial_kernels_resources(usage):
    assert len(usage) == 4
    for kernel in ("partial_power_kernel", "partial_shell_kernel"):
        for nc in (1, 4):
            name, u = next((k, v) for k, v in usage.items() if f"{kernel}ILi{nc}EE" in k)
            assert u["ScratchSize [bytes/lane]"] == 0 and u["VGPRs Spill"] == 0 and u["SGPRs Spill"] == 0, (name, u)
            assert u["VGPRs"] + u["AGPRs"] <= 128 and u["LDS Size [bytes/block]"] == 0, (name, u)
