"""The table of the context's device buffers (psa_debug_scratch_info, api_core.hip) against the DevBuf members of psa_ctx,
the least classification the scratch-history tests rely on, the two entries in the header, and the comparison helper of
tests/scratch_cases.py shown to fail when it should.  No GPU."""
import re

import numpy as np
import pytest

import scratch_cases as S
from conftest import ROOT

CTX_H = ROOT / "psa_amd" / "csrc" / "psa_ctx.h"
HEADER = ROOT / "include" / "psa_hip.h"


def _ctx_members():
    """every psa::DevBuf member of struct psa_ctx, in the order of the header"""
    text = CTX_H.read_text()
    body = text[text.index("struct psa_ctx {"):]
    body = body[:body.index("\n};")]
    body = re.sub(r"//[^\n]*", "", body)
    names = []
    for decl in re.findall(r"psa::DevBuf\s+([^;]+);", body):
        names += [n.strip() for n in decl.split(",")]
    assert all(re.fullmatch(r"d_\w+", n) for n in names), names
    return names


@pytest.fixture(scope="module")
def table():
    from psa_amd import _hip
    return _hip.scratch_table()


def test_every_member_is_in_the_table_exactly_once(table):
    members = _ctx_members()
    assert len(members) >= 75 and len(set(members)) == len(members), len(members)
    names = [n for n, _ in table]
    assert sorted(names) == sorted(members), (set(members) - set(names), set(names) - set(members))
    assert len(set(names)) == len(names)
    assert all(c in ("real", "index", "state") for _, c in table)


def test_the_table_ends(table):
    from psa_amd import _hip
    lib = _hip.load_library()
    assert lib.psa_debug_scratch_info(len(table), None, None) != 0
    assert lib.psa_debug_scratch_info(-1, None, None) != 0
    assert lib.psa_debug_scratch_info(0, None, None) == 0            # either output may be null


INDEX = ("d_idx d_rc_idx d_rc_tiles d_rc_ent d_rc_slot d_rc_dest d_rc_bins d_rc_groups d_rs_idx d_rs_items d_vdos_pairs "
         "d_vdos_off d_kmap d_cols d_peaks_bands d_angle_work").split()
NOT_STATE = ("d_qwork d_fft_work d_phase d_mean_g d_kvec d_seg d_qrows d_stage d_vdos_work d_vdos_part d_vdos_acc d_modes_work "
             "d_cov_slab d_peaks_part d_pair_c d_msd_u d_msd_sums d_msd_offs d_lr_diff d_lr_qn d_lr_L d_lr_phi d_lr_f64").split()
REAL = "d_slab d_out d_aux d_inten".split()
STATE = "d_weights d_seg_window d_zeros".split()


def test_minimum_classification(table):
    cls = dict(table)
    rc = [n for n in cls if n.startswith("d_rc_")]
    rs = [n for n in cls if n.startswith("d_rs_")]
    assert len(rc) == 14 and len(rs) == 4, (rc, rs)
    for n in rc + rs + NOT_STATE:
        assert cls[n] in ("real", "index"), (n, cls[n])
    for n in INDEX:
        assert cls[n] == "index", (n, cls[n])
    for n in REAL:
        assert cls[n] == "real", (n, cls[n])
    for n in STATE:
        assert cls[n] == "state", (n, cls[n])
    # no expected buffer was moved to "state": DESIGN.md would have to say why
    assert sorted(n for n, c in cls.items() if c == "state") == sorted(STATE)


def test_the_header_declares_both_entries_and_abi_6():
    from psa_amd import _hip
    text = HEADER.read_text()
    assert re.search(r"#define PSA_HIP_ABI_VERSION 6\b", text)
    assert _hip.ABI_VERSION == 6 and _hip.load_library().psa_abi_version() == 6
    assert re.search(r"int\s+psa_debug_scratch_info\(int index, const char\*\* name, int32_t\* cls\);", text)
    assert re.search(r"int\s+psa_debug_scratch_fill\(psa_ctx\* ctx, int byte, int64_t\* buffers, int64_t\* bytes\);", text)
    for i, name in enumerate(("REAL", "INDEX", "STATE")):
        assert re.search(rf"#define PSA_SCRATCH_{name} {i}\b", text)
        assert _hip.SCRATCH_CLASSES[i] == name.lower()
    for entry in ("psa_debug_scratch_info", "psa_debug_scratch_fill"):
        assert entry in _hip.SIGNATURES


# ---- the comparison helper fails when it should ------------------------------------------------------------------------------
class StubEngine:
    """A test double in the manner of tests/oracle_engine.py: its one "kernel" reads a padded table of 8 x 12 values of
    which the call writes 8 x 10; `leak` = (row, column): that output element also takes in the padded cell behind its
    row, which holds whatever the last fill left there."""

    def __init__(self, leak=None, fills=True):
        self.table = np.zeros((8, 12), np.float32)
        self.leak, self.fills, self.filled = leak, fills, []

    def scratch_fill(self, byte):
        self.filled.append(byte)
        if not self.fills:
            return 0, 0
        if byte >= 0:
            self.table.view(np.uint8)[:] = byte
        return 1, self.table.nbytes

    def run(self):
        self.table[:, :10] = np.arange(80, dtype=np.float32).reshape(8, 10) + 0.5
        out = 2.0 * self.table[:, :10]
        if self.leak is not None:
            r, c = self.leak
            out[r, c] += self.table[r, 11]
        return out, np.arange(8, dtype=np.int64)


def _call(engine):
    return S.as_arrays(engine.run())


def test_helper_passes_a_kernel_that_reads_what_it_wrote():
    eng = StubEngine()
    r0 = _call(eng)
    assert S.check_poisoned(eng, "stub", _call, r0) == (1, 8 * 12 * 4)
    assert eng.filled == [0x00, 0xFF]


def test_helper_reports_the_element_that_read_the_padding(capsys):
    eng = StubEngine(leak=(5, 9))
    r0 = _call(eng)                                        # the padding holds zeros: the first result is the right one
    S.compare("stub", "repeated", r0, _call(eng))          # ... and so is a repeat, and a fill with zeros
    with pytest.raises(S.Differs) as e:
        S.check_poisoned(eng, "stub", _call, r0)
    assert eng.filled == [0x00, 0xFF]                      # the zero pattern passed, the NaN pattern did not
    assert (e.value.array, e.value.element) == (0, (5, 9))
    assert np.isnan(e.value.got) and e.value.want == np.float32(2 * 59.5)
    assert "array 0 element (5, 9)" in str(e.value) and "1 of 80 elements differ" in str(e.value)
    assert "array 0 element (5, 9)" in capsys.readouterr().out


def test_helper_reports_a_finite_difference_and_a_later_array():
    a = [np.zeros((3, 4), np.complex64), np.arange(6, dtype=np.uint64).reshape(2, 3)]
    b = [a[0].copy(), a[1].copy()]
    assert S.first_difference(a, b) is None
    b[1][1, 2] += 1
    assert S.first_difference(a, b)[:2] == (1, (1, 2))
    b[0][2, 0] = np.complex64(-0.0)                        # bits, not values: -0.0 is not 0.0
    assert S.first_difference(a, b)[:2] == (0, (2, 0))


def test_helper_refuses_a_hook_that_fills_nothing():
    eng = StubEngine(fills=False)
    with pytest.raises(AssertionError, match="the hook did nothing"):
        S.check_poisoned(eng, "stub", _call, _call(eng))


def test_case_table_is_whole():
    """every entry family has a case that stands for it, every case a family that some fresh context runs"""
    families = {f for f, _ in S.CASES.values()}
    assert families == set(S.HISTORY) and all(S.CASES[n][0] == f for f, n in S.HISTORY.items())
    assert sorted(f for row in S.FRESH.values() for f in row) == sorted(families)
    for members in S.SHARING.values():
        assert set(members) <= families
    assert S.others_sharing("pair") == ["msd", "angle", "order"]
    assert "dynamic" in S.others_sharing("sed") and "sed" in S.others_sharing("lattice")
