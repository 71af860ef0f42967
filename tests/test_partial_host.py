"""Host proof for the partial spectra (tests/partial_cases.py, tests/partial64.py, psa_amd/partial.py): the float32 twin of
the two pair kernels stays inside every bar on every case, with plain and with fused multiply-adds; the exact items hold
for it bit for bit; every planted fault breaks an exact item or a bar; the sum rule of the definition holds in float64;
`combine`, `structure_factor`, the pair order and the species resolution of the calculator; the header and the library
carry the three entry points under ABI version 6.  Prints the worst fraction of each bar.  No GPU."""
import ctypes as Ct
import re
from pathlib import Path

import numpy as np
import pytest

import partial64 as R
import partial_cases as C
import power64
import power_cases as P

ROOT = Path(__file__).resolve().parents[1]
ENTRIES = ("psa_partial_spectra", "psa_debug_partial_project", "psa_debug_partial_power")


@pytest.fixture(scope="module")
def refs():
    return C.references()


@pytest.mark.parametrize("fused", [False, True], ids=["plain", "fused"])
@pytest.mark.parametrize("kind", ["vector", "shell"])
def test_twin_inside_every_bar(refs, kind, fused):
    worst = {}
    for name, (c, args, ref, bars) in refs[kind].items():
        got = C.run_model(c, args, fused=fused)
        assert got.shape == ref["out"].shape and not np.isnan(got).any(), name     # every element written
        for r, (f, at) in enumerate(C.worst(got, ref, bars)):
            assert f <= 1.0, (kind, name, C.ROWS[r], f, at)
            if C.ROWS[r] not in worst or f > worst[C.ROWS[r]][0]:
                worst[C.ROWS[r]] = (f, name, at)
        if got.shape[0] == 3:
            diag = [C.n_pairs(c["S"]) - C.n_pairs(c["S"] - a) for a in range(c["S"])]
            assert (got[2][diag] >= 0).all(), (kind, name)                  # transverse_aa: a sum of squares
        if c["relation"] == "i":
            assert not ref["out"][0][1].any() and ref["D"][1].any(), name   # the cross density is exactly 0, its bar is not
    for row, (f, name, at) in worst.items():
        print(f"{kind} {'fused' if fused else 'plain'} {row}: worst fraction of the bar {f:.3f} ({name} at {at})")


def _exact_items(fused=False, fault=None, kinds=("vector", "shell")):
    """(label, twin's result, the one right answer) of every exact item"""
    for L in C.EXACT_L:
        if "vector" in kinds:
            seg, k, norm = C.exact_vector(L)
            ref = R.vector64(seg, k, norm)["out"]
            assert np.array_equal(ref.astype(np.float32).astype(np.float64), ref)      # nothing to round
            for kb, sb in C.VECTOR_CUTS:
                yield f"vector L{L} cut {kb},{sb}", C.pair_model(seg, P.khat32(k), norm, None, 0, kb, sb, fused, fault), ref.astype(np.float32)
        if "shell" in kinds:
            seg, k, bin_of, n_bins, norm = C.exact_shell(L)
            ref = R.shell64(seg, k, bin_of, n_bins, norm)["out"].astype(np.float32)
            assert not ref[..., [0, 3, 5]].any() and ref[..., [1, 2, 4]].all()         # the empty bins: rows of zeros
            for kb, sb in C.SHELL_CUTS:
                yield f"shell L{L} cut {kb},{sb}", C.pair_model(seg, P.khat32(k), norm, bin_of, n_bins, kb, sb, fused, fault), ref


@pytest.mark.parametrize("fused", [False, True], ids=["plain", "fused"])
def test_exact_items_hold_for_the_twin(fused):
    n = 0
    for label, got, ref in _exact_items(fused):
        assert np.array_equal(C.bits(got), C.bits(ref)), label
        n += 1
    assert n == 2 * (3 + 3)


@pytest.mark.parametrize("fault", C.FAULTS)
def test_every_planted_fault_is_caught(refs, fault):
    kinds = ("shell",) if fault in C.SHELL_ONLY else ("vector", "shell")
    caught = []
    for kind in kinds:
        for label, got, ref in _exact_items(fault=fault, kinds=(kind,)):
            if not np.array_equal(C.bits(got), C.bits(ref)):
                caught.append(label)
        for name, (c, args, ref, bars) in refs[kind].items():
            if "tail" in name:
                continue                                                   # the small cases are enough
            got = C.run_model(c, args, fault=fault)
            if any(f > 1.0 for f, _ in C.worst(got, ref, bars)):
                caught.append(f"{kind} {name}")
        assert any(x.startswith(kind) for x in caught), (fault, kind)
    print(f"{fault}: caught by {len(caught)} items, first {caught[0]}")


def test_difference_form_breaks_the_bar_where_the_transverse_part_is_small(refs):
    c, args, ref, bars = refs["vector"]["S3_families"]
    fam = np.array([c["families"][i % len(c["families"])] for i in range(c["K"])])
    with np.errstate(divide="ignore", invalid="ignore"):
        f_old = np.abs(C.run_model(c, args, fault="diff_transverse")[2] - ref["out"][2]) / bars[2]
    for name in ("long", "1e-4"):
        assert f_old[..., fam == name].max() > 1.0, name
    assert C.fraction(C.run_model(c, args)[2], ref["out"][2], bars[2])[0] <= 1.0


def test_pair_order_and_rows():
    from psa_amd.partial import pair_row, pair_table
    for S in range(1, 9):
        pr = pair_table(S)
        assert np.array_equal(pr, R.pairs(S)) and pr.shape == (C.n_pairs(S), 2)
        for row, (a, b) in enumerate(pr):
            assert pair_row(a, b, S) == pair_row(b, a, S) == row
    assert R.pairs(3).tolist() == [[0, 0], [0, 1], [0, 2], [1, 1], [1, 2], [2, 2]]
    with pytest.raises(IndexError):
        pair_row(0, 3, 3)


@pytest.mark.parametrize("S", [1, 2, 3, 8])
def test_sum_rule_in_float64(S):
    """sum_a X_aa + 2 sum_{a<b} X_ab is the field X of the union, per vector and per shell; with coefficients, of the union
    weighted by them"""
    rng = np.random.default_rng(S)
    K, ns, L = 7, 3, 33
    k = P.family_vectors(rng, K, P.FAMILIES)
    seg = C.species_segments(rng, k, S, 4, ns, L, P.FAMILIES).astype(np.complex128)
    coef = rng.standard_normal(S)
    pr = R.pairs(S)
    bin_of = np.repeat(np.arange(3), [3, 0, 4])
    for c in (np.ones(S), coef):
        factor = c[pr[:, 0]] * c[pr[:, 1]] * np.where(pr[:, 0] == pr[:, 1], 1.0, 2.0)
        whole = np.sum(c[None, :, None, None, None] * seg, axis=1)
        for got, want in ((R.vector64(seg, k, 1.0), power64.dynamic64(whole, k, 1.0)),
                          (R.shell64(seg, k, bin_of, 3, 1.0), power64.shell64(whole, k, bin_of, 3, 1.0))):
            total = np.tensordot(factor, got["out"], axes=(0, 1))
            size = np.tensordot(np.abs(factor), np.abs(got["out"]), axes=(0, 1)).max()
            assert np.abs(total - want["out"]).max() <= 1e-13 * size


def _result(S=3, L=8, K=2, currents=True, dt=0.5):
    from psa_amd import PartialSpectra
    from psa_amd.partial import pair_table
    rng = np.random.default_rng(5)
    f = lambda: rng.standard_normal((C.n_pairs(S), L, K)).astype(np.float32)
    return PartialSpectra(f(), f() if currents else None, f() if currents else None, pair_table(S), [np.arange(i + 1) for i in range(S)],
                          np.array([2.0, 8.0, 0.0][:S]), np.fft.fftfreq(L, dt), np.zeros(K), np.zeros((K, 3)), dt)


def test_combine_and_structure_factor():
    r = _result()
    c = np.array([1.5, -2.0, 0.25])
    for field in ("density", "longitudinal", "transverse"):
        X = getattr(r, field).astype(np.float64)
        want = sum(c[a] * c[b] * X[r.pair(a, b)] for a in range(3) for b in range(3))   # every ordered pair
        np.testing.assert_allclose(r.combine(c, field), want, rtol=0, atol=1e-12)
    assert r.combine(c).dtype == np.float64 and r.combine(c).shape == (8, 2)
    sf = r.structure_factor
    assert sf.dtype == np.float64 and sf.shape == r.density.shape
    np.testing.assert_allclose(sf[r.pair(0, 1)], r.density[1].astype(np.float64) * 8 * 0.5 / 4.0)   # sqrt(2 x 8)
    np.testing.assert_allclose(sf[r.pair(1, 1)], r.density[3].astype(np.float64) * 8 * 0.5 / 8.0)
    assert not sf[r.pair(0, 2)].any() and not sf[r.pair(2, 2)].any()       # an empty species
    r.dt_ps = None
    np.testing.assert_allclose(r.structure_factor, sf)                     # the time step from the frequencies
    with pytest.raises(ValueError):
        r.combine(c[:2])
    with pytest.raises(ValueError):
        r.combine(c, "power")
    with pytest.raises(ValueError):
        _result(currents=False).combine(c, "transverse")


def _calculator(n=12, T=4):
    from psa_amd import SEDCalculator, Trajectory
    rng = np.random.default_rng(0)
    box = np.diag([4.0, 5.0, 6.0]).astype(np.float32)
    pos = rng.uniform(0, 4, (T, n, 3)).astype(np.float32)
    types = (1 + np.arange(n) % 3).astype(np.int32)
    tr = Trajectory(pos, np.zeros_like(pos), types, np.arange(T, dtype=np.float32), box, np.diag(box).copy(), np.zeros(3, np.float32), 0.002)
    return SEDCalculator(tr, 1, 1, 1)


def test_species_resolution_and_value_errors():
    calc = _calculator()
    w = np.arange(1, 13, dtype=np.float32)
    groups, norms = calc._partial_species(None, [1, 2], w)
    assert [g.tolist() for g in groups] == [[0, 3, 6, 9], [1, 4, 7, 10]]    # a flat type list: one species per type
    np.testing.assert_allclose(norms, [np.sum(w[g].astype(np.float64) ** 2) for g in groups])
    assert len(calc._partial_species(None, [[1, 2], [3]], None)[0]) == 2
    groups, norms = calc._partial_species(None, None, None)
    assert len(groups) == 1 and groups[0].tolist() == list(range(12)) and norms.tolist() == [12.0]
    assert [g.tolist() for g in calc._partial_species([[5, 2], [7]], None, None)[0]] == [[5, 2], [7]]     # the order given
    with pytest.raises(ValueError, match="disjoint"):
        calc._partial_species([[0, 1], [1, 2]], None, None)
    with pytest.raises(ValueError, match="at most 8"):
        calc._partial_species([[i] for i in range(9)], None, None)
    ind = np.array([[1, 0, 0]])
    for method, first in ((calc.calculate_partial_spectra, ind), (calc.calculate_powder_partial_spectra, [0.5, 2.0])):
        with pytest.raises(ValueError, match="disjoint"):
            method(first, [[0, 1], [1, 2]])
        with pytest.raises(ValueError, match="at most 8"):
            method(first, [[i] for i in range(9)])
        with pytest.raises(TypeError):
            method(first, segments=(64, 32))
        with pytest.raises(ValueError):
            method(first, atom_weights=np.ones(5))
    with pytest.raises(ValueError):
        calc.calculate_partial_spectra(np.array([[65, 0, 0]]))
    with pytest.raises(ValueError):
        calc.calculate_powder_partial_spectra([2.0, 1.0])
    empty = calc.calculate_partial_spectra(np.zeros((0, 3), int), currents=False)      # nothing to do: no engine is asked
    assert empty.density.shape == (1, 4, 0) and empty.longitudinal is None and empty.pairs.tolist() == [[0, 0]]


def test_engine_species_arguments():
    from psa_amd import _hip
    idx, off, S = _hip.Engine._species_args([[3, 1], [], [2]])
    assert idx.dtype == np.int32 and idx.tolist() == [3, 1, 2] and off.dtype == np.int64 and off.tolist() == [0, 2, 2, 3] and S == 3
    assert _hip.Engine._species_args([[], []])[0].size == 1                # a pointer to something
    for bad in ([], [[i] for i in range(9)]):
        with pytest.raises(ValueError, match="species"):
            _hip.Engine._species_args(bad)
    assert _hip.PARTIAL_MAX_SPECIES == 8


def test_header_declares_and_library_exports_the_entry_points():
    from psa_amd import _hip
    header = (ROOT / "include" / "psa_hip.h").read_text()
    assert re.search(r"#define PSA_HIP_ABI_VERSION 6\b", header)
    for name in ENTRIES:
        assert re.search(rf"\bint {name}\(psa_ctx\* ctx,", header), name
        assert name in _hip.SIGNATURES, name
    assert "PARTIAL_MAX_SPECIES = 8" in (ROOT / "psa_amd" / "csrc" / "psa_ctx.h").read_text()
    lib = _hip.load_library()
    assert lib.psa_abi_version() == _hip.ABI_VERSION == 6
    for name in ENTRIES:
        assert isinstance(getattr(lib, name), Ct._CFuncPtr), name
