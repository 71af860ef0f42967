"""The self (incoherent) spectra without a GPU: the float64 restatement (tests/self64.py) against what is known exactly --
the sum rule, frozen atoms, ballistic lines, wrapped against unwrapped coordinates --, that it is not the coherent
spectrum, the float32 model of the series kernel inside the series bound (and outside it with the fractional coordinate
rounded to one float32), the tile rule, and the Python layer's refusals, raised before any device is reached."""
import numpy as np
import pytest

import lattice64
import self64
import self_cases as S
from conftest import rel_max
from psa_amd import DynamicSpectra, PowderSpectra, SEDCalculator, Segments, Trajectory, _hip, draw_atoms

N0 = np.array([2, -1, 3])


def _vectors():
    return np.concatenate([S.C.mixed_indices(4, seed=4), N0[None], -N0[None]]).astype(np.int32)


@pytest.mark.parametrize("box", [S.CUBIC, S.TRICLINIC], ids=["cubic", "triclinic"])
def test_sum_rule_of_the_reference(box):
    """sum_o density[o,n] = sum_a w_a^2 for every vector, one boxcar segment: Parseval"""
    pos = S.random_walk(9, 50, seed=1, box=box)[0]
    w = S.weights("signed", 9, seed=2)
    den = self64.density64(pos, _vectors(), S.inverse(box), None, w)
    total = float(np.sum(w.astype(np.float64) ** 2))
    assert np.max(np.abs(den.sum(0) - total)) <= 1e-12 * total


def test_frozen_atoms_sit_in_bin_zero():
    pos = S.frozen(7, 40, seed=3, box=S.TRICLINIC)
    w = S.weights("sqrt_mass", 7, seed=4)
    total = float(np.sum(w.astype(np.float64) ** 2))
    den = self64.density64(pos, _vectors(), S.inverse(S.TRICLINIC), None, w)
    assert np.max(np.abs(den[0] - total)) <= 1e-12 * total
    assert np.max(np.abs(den[1:])) <= 1e-20 * total


def test_ballistic_atoms_are_lines():
    """column n0 of family (b) has w_a^2 in bin b_a; what the float32 positions leak is (2 pi |n0| 3 sqrt(3) 2^-24)^2"""
    T, n = 60, 12
    pos, b = S.ballistic(n, T, seed=5, n0=N0, box=S.CUBIC)
    w = S.weights("signed", n, seed=6)
    den = self64.density64(pos, N0[None], S.inverse(S.CUBIC), None, w)[:, 0]
    want = np.zeros(T)
    want[b % T] = w.astype(np.float64) ** 2
    leak = (2 * np.pi * np.linalg.norm(N0) * 3 * np.sqrt(3.0) * 2.0 ** -24) ** 2
    assert np.max(np.abs(den - want)) <= 2 * np.sqrt(leak) * want.max()
    assert rel_max(den, want) <= 1e-5


def test_wrapped_and_unwrapped_agree():
    _, _, wrapped, unwrapped = S.random_walk(8, 48, seed=7, box=S.TRICLINIC)
    inv = S.inverse(S.TRICLINIC)
    s = Segments(16, 8, "hann")
    for win in ((None, None, None), (s.window_array(), 16, 8)):
        a = self64.density64(wrapped, _vectors(), inv, None, None, *win)
        b = self64.density64(unwrapped, _vectors(), inv, None, None, *win)
        assert rel_max(a, b) <= 1e-9


def test_it_is_not_the_coherent_spectrum():
    pos = S.random_walk(20, 64, seed=8)[0]
    inv = S.inverse(S.CUBIC)
    ind = _vectors()[[0, 2, 4]]
    w = S.weights("sqrt_mass", 20, seed=9)
    own = self64.density64(pos, ind, inv, None, w)
    coherent = lattice64.spectra64(lattice64.project64(pos, None, ind, inv, None, w, False), ind, inv)[0]
    assert np.max(np.abs(own - coherent)) > 0.1 * own.max()


def test_series_model_inside_the_bound_and_single_precision_outside():
    """family (d), |k.r| ~ 1e4 rad: the kernel's arithmetic in NumPy float32 (sine and cosine exact) stays inside the series
    bound; with s rounded to one float32 it does not -- the bound can fail"""
    box, n, T = S.TRICLINIC, 5, 12
    inv = S.inverse(box)
    pos = S.far(n, T, seed=10, box=box)
    ind = S.C.corner_indices()
    w = S.weights("signed", n, seed=11)
    idx = np.array([3, 0, 4])
    assert S.C.max_abs_phase(pos, ind, inv, idx) >= 1e4
    ref = self64.series64(pos, ind, inv, idx, w)
    lim = S.bound(w[idx])[:, None, None]
    good = np.abs(S.series_model(pos, ind, inv, idx, w).astype(np.complex128) - ref) / lim
    bad = np.abs(S.series_model(pos, ind, inv, idx, w, single=True).astype(np.complex128) - ref) / lim
    print(f"two-float32 s: {good.max():.3f} of the bound; one float32: {bad.max():.3f}")
    assert good.max() <= 1.0
    assert bad.max() > 1.0


def test_tile_rule():
    assert S.tiles(S.grid_indices(63)) == [63] and S.tiles(S.grid_indices(64)) == [64] and S.tiles(S.grid_indices(65)) == [64, 1]
    assert S.tiles(S.C.corner_indices()) == [8]
    line = np.stack([np.arange(-30, 31), np.zeros(61, int), np.zeros(61, int)], 1)      # a new entry per vector
    assert S.tiles(line) == [_hip.SELF_ENTRIES - 2] * 2 + [61 - 2 * (_hip.SELF_ENTRIES - 2)]
    assert _hip.SELF_ATOMS * _hip.SELF_FRAMES == _hip.SELF_THREADS


def test_draw_atoms():
    atoms = np.arange(100, 230)
    assert draw_atoms(atoms, None) is not None and np.array_equal(draw_atoms(atoms, None), atoms)
    assert np.array_equal(draw_atoms(atoms, 130), atoms) and np.array_equal(draw_atoms(atoms, 500), atoms)
    a, b, c = draw_atoms(atoms, 40, 0), draw_atoms(atoms, 40, 0), draw_atoms(atoms, 40, 1)
    assert a.size == 40 and np.unique(a).size == 40 and np.all(np.isin(a, atoms)) and np.array_equal(a, b)
    assert not np.array_equal(a, c)
    for bad in (0, -3, 2.5, "7", True):
        with pytest.raises(ValueError, match="max_atoms"):
            draw_atoms(atoms, bad)


# ---- the Python layer ---------------------------------------------------------------------------------------------------
def _calculator(n_atoms=8, n_frames=16, box=S.CUBIC):
    pos, vel = S.C.trajectory(n_atoms, n_frames, seed=1, box=box)
    box = np.asarray(box, np.float32)
    tr = Trajectory(pos, vel, np.ones(n_atoms, np.int32), np.arange(n_frames, dtype=np.float32), box, np.diag(box).copy(),
                    np.zeros(3, np.float32), 0.002)
    return SEDCalculator(tr, 4, 4, 4)


@pytest.mark.parametrize("method", ["vector", "powder"])
def test_argument_checks_need_no_device(method):
    calc = _calculator()
    g1 = 2 * np.pi / 21.72
    if method == "vector":
        first = np.array([[1, 0, 0], [0, -2, 1]])
        call = calc.calculate_self_spectra
        with pytest.raises(ValueError, match="integers"):
            call(np.array([[0.5, 0.0, 1.0]]))
        with pytest.raises(ValueError, match="are served"):
            call(np.array([[0, _hip.LAT_MAX_INDEX + 1, 0]]))
        with pytest.raises(ValueError, match=r"\(K, 3\)"):
            call(np.arange(4))
    else:
        first = [0.9 * g1, 1.1 * g1]
        call = calc.calculate_powder_self_spectra
        with pytest.raises(ValueError, match="q_edges"):
            call([0.5, 0.4])
        with pytest.raises(ValueError, match="are served"):
            call([0.1, (_hip.LAT_MAX_INDEX + 1.5) * g1])
        with pytest.raises(ValueError, match="max_per_bin"):
            call(first, max_per_bin=0)
    for bad in (0, -1, 1.5):
        with pytest.raises(ValueError, match="max_atoms"):
            call(first, max_atoms=bad)
    with pytest.raises(TypeError, match="Segments"):
        call(first, segments=(8, 4, "hann"))
    with pytest.raises(ValueError):
        call(first, segments=Segments(32, 16, "hann"))                     # L > T
    with pytest.raises(ValueError):
        call(first, atom_weights=np.ones(7, np.float32))

    class TwoRanks:
        nranks, mode, engine = 2, "k", None
    calc._shard = TwoRanks()
    with pytest.raises(NotImplementedError, match="sharded"):
        call(first)
    calc._shard = None
    assert calc._engine is None                                            # nothing above reached for a device


def test_empty_inputs_and_the_result_types():
    calc = _calculator()
    out = calc.calculate_self_spectra(np.zeros((0, 3), np.int32), segments=Segments(8, 4, "hann"))
    assert isinstance(out, DynamicSpectra) and out.density.shape == (8, 0) and out.longitudinal is None and out.transverse is None
    g1 = 2 * np.pi / 21.72
    pw = calc.calculate_powder_self_spectra([0.2 * g1, 0.6 * g1, 0.9 * g1])     # no vector below the first shell |G_1|
    assert isinstance(pw, PowderSpectra) and pw.density.shape == (16, 2) and pw.longitudinal is None and pw.transverse is None
    assert np.all(pw.density == 0) and np.all(pw.counts == 0) and np.all(np.isnan(pw.q)) and pw.weight_norm == 0.0
    assert calc._engine is None
    import psa_amd
    assert "draw_atoms" in psa_amd.__all__ and hasattr(SEDCalculator, "calculate_powder_self_spectra")
    assert {"psa_self_spectra", "psa_debug_self_series"} <= set(_hip.SIGNATURES)
