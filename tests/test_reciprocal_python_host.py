"""The Python layer above the reciprocal core -- the ten `SEDCalculator` methods on the box's lattice and the five
`Engine` entries below them -- held to its plumbing on the CPU: a recording stand-in takes the engine's place, and every
call it receives, every field of the result, the order of the refusals and the empty inputs are compared with
expectations written out from the documented definitions.  Inputs: T = 16 frames, N = 8 atoms of two types (3 + 5; 2 + 3
under the index subset), K = 3 vectors, two shells of 3 and 6 half-space vectors in a cubic box of side 10."""
import inspect
import itertools
import threading

import numpy as np
import pytest

from psa_amd import (DynamicSpectra, PartialSpectra, PowderPartialSpectra, PowderSpectra, PowderTimeCorrelations, SEDCalculator,
                     Segments, TimeCorrelations, Trajectory, _hip)

T, N, DT, SIDE = 16, 8, 0.002, 10.0
TYPES = np.array([1, 1, 1, 2, 2, 2, 2, 2], np.int32)
SUBSET = [0, 1, 3, 4, 5]                                   # two atoms of type 1, three of type 2
INDICES = np.array([[1, 0, 0], [0, 2, 1], [-1, 1, 3]])
G1 = 2 * np.pi / SIDE
EDGES = np.array([0.8 * G1, 1.2 * G1, 1.6 * G1])           # |n| = 1: 3 half-space vectors; |n| = sqrt 2: 6
# the half space of the two shells, sorted by |k|, then by index
SHELL_N = np.array([[0, 0, 1], [0, 1, 0], [1, 0, 0], [0, 1, -1], [0, 1, 1], [1, -1, 0], [1, 0, -1], [1, 0, 1], [1, 1, 0]], np.int32)
SHELL_B = np.array([0, 0, 0, 1, 1, 1, 1, 1, 1], np.int32)
SEG = Segments(8, 4, "boxcar")                             # L = 8 != T, n_seg = 3
WEIGHTS = np.linspace(0.5, 2.25, N)

# name -> (kind, family, powder)
METHODS = {f"calculate_{'powder_' if p else ''}{'lattice_' if f == 'coherent' and not p else ''}"
           f"{'' if f == 'coherent' else f + '_'}{k}": (k, f, p)
           for k, f, p in itertools.product(("spectra", "correlations"), ("coherent", "self", "partial"), (False, True))
           if (k, f) != ("correlations", "partial")}
ENTRY = {("spectra", "coherent"): "lattice_spectra", ("spectra", "self"): "self_spectra", ("spectra", "partial"): "partial_spectra",
         ("correlations", "coherent"): "lattice_correlations", ("correlations", "self"): "self_correlations"}
RESULT = {("spectra", "coherent"): (DynamicSpectra, PowderSpectra), ("spectra", "self"): (DynamicSpectra, PowderSpectra),
          ("spectra", "partial"): (PartialSpectra, PowderPartialSpectra),
          ("correlations", "coherent"): (TimeCorrelations, PowderTimeCorrelations),
          ("correlations", "self"): (TimeCorrelations, PowderTimeCorrelations)}


def frozen(a):
    """what a logged argument is compared by: dtype, shape and bytes of an array, type and value of anything else"""
    if isinstance(a, np.ndarray):
        return ("array", a.dtype.str, a.shape, a.tobytes())
    if isinstance(a, (list, tuple)):
        return (type(a).__name__,) + tuple(frozen(v) for v in a)
    return (type(a).__name__, a)


class Recorder:
    """The engine's stand-in: logs every call, returns arrays of the documented shapes whose elements are all distinct."""

    def __init__(self, fail=None):
        self.lock, self.log, self.returned, self.fail, self.length = threading.RLock(), [], None, fail, None

    def _note(self, name, *args):
        self.log.append((name,) + tuple(frozen(a) for a in args))
        if name == self.fail:
            raise RuntimeError("planted")

    def _give(self, *shape):
        self.returned = np.arange(int(np.prod(shape)), dtype=np.float32).reshape(shape)
        return self.returned

    def set_atom_weights(self, weights):
        self._note("set_atom_weights", weights)

    def set_segments(self, segments):
        self._note("set_segments", segments)
        self.length = None if segments is None else segments.length

    def ensure_resident(self, slot, array):
        self._note("ensure_resident", slot, array)

    @staticmethod
    def _cols(indices, bin_of, n_bins):
        return len(indices) if bin_of is None else n_bins

    def dynamic_spectra(self, k_vectors, idx=None, currents=True):
        self._note("dynamic_spectra", k_vectors, idx, currents)
        return self._give(3 if currents else 1, self.length or T, len(k_vectors))

    def lattice_spectra(self, box_inverse, indices, bin_of=None, n_bins=0, idx=None, currents=True):
        self._note("lattice_spectra", box_inverse, indices, bin_of, n_bins, idx, currents)
        return self._give(3 if currents else 1, self.length or T, self._cols(indices, bin_of, n_bins))

    def self_spectra(self, box_inverse, indices, bin_of=None, n_bins=0, idx=None):
        self._note("self_spectra", box_inverse, indices, bin_of, n_bins, idx)
        return self._give(self.length or T, self._cols(indices, bin_of, n_bins))

    def partial_spectra(self, box_inverse, indices, species, bin_of=None, n_bins=0, currents=True):
        self._note("partial_spectra", box_inverse, indices, species, bin_of, n_bins, currents)
        S = len(species)
        return self._give(3 if currents else 1, S * (S + 1) // 2, self.length or T, self._cols(indices, bin_of, n_bins))

    def lattice_correlations(self, box_inverse, indices, n_lags, bin_of=None, n_bins=0, idx=None, currents=True):
        self._note("lattice_correlations", box_inverse, indices, n_lags, bin_of, n_bins, idx, currents)
        return self._give(3 if currents else 1, n_lags, self._cols(indices, bin_of, n_bins))

    def self_correlations(self, box_inverse, indices, n_lags, bin_of=None, n_bins=0, idx=None):
        self._note("self_correlations", box_inverse, indices, n_lags, bin_of, n_bins, idx)
        return self._give(n_lags, self._cols(indices, bin_of, n_bins))


def calculator(engine=None, n_frames=T, n_atoms=N):
    rng = np.random.default_rng(7)
    pos = rng.uniform(0, SIDE, (n_frames, n_atoms, 3)).astype(np.float32)
    vel = rng.standard_normal((n_frames, n_atoms, 3)).astype(np.float32)
    box = np.diag(np.full(3, SIDE, np.float32))
    calc = SEDCalculator(Trajectory(pos, vel, TYPES[:n_atoms].copy(), np.arange(n_frames, dtype=np.float32), box, np.diag(box).copy(),
                                    np.zeros(3, np.float32), DT), 1, 1, 1)
    return calc.attach(engine=engine) if engine is not None else calc


def first_argument(powder):
    return EDGES if powder else INDICES


# ------------------------------------------------------------------ the call sequence and the result
def options(kind, family, powder, full):
    """(keyword arguments, what they mean for the expectations) of the plain and of the full call of a method"""
    kw = dict(lags=3) if kind == "correlations" else {}
    if full:
        kw.update(atom_weights=WEIGHTS, segments=SEG, **(dict(seed=5) if family == "self" or powder else {}))
        kw.update(basis_atom_indices=[[0, 1], [3, 4, 5]] if family == "partial" else SUBSET)
        if family == "self":
            kw["max_atoms"] = 3
        else:
            kw["currents"] = False
        if powder:
            kw["max_per_bin"] = 3
    elif family == "partial":
        kw["basis_atom_types"] = [1, 2]
    return kw


def expected_vectors(powder, kw):
    """(indices int32, bin_of or None, n_bins, the result's fields about the vectors) by the documented definitions"""
    if not powder:
        k = 2 * np.pi * INDICES / SIDE
        return INDICES.astype(np.int32), None, 0, dict(k_vectors=k, k_points=np.linalg.norm(k, axis=1))
    keep = np.ones(9, bool)
    if kw.get("max_per_bin") == 3:                          # the first shell holds 3 and is taken whole; 3 of the second are drawn
        rng = np.random.default_rng(kw["seed"])
        keep[3:] = False
        keep[rng.choice(np.arange(3, 9), 3, replace=False)] = True
    n, b = SHELL_N[keep], SHELL_B[keep]
    used = np.bincount(b, minlength=2)
    q = np.bincount(b, weights=G1 * np.linalg.norm(n, axis=1), minlength=2) / used
    return n, b, 2, dict(q=q, q_edges=EDGES, counts=2 * used, available=np.array([6, 12]), indices=n, bin_index=b)


@pytest.mark.parametrize("full", [False, True], ids=["plain", "full"])
@pytest.mark.parametrize("method", METHODS)
def test_call_sequence_and_result(method, full):
    kind, family, powder = METHODS[method]
    kw = options(kind, family, powder, full)
    eng = Recorder()
    calc = calculator(eng)
    res = getattr(calc, method)(first_argument(powder), **kw)
    currents = family != "self" and kw.get("currents", True)
    L = 8 if full else T
    rows = 3 if kind == "correlations" else L
    n, b, n_bins, about = expected_vectors(powder, kw)

    if family == "partial":
        listed = [np.array([0, 1]), np.array([3, 4, 5])] if full else [np.arange(3), np.arange(3, 8)]
    elif not full:
        listed = None                                       # all atoms in order
    elif family == "self":                                  # 3 of the 5, drawn by `seed`, in the order of the set
        listed = np.array(SUBSET)[np.sort(np.random.default_rng(5).choice(5, 3, replace=False))]
    else:
        listed = np.array(SUBSET)
    w32 = WEIGHTS.astype(np.float32)
    middle = (n, rows) if kind == "correlations" else (n,)
    entry = (ENTRY[kind, family], np.linalg.inv(np.eye(3) * SIDE)) + middle
    entry += (listed, b, n_bins, currents) if family == "partial" else (b, n_bins, listed) + ((currents,) if family == "coherent" else ())
    want = []
    if full:
        want += [("set_atom_weights", w32), ("set_segments", SEG)]
    want.append(("ensure_resident", _hip.SLOT_POSITIONS, calc.traj.positions))
    if currents:
        want.append(("ensure_resident", _hip.SLOT_VELOCITIES, calc.traj.velocities))
    want.append(entry)
    if full:
        want += [("set_atom_weights", None), ("set_segments", None)]
    assert eng.log == [(c[0],) + tuple(frozen(a) for a in c[1:]) for c in want]

    assert type(res) is RESULT[kind, family][powder]
    block = eng.returned[None] if family == "self" else eng.returned
    assert block.shape[0] == (3 if currents else 1) and block.shape[-2:] == (rows, n_bins if powder else 3)
    for i, field in enumerate(("density", "longitudinal", "transverse")):
        got = getattr(res, field)
        assert (got is None) if i >= block.shape[0] else (got.dtype == np.float32 and np.array_equal(got, block[i]))
    if kind == "spectra":
        assert np.array_equal(res.freqs, np.fft.fftfreq(L, DT))
    else:
        n_seg = 3 if full else 1
        assert np.array_equal(res.times, np.arange(3) * DT) and res.origins.dtype == np.int64
        assert np.array_equal(res.origins, n_seg * (L - np.arange(3)))
    for name, value in about.items():
        got = getattr(res, name)
        assert got.shape == np.shape(value) and np.allclose(got, value, rtol=1e-14, atol=0), name
        if name in ("indices", "bin_index"):
            assert got.dtype == np.int32
    w2 = WEIGHTS.astype(np.float32).astype(np.float64) ** 2 if full else np.ones(N)
    if family == "partial":
        assert len(res.groups) == 2 and all(np.array_equal(g, e) for g, e in zip(res.groups, listed))
        assert np.allclose(res.weight_norms, [w2[g].sum() for g in listed], rtol=1e-14)
        assert np.array_equal(res.pairs, [[0, 0], [0, 1], [1, 1]])
    else:
        atoms = np.arange(N) if listed is None else listed
        assert np.array_equal(res.atoms, atoms) and res.weight_norm == pytest.approx(w2[atoms].sum(), rel=1e-14)
    assert res.dt_ps == DT


@pytest.mark.parametrize("method", METHODS)
def test_state_is_cleared_when_the_entry_raises(method):
    kind, family, powder = METHODS[method]
    eng = Recorder(fail=ENTRY[kind, family])
    with pytest.raises(RuntimeError, match="planted"):
        getattr(calculator(eng), method)(first_argument(powder), **options(kind, family, powder, True))
    assert [c[0] for c in eng.log[-3:]] == [ENTRY[kind, family], "set_atom_weights", "set_segments"]
    assert eng.log[-2][1] == frozen(None) and eng.log[-1][1] == frozen(None)


def test_dynamic_spectra_shares_the_run():
    eng = Recorder()
    calc = calculator(eng)
    k = (2 * np.pi * INDICES / SIDE).astype(np.float32)
    res = calc.calculate_dynamic_spectra(np.linalg.norm(k, axis=1), k, SUBSET, atom_weights=WEIGHTS, segments=SEG)
    assert [c[0] for c in eng.log] == ["set_atom_weights", "set_segments", "ensure_resident", "ensure_resident", "dynamic_spectra",
                                       "set_atom_weights", "set_segments"]
    assert eng.log[4][1:] == (frozen(k), frozen(np.array(SUBSET)), frozen(True))
    assert all(np.array_equal(getattr(res, f), eng.returned[i]) for i, f in enumerate(("density", "longitudinal", "transverse")))


# ------------------------------------------------------------------ the order of the refusals
# fault -> (keyword arguments, the exception); a fault of the first argument is keyed "first"
FAULTS = {
    "weights": (dict(atom_weights=np.ones(N - 1)), (ValueError, r"atom_weights must have shape \(8,\)")),
    "segments_type": (dict(segments=(8, 4)), (TypeError, "segments must be a psa_amd.Segments, got tuple")),
    "tapered": (dict(segments=Segments(8, 4, "hann")), (ValueError, "time correlations need boxcar segments")),
    "too_long": (dict(segments=Segments(32, 16, "boxcar")), (ValueError, "segment length 32 exceeds the trajectory's 16 frames")),
    "lags": (dict(lags=0), (ValueError, r"lags = 0 is outside \[1, L = ")),
    "indices": (dict(first=INDICES + 0.5), (ValueError, "indices must be integers")),
    "edges": (dict(first=EDGES[::-1]), (ValueError, "q_edges must be at least two finite")),
    "max_per_bin": (dict(max_per_bin=0), (ValueError, "max_per_bin must be at least 1, got 0")),
    "max_atoms": (dict(max_atoms=0), (ValueError, "max_atoms must be an integer of at least 1, got 0")),
    "atoms": (dict(basis_atom_indices=[0, N]), (ValueError, "Atom indices in basis out of bounds")),
}
ORDER = {"spectra": ["weights", "segments_type", "indices", "edges", "max_per_bin", "too_long", "max_atoms", "atoms"],
         "correlations": ["weights", "segments_type", "tapered", "too_long", "lags", "indices", "edges", "max_per_bin", "max_atoms", "atoms"]}


def faults_of(kind, family, powder):
    skip = {"edges", "max_per_bin"} if not powder else {"indices"}
    if family != "self":
        skip.add("max_atoms")
    return [f for f in ORDER[kind] if f not in skip]


def both(earlier, later):
    """the keyword arguments of two simultaneous faults, or None where one argument cannot carry both"""
    a, b = FAULTS[earlier][0], FAULTS[later][0]
    if {earlier, later} == {"tapered", "too_long"}:
        return dict(segments=Segments(32, 16, "hann"))
    return None if set(a) & set(b) else {**a, **b}


@pytest.mark.parametrize("method", METHODS)
def test_refusal_precedence(method):
    kind, family, powder = METHODS[method]
    faults = faults_of(kind, family, powder)
    eng = Recorder()
    calc = calculator(eng)
    tried = 0
    for earlier, later in [(f, f) for f in faults] + list(itertools.combinations(faults, 2)):
        kw = both(earlier, later) if earlier != later else dict(FAULTS[earlier][0])
        if kw is None:
            continue
        if kind == "correlations":
            kw.setdefault("lags", 3)
        error, text = FAULTS[earlier][1]
        with pytest.raises(error, match=text):
            getattr(calc, method)(kw.pop("first", first_argument(powder)), **kw)
        tried += 1
    assert tried >= len(faults) * (len(faults) + 1) // 2 - 3 and eng.log == []      # no device was touched


def test_the_two_spellings_of_the_name(caplog):
    class TwoRanks:
        nranks, mode, engine = 2, "k", None
    for method, (kind, family, powder) in METHODS.items():
        name = method[len("calculate_"):].replace("_", " ")
        calc = calculator()
        with caplog.at_level("WARNING"):
            getattr(calc, method)(np.array([0.01, 0.02]) if powder else np.zeros((0, 3), int))
        assert f"Cannot calculate {name}: 0 frames, 0 atoms or 0 k-vectors." in caplog.text
        calc._shard = TwoRanks()
        with pytest.raises(NotImplementedError, match=f"^the {name} are not available on a sharded calculator$"):
            getattr(calc, method)(first_argument(powder))
        assert calc._engine is None


# ------------------------------------------------------------------ the empty inputs
EMPTY = [(m, why, c) for m in METHODS for why in ("no vectors", "no frames", "no atoms")
         for c in ((True, False) if METHODS[m][1] != "self" else (False,))]       # (the self methods take no `currents`)


@pytest.mark.parametrize("method,why,currents", EMPTY, ids=["-".join(map(str, e)) for e in EMPTY])
def test_empty_inputs(method, why, currents):
    kind, family, powder = METHODS[method]
    calc = calculator(n_frames=0 if why == "no frames" else T, n_atoms=0 if why == "no atoms" else N)
    kw = dict(lags=5) if kind == "correlations" else {}
    if family != "self":
        kw["currents"] = currents
    first = first_argument(powder)
    if why == "no vectors":
        first = np.array([0.01, 0.02, 0.03]) if powder else np.zeros((0, 3), int)
    res = getattr(calc, method)(first, **kw)
    assert calc._engine is None and type(res) is RESULT[kind, family][powder]
    frames = 0 if why == "no frames" else T
    rows = (5 if frames else 0) if kind == "correlations" else frames
    cols = 2 if powder else (0 if why == "no vectors" else 3)
    shape = ((1,) if family == "partial" else ()) + (rows, cols)
    for i, field in enumerate(("density", "longitudinal", "transverse")):
        got = getattr(res, field)
        if i and not currents:
            assert got is None
        else:
            assert got.dtype == np.float32 and got.shape == shape and not got.any()
    if kind == "spectra":
        assert res.freqs.dtype == np.float64 and res.freqs.shape == (rows,)
    else:
        assert res.times.dtype == np.float64 and res.origins.dtype == np.int64 and res.times.shape == res.origins.shape == (rows,)
    if family == "partial":
        assert len(res.groups) == 1 and res.groups[0].shape == (0,) and res.groups[0].dtype == np.dtype(int)
        assert np.array_equal(res.weight_norms, np.zeros(1)) and np.array_equal(res.pairs, [[0, 0]])
    else:
        assert res.atoms.shape == (0,) and res.atoms.dtype == np.dtype(int) and res.weight_norm == 0.0
    if powder:
        populated = why != "no vectors"
        assert np.array_equal(res.counts, [6, 12] if populated else [0, 0]) and res.indices.shape == (9 if populated else 0, 3)
    else:
        assert res.k_vectors.shape == (cols, 3) and res.k_points.shape == (cols,)


# ------------------------------------------------------------------ the structure factor's time step
def test_structure_factor_time_step():
    den = np.arange(8, dtype=np.float32).reshape(4, 2)
    freqs = np.fft.fftfreq(4, 0.5)
    for dt in (0.5, None):                                           # given, or read from freqs[1] = 1 / (L dt)
        dyn = DynamicSpectra(den, None, None, freqs, np.zeros(2), np.zeros((2, 3)), np.arange(3), 3.0, dt)
        pw = PowderSpectra(den, None, None, np.zeros(2), np.zeros(3), np.ones(2), np.ones(2), np.zeros((2, 3), np.int32),
                           np.zeros(2, np.int32), freqs, np.arange(3), 3.0, dt)
        par = PartialSpectra(den[None], None, None, np.array([[0, 0]]), [np.arange(3)], np.array([3.0]), freqs, np.zeros(2),
                             np.zeros((2, 3)), dt)
        for got in (dyn.structure_factor, pw.structure_factor, par.structure_factor[0]):
            assert got.dtype == np.float64 and np.array_equal(got, den.astype(np.float64) * (4 * 0.5 / 3.0))
    one = DynamicSpectra(den[:1], None, None, freqs[:1], np.zeros(2), np.zeros((2, 3)), np.arange(3), 3.0, None)
    with pytest.raises(ValueError, match="structure_factor needs dt_ps: the frequencies of a one-bin spectrum hold no time step"):
        one.structure_factor


# ------------------------------------------------------------------ the signatures
_ATOMS = ("basis_atom_indices: 'Optional[Union[List[int], List[List[int]], np.ndarray]]' = None, "
          "basis_atom_types: 'Optional[Union[List[int], List[List[int]]]]' = None, *, atom_weights: 'Optional[np.ndarray]' = None, ")
_SEG, _LAGS, _CUR = "segments: 'Optional[Segments]' = None", "lags: 'Optional[int]' = None, ", ", currents: 'bool' = True"
_BIN, _MAX, _SEED = ", max_per_bin: 'Optional[int]' = None", ", max_atoms: 'Optional[int]' = None", ", seed: 'int' = 0"
_N, _Q = "(self, indices: 'np.ndarray', ", "(self, q_edges: 'np.ndarray', "
SIGNATURES = {
    "calculate_lattice_spectra": _N + _ATOMS + _SEG + _CUR + ") -> 'DynamicSpectra'",
    "calculate_powder_spectra": _Q + _ATOMS + _SEG + _CUR + _BIN + _SEED + ") -> 'PowderSpectra'",
    "calculate_self_spectra": _N + _ATOMS + _SEG + _MAX + _SEED + ") -> 'DynamicSpectra'",
    "calculate_powder_self_spectra": _Q + _ATOMS + _SEG + _BIN + _MAX + _SEED + ") -> 'PowderSpectra'",
    "calculate_partial_spectra": _N + _ATOMS + _SEG + _CUR + ") -> 'PartialSpectra'",
    "calculate_powder_partial_spectra": _Q + _ATOMS + _SEG + _CUR + _BIN + _SEED + ") -> 'PowderPartialSpectra'",
    "calculate_lattice_correlations": _N + _ATOMS + _LAGS + _SEG + _CUR + ") -> 'TimeCorrelations'",
    "calculate_powder_correlations": _Q + _ATOMS + _LAGS + _SEG + _CUR + _BIN + _SEED + ") -> 'PowderTimeCorrelations'",
    "calculate_self_correlations": _N + _ATOMS + _LAGS + _SEG + _MAX + _SEED + ") -> 'TimeCorrelations'",
    "calculate_powder_self_correlations": _Q + _ATOMS + _LAGS + _SEG + _BIN + _MAX + _SEED + ") -> 'PowderTimeCorrelations'",
}
ENGINE_SIGNATURES = {
    "lattice_spectra": "(self, box_inverse, indices, bin_of=None, n_bins=0, idx=None, currents: 'bool' = True) -> 'np.ndarray'",
    "self_spectra": "(self, box_inverse, indices, bin_of=None, n_bins=0, idx=None) -> 'np.ndarray'",
    "partial_spectra": "(self, box_inverse, indices, species, bin_of=None, n_bins=0, currents: 'bool' = True) -> 'np.ndarray'",
    "lattice_correlations": "(self, box_inverse, indices, n_lags: 'int', bin_of=None, n_bins=0, idx=None, currents: 'bool' = True) -> 'np.ndarray'",
    "self_correlations": "(self, box_inverse, indices, n_lags: 'int', bin_of=None, n_bins=0, idx=None) -> 'np.ndarray'",
}


def test_signatures():
    assert set(SIGNATURES) == set(METHODS) and set(ENGINE_SIGNATURES) == set(ENTRY.values())
    for name, text in SIGNATURES.items():
        assert str(inspect.signature(getattr(SEDCalculator, name))) == text, name
    for name, text in ENGINE_SIGNATURES.items():
        assert str(inspect.signature(getattr(_hip.Engine, name))) == text, name
        assert set(inspect.signature(getattr(Recorder, name)).parameters) == set(inspect.signature(getattr(_hip.Engine, name)).parameters)


# ------------------------------------------------------------------ the Engine entries' one marshalling
class _Library:
    """libpsa_hip's stand-in under `Engine`: every entry logs its arguments -- what a pointer points at by dtype and bytes"""

    def __init__(self):
        self.log = []

    def __getattr__(self, name):
        def entry(*args):
            self.log.append((name,) + args)
            return 0
        return entry


def _engine(length=None):
    eng = object.__new__(_hip.Engine)
    eng._lib, eng._h, eng.segment_length = _Library(), 77, length
    eng.shape = lambda slot: (T, N)
    return eng


def _at(pointer, dtype, count):
    return np.ctypeslib.as_array(pointer, (count,)).astype(dtype).tolist()


def test_index_args_keep_a_valid_pointer():
    assert _hip.Engine._index_args(None) == (None, None, 0)
    keep, pointer, n = _hip.Engine._index_args(np.array([3, 1], np.int64))
    assert keep.dtype == np.int32 and keep.tolist() == [3, 1] and n == 2 and _at(pointer, np.int32, 2) == [3, 1]
    keep, pointer, n = _hip.Engine._index_args(np.zeros(0, int))
    assert keep.shape == (1,) and n == 0 and pointer                     # the dummy element: a pointer that may be passed
    assert _hip.Engine._dynamic_args(np.zeros(3), None)[1:] == (None, None, 0)
    assert _hip.Engine._dynamic_args(np.zeros((2, 3)), np.zeros(0, int))[1].shape == (1,)
    flat = _hip.Engine._displacement_args(np.eye(3), None, [np.zeros(0, int), np.zeros(0, int)])
    assert flat[2].shape == (1,) and flat[4].tolist() == [0, 0, 0] and flat[6] == 2


@pytest.mark.parametrize("entry", ENTRY.values())
@pytest.mark.parametrize("shells", [False, True])
def test_engine_entries_marshal_alike(entry, shells):
    eng = _engine(length=8)
    inv, n = np.eye(3) * 0.1, SHELL_N[:4]
    bins = dict(bin_of=[0, 0, 1, 1], n_bins=2) if shells else {}
    lags = (3,) if "correlations" in entry else ()
    if entry == "partial_spectra":
        out = eng.partial_spectra(inv, n, [[0, 1], [], [5]], currents=False, **bins)
        atoms_at, lead = 6, (1, 6)
    elif entry.startswith("self"):
        out = getattr(eng, entry)(inv, n, *lags, idx=[2, 6], **bins)
        atoms_at, lead = 6, ()
    else:
        out = getattr(eng, entry)(inv, n, *lags, idx=[2, 6], **bins)
        atoms_at, lead = 6, (3,)
    assert out.dtype == np.float32 and out.shape == lead + (3 if lags else 8, 2 if shells else 4)
    (call,) = eng._lib.log
    assert call[0] == "psa_" + entry and call[1] == 77 and call[4] == 4 and call[6] == (2 if shells else 0)
    assert _at(call[2], np.float64, 9) == inv.ravel().tolist() and _at(call[3], np.int32, 12) == n.ravel().tolist()
    assert (_at(call[5], np.int32, 4) == [0, 0, 1, 1]) if shells else (call[5] is None)
    if entry == "partial_spectra":
        assert _at(call[7], np.int32, 3) == [0, 1, 5] and _at(call[8], np.int64, 4) == [0, 2, 2, 3] and call[9:11] == (3, 0)
        tail = call[11:]
    else:
        assert _at(call[7], np.int32, 2) == [2, 6] and call[8] == 2
        tail = call[9:]
    middle = {"lattice_spectra": (1,), "self_spectra": (), "partial_spectra": (), "lattice_correlations": (1, 3), "self_correlations": (3,)}[entry]
    assert tail[:-2] == middle and tail[-1] == out.nbytes
    assert np.ctypeslib.as_array(tail[-2], out.shape).ctypes.data == out.ctypes.data


def test_engine_entries_refuse_as_before():
    eng = _engine()
    for entry in ENTRY.values():
        lags = (3,) if "correlations" in entry else ()
        who = ([[0]],) if entry == "partial_spectra" else ()
        with pytest.raises(ValueError, match=r"box_inverse must be \(3, 3\), got \(2, 2\)"):
            getattr(eng, entry)(np.eye(2), SHELL_N, *who, *lags)
        with pytest.raises(ValueError, match="bin_of has 2 entries for 9 vectors"):
            getattr(eng, entry)(np.eye(3), SHELL_N, *who, *lags, bin_of=[0, 1], n_bins=2)
    with pytest.raises(ValueError, match="1 to 8 species are served, got 0"):
        eng.partial_spectra(np.eye(3), SHELL_N, [])
    assert eng._lib.log == []
