"""Cases and the comparison helper of tests/test_gpu_scratch_history.py: no result may depend on what the context's
scratch memory held before the call.

A case is one entry-point call -- for the entries that come as a sequence (project + finalize, fs_project .. fs_finish)
the whole sequence -- that sets everything it depends on itself: options, K1 selector, atom weights, segments, the
resident arrays.  It is run at two sizes.  The small one is the smallest ragged shape that still reaches the code path:
130 atoms (two species: 90 + 40, angle_cases.two_species), 100 frames (no multiple of 16 or 64), Segments(32, 16, "hann")
-- the boxcar window for the time correlations, which refuse any other -- and the k-list length that selects the form.
The streamed upload alone needs 700 atoms: below 8 KiB per frame its smallest chunk holds all 100 frames.  The loud one
is what runs BEFORE the small one in the history test: 257 atoms, 160 frames, a longer k-list or more bins, another
group layout (three interleaved groups where the small call has two blocks, or none), velocities and atom weights
scaled by 2^20.  Positions are not scaled: a position is only meaningful inside its box, so the loud positions are moved
by whole box vectors instead.

compare / first_difference: bit for bit over every returned array, and finite wherever the first result is finite.
tests/test_scratch_table_host.py shows with a stub engine that the helper reports the element that differs."""
import os

import numpy as np

import angle_cases
import lattice_cases as LC
import lowrank_cases as LR
import pair_cases

SMALL = dict(N=130, T=100)
LOUD = dict(N=257, T=160)
LOUD_SCALE = np.float32(2.0 ** 20)
BOX = LC.CUBIC
FILL_BYTES = (0x00, 0xFF)               # 0xFF..FF is a NaN as float16, float32 and float64


# ---- the comparison helper ---------------------------------------------------------------------------------------------
class Differs(AssertionError):
    """two runs of a case differ: `array` (position in the returned list), `element` (index tuple), `want`, `got`"""

    def __init__(self, text, array, element, want, got):
        super().__init__(text)
        self.array, self.element, self.want, self.got = array, element, want, got


def as_arrays(result):
    """what a case returned as a flat list of arrays (None left out; a PeakFit by its fields)"""
    if result is None:
        return []
    if isinstance(result, np.ndarray):
        return [result]
    if isinstance(result, (tuple, list)):
        return [a for r in result for a in as_arrays(r)]
    if hasattr(result, "__dataclass_fields__"):
        return [np.asarray(getattr(result, f)) for f in result.__dataclass_fields__]
    return [np.asarray(result)]


def first_difference(want, got):
    """None, or (array, element, want value, got value, reason) of the first element that differs in its bits, or is not
    finite where `want` is"""
    assert len(want) == len(got), (len(want), len(got))
    for i, (a, b) in enumerate(zip(want, got)):
        assert a.shape == b.shape and a.dtype == b.dtype, (i, a.shape, b.shape, a.dtype, b.dtype)
        if a.size == 0:
            continue
        a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
        rows_a = a.reshape(-1).view(np.uint8).reshape(a.size, a.itemsize)
        rows_b = b.reshape(-1).view(np.uint8).reshape(b.size, b.itemsize)
        bad = np.any(rows_a != rows_b, axis=1)
        if a.dtype.kind in "fc":
            bad |= (np.isfinite(a) & ~np.isfinite(b)).reshape(-1)
        if bad.any():
            flat = int(np.argmax(bad))
            el = tuple(int(v) for v in np.unravel_index(flat, a.shape))
            return i, el, a.reshape(-1)[flat], b.reshape(-1)[flat], f"{int(bad.sum())} of {a.size} elements differ"
    return None


def compare(name, step, want, got, note=""):
    """prints `name step: equal`, or raises Differs naming the first element that differs"""
    d = first_difference(want, got)
    if d is None:
        print(f"{name} {step}{note}: equal")
        return
    i, el, w, g, how = d
    text = f"{name} {step}{note}: array {i} element {el}: {g!r} where the first run gave {w!r} ({how})"
    print(text)
    raise Differs(text, i, el, w, g)


def check_poisoned(engine, name, call, r0):
    """(b): scratch_fill(byte) then call() equals r0, for the zero pattern and the NaN pattern; the hook must have filled
    something.  Returns the (buffers, bytes) of the last fill."""
    filled = (0, 0)
    for byte in FILL_BYTES:
        filled = engine.scratch_fill(byte)
        assert filled[0] > 0 and filled[1] > 0, f"{name}: scratch_fill(0x{byte:02X}) filled {filled}: the hook did nothing"
        got = as_arrays(call(engine))
        compare(name, f"after scratch_fill(0x{byte:02X})", r0, got, f" [{filled[0]} buffers, {filled[1]} bytes filled]")
    return filled


# ---- inputs --------------------------------------------------------------------------------------------------------------
_INPUTS = {}


def _memo(key, make):
    if key not in _INPUTS:
        _INPUTS[key] = make()
    return _INPUTS[key]


def shape(loud, N=None):
    s = LOUD if loud else SMALL
    return (N or s["N"]), s["T"]


def velocities(loud, N=None, seed=1):
    """(T, N, 3) float32, standard normal, times 2^20 when loud"""
    n, t = shape(loud, N)

    def make():
        v = np.random.default_rng(seed + 100 * loud).standard_normal((t, n, 3)).astype(np.float32)
        return v * LOUD_SCALE if loud else v
    return _memo(("vel", loud, n, seed), make)


def sites(loud, N=None):
    """(N, 3) float32 mean positions scattered over the 40 A box centred on the origin (lowrank_cases.box)"""
    n, _ = shape(loud, N)
    return _memo(("sites", loud, n), lambda: LR.box(n, 40.0, 3 + loud, -20.0))


def walk(loud, kind="wrapped"):
    """(T, N, 3) float32 positions of a random walk in BOX (pair_cases.walk): wrapped; loud: moved by whole box vectors"""
    n, t = shape(loud)
    return _memo(("walk", loud, kind), lambda: np.ascontiguousarray(pair_cases.walk(n, t, 7 + loud, box=BOX)["moved" if loud and kind == "wrapped" else kind]))


def lattice_traj(loud):
    """(positions, velocities) of lattice_cases.trajectory in BOX; loud: shifted by up to 2 box vectors, velocities x 2^20"""
    n, t = shape(loud)

    def make():
        pos, vel = LC.trajectory(n, t, 5 + loud, box=BOX, shift=2 if loud else 0)
        return pos, (vel * LOUD_SCALE if loud else vel)
    return _memo(("lat", loud), make)


def k_random(K, seed=2):
    return _memo(("k", K, seed), lambda: (np.random.default_rng(seed).uniform(-1.5, 1.5, (K, 3))).astype(np.float32))


def k_path(K):
    return _memo(("kpath", K), lambda: LR.path([1, -1, 0], 0.0, 1.5, K))


def groups_of(loud, layout):
    """None: all atoms; "list": one index list with a duplicate; "two": two species (small: 90 + 40; loud: three
    interleaved groups, the other layout)"""
    n, _ = shape(loud)
    if layout is None:
        return None
    if layout == "list":
        idx = np.random.default_rng(9 + loud).choice(n, n // 2 + 3, replace=False).astype(np.int32)
        idx[5] = idx[6]
        return [idx]
    if loud:
        return [np.arange(i, n, 3, dtype=np.int32) for i in range(3)]
    return [g.astype(np.int32) for g in angle_cases.two_species(n)]


def species_of(loud):
    """disjoint species for the partial spectra and the real-space entries: two (small), three interleaved (loud)"""
    return groups_of(loud, "two")


def weights_of(loud, N=None):
    n, _ = shape(loud, N)
    w = LR.mass_weights(n, 4 + loud)
    return w * LOUD_SCALE if loud else w


def segments_of(loud, window="hann"):
    from psa_amd import Segments
    return Segments(48, 16, window) if loud else Segments(32, 16, window)


# ---- the state every case sets itself ----------------------------------------------------------------------------------
def prepare(engine, options=(), k1=None, weights=None, segments=None):
    """every option at its default, then `options`; planes for every group at first sight (so that the first call takes the
    route the second takes); the selector, the weights and the segments of the case"""
    from psa_amd import _hip
    engine.reset_options()
    for opt, val in ((_hip.OPT_PLANES_EAGER, 1), (_hip.OPT_PLANES_MIN_K, 1)) + tuple(options):
        engine.set_option(opt, val)
    engine.set_k1(_hip.K1_AUTO if k1 is None else k1)
    engine.set_atom_weights(weights)
    engine.set_segments(segments)


def _copy(result):
    return [np.array(a, copy=True) for a in as_arrays(result)]


# ---- SED: Engine.calculate / project / finalize ----------------------------------------------------------------------------
# form: (K small, K loud, options)
def _sed_forms():
    from psa_amd import _hip
    P, W, LW = _hip.OPT_PLANES, _hip.OPT_K1_WIDE, _hip.OPT_K1_LOADER_WAVES
    LO, LP = _hip.OPT_K1_LOWRANK, _hip.OPT_K1_LOWRANK_PAIR
    low = ((_hip.OPT_K1_LOWRANK_MIN_K, 1), (_hip.OPT_K1_LOWRANK_MIN_LOCAL, 1))
    return {
        "bf16_K9": (9, 15, ((P, 0), (LO, 0))),
        "planes64_K24": (24, 31, ((P, 1), (W, 0), (LW, 0), (LO, 0))),
        "planes128_K40": (40, 100, ((P, 1), (W, 0), (LW, 0), (LO, 0))),
        "fly_K40": (40, 100, ((P, 0), (LO, 0))),
        "wide_K128": (128, 192, ((P, 1), (W, 1), (LW, 0), (LO, 0))),
        "lw_K40": (40, 100, ((P, 1), (W, 0), (LW, 1), (LO, 0))),
        "lowrank_K64": (64, 300, ((P, 1), (LO, 1), (LP, 0)) + low),
        "lowrank_pair_K64": (64, 200, ((P, 1), (LO, 1), (LP, 1)) + low),
    }


def sed_case(form, layout=None, disp=False, weighted=False, segmented=False, intensity=False, chiral=False, two_calls=False):
    """one SED case: the form's options, then calculate (or project + finalize for the low-rank route and with
    `two_calls`), with the modifiers; chiral: the complex result's intensity and chiral phase as well"""
    def call(engine, loud=False):
        from psa_amd import _hip
        k_small, k_loud, options = _sed_forms()[form]
        K = k_loud if loud else k_small
        lowrank = form.startswith("lowrank")
        k = k_path(K) if lowrank else k_random(K)
        x = walk(loud, "unwrapped") if disp else velocities(loud)
        r = x.mean(axis=0).astype(np.float32) if disp else sites(loud)
        slot = _hip.SLOT_POSITIONS if disp else _hip.SLOT_VELOCITIES
        flags = (_hip.F_DISPLACEMENTS if disp else 0) | (_hip.F_INTENSITY if intensity or segmented else 0)
        seg = segments_of(loud) if segmented else None
        prepare(engine, options, None, weights_of(loud) if weighted else None, seg)
        engine.ensure_resident(slot, x)
        groups = groups_of(loud, layout)
        T = seg.length if seg else x.shape[0]
        n_lr, n_pair = engine.lowrank_launches(), engine.lowrank_pair_launches()
        if lowrank or two_calls:
            cut = K // 2 if two_calls else K
            for lo, hi in ((0, cut), (cut, K)):
                if hi > lo:
                    engine.project(slot, r, k[lo:hi], groups, flags, K_total=K, k_offset=lo)
            out = [engine.finalize(T, K, bool(flags & _hip.F_INTENSITY))]
        else:
            out = [engine.calculate(slot, r, k, groups, flags, with_intensity=chiral)]
        if chiral:
            out += [engine.result_intensity(T, K), engine.result_chiral_phase(T, K, 0, 1)]
        if lowrank:
            assert engine.lowrank_launches() > n_lr, f"{form}: the low-rank route was not taken"
            assert (engine.lowrank_pair_launches() > n_pair) == (form == "lowrank_pair_K64"), f"{form}: pair launches"
        else:
            assert engine.lowrank_launches() == n_lr, f"{form}: the low-rank route was taken"
        planes = dict(options).get(_hip.OPT_PLANES, 1)
        assert (engine.plane_cache()[0] > 0) == bool(planes), f"{form}: {engine.plane_cache()[0]} plane sets cached"
        return _copy(out)
    return call


def single_bin(engine, loud=False):
    from psa_amd import _hip
    prepare(engine)
    x = velocities(loud)
    engine.ensure_resident(_hip.SLOT_VELOCITIES, x)
    g = groups_of(loud, "list")[0]
    return _copy([engine.single_bin(_hip.SLOT_VELOCITIES, sites(loud), k_random(9)[3], g, 7),
                  engine.single_bin(_hip.SLOT_VELOCITIES, sites(loud), k_random(9)[4], None, x.shape[0] - 1)])


def project_upload(engine, loud=False):
    """psa_sed_project_upload in two chunks of 64 and 36 frames (loud: 64, 64, 32): 700 atoms, a 1 MiB chunk target"""
    from psa_amd import _hip
    prepare(engine)
    x = velocities(loud, N=900 if loud else 700, seed=3)
    K = 40 if loud else 24
    old = os.environ.get("PSA_UPLOAD_CHUNK_MIB")
    os.environ["PSA_UPLOAD_CHUNK_MIB"] = "1"
    try:
        engine.project_upload(_hip.SLOT_VELOCITIES, np.array(x), sites(loud, x.shape[1]), k_random(K))
    finally:
        if old is None:
            del os.environ["PSA_UPLOAD_CHUNK_MIB"]
        else:
            os.environ["PSA_UPLOAD_CHUNK_MIB"] = old
    out = engine.finalize(x.shape[0], K, False)
    engine.invalidate(_hip.SLOT_VELOCITIES)
    return _copy(out)


def frame_sharded(engine, loud=False):
    """fs_project -> fs_read / fs_write -> fs_finish on one context: its own frames are all frames"""
    from psa_amd import _hip
    prepare(engine)
    x = velocities(loud)
    T, K = x.shape[0], (40 if loud else 24)
    engine.ensure_resident(_hip.SLOT_VELOCITIES, x)
    g = groups_of(loud, "list")[0]
    engine.fs_project(_hip.SLOT_VELOCITIES, sites(loud), k_random(K), g, 0, T, 0, K)
    q = engine.fs_read(0, K, T)
    engine.fs_write(0, q)
    engine.fs_finish(True)
    return _copy([q, engine.finalize(T, K, False)])


# ---- spectral --------------------------------------------------------------------------------------------------------------
def vdos_case(two, segmented):
    def call(engine, loud=False):
        from psa_amd import _hip
        prepare(engine, weights=weights_of(loud) if two else None, segments=segments_of(loud) if segmented else None)
        engine.ensure_resident(_hip.SLOT_VELOCITIES, velocities(loud))
        return _copy(engine.vdos(_hip.SLOT_VELOCITIES, None, groups_of(loud, "two") if two else None))
    return call


def _eig(K, M, B, seed=6):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((K, M, B, 3)) + 1j * rng.standard_normal((K, M, B, 3))).astype(np.complex64)


def modes_case(kind):
    """kind: modes, welch, covariance, modes_fit"""
    def call(engine, loud=False):
        from psa_amd import _hip
        welch = kind == "welch"
        prepare(engine, segments=segments_of(loud) if welch else None)
        x = velocities(loud)
        engine.ensure_resident(_hip.SLOT_VELOCITIES, x)
        groups = groups_of(loud, "two")
        K, M, B = (17 if loud else 9), (7 if loud else 5), len(groups)
        args = (_hip.SLOT_VELOCITIES, sites(loud), k_random(K), groups)
        if kind == "covariance":
            g = np.random.default_rng(8).uniform(0.0, 1.0, (2 if loud else 1, x.shape[0])).astype(np.float32)
            return _copy(engine.sed_covariance(*args, g))
        if kind == "modes_fit":
            fit, sed = engine.sed_modes_fit(*args, _eig(K, M, B), 0.1, return_sed=True)
            return _copy([fit, sed])
        return _copy((engine.sed_modes_welch if welch else engine.sed_modes)(*args, _eig(K, M, B)))
    return call


def fit_peaks(engine, loud=False):
    prepare(engine)
    F, C = (257, 70) if loud else (100, 9)
    f = np.arange(F, dtype=np.float64)[:, None]
    rng = np.random.default_rng(10 + loud)
    f0, w, h = rng.uniform(0.15 * F, 0.35 * F, C), rng.uniform(1.0, 3.0, C), rng.uniform(1.0, 5.0, C) * (float(LOUD_SCALE) if loud else 1.0)
    spec = (h * w * w / ((f - f0) ** 2 + w * w) + 0.01 * h * rng.uniform(0.0, 1.0, (F, C))).astype(np.float32)
    return _copy(engine.fit_peaks(spec, 0.1))


# ---- reciprocal ------------------------------------------------------------------------------------------------------------
def _resident_pair(engine, loud):
    from psa_amd import _hip
    pos, vel = lattice_traj(loud)
    engine.ensure_resident(_hip.SLOT_POSITIONS, pos)
    engine.ensure_resident(_hip.SLOT_VELOCITIES, vel)


def _shell_vectors(K, n_bins):
    """(indices of half-space members, sorted by bin; bin_of)"""
    n = LC.mixed_indices(4 * K, 12)
    lead = np.where(n[:, 0] != 0, n[:, 0], np.where(n[:, 1] != 0, n[:, 1], n[:, 2]))
    n = n[lead > 0][:K]
    assert len(n) == K
    bin_of = np.sort(np.random.default_rng(13).integers(0, n_bins, K)).astype(np.int32)
    bin_of[bin_of == 2] = 3                                  # an empty bin
    return n, bin_of


def reciprocal_case(entry, shell=False, currents=True, listed=False):
    """entry: dynamic, lattice, self, partial, lattice_corr, self_corr"""
    def call(engine, loud=False):
        corr = entry.endswith("corr")
        seg = segments_of(loud, "boxcar" if corr else "hann")
        prepare(engine, weights=weights_of(loud), segments=seg)
        _resident_pair(engine, loud)
        inv = LC.inverse(BOX)
        K, n_bins = (70, 9) if loud else (11, 5)
        idx = groups_of(loud, "list")[0] if listed else None
        if entry == "dynamic":
            return _copy(engine.dynamic_spectra(k_random(K, 14), idx, currents))
        n, bin_of = _shell_vectors(K, n_bins) if shell else (LC.mixed_indices(K, 15), None)
        nb = n_bins if shell else 0
        if entry == "lattice":
            return _copy(engine.lattice_spectra(inv, n, bin_of, nb, idx, currents))
        if entry == "self":
            return _copy(engine.self_spectra(inv, n, bin_of, nb, idx))
        if entry == "partial":
            return _copy(engine.partial_spectra(inv, n, species_of(loud), bin_of, nb, currents))
        n_lags = 20 if loud else 9
        if entry == "lattice_corr":
            return _copy(engine.lattice_correlations(inv, n, n_lags, bin_of, nb, idx, currents))
        return _copy(engine.self_correlations(inv, n, n_lags, bin_of, nb, idx))
    return call


# ---- real space ------------------------------------------------------------------------------------------------------------
def realspace_case(entry, two=True):
    """entry: moments, van_hove, pair, angle, order"""
    def call(engine, loud=False):
        from psa_amd import _hip
        prepare(engine)
        engine.ensure_resident(_hip.SLOT_POSITIONS, walk(loud))
        groups = species_of(loud) if two else None
        n_r = 200 if loud else 37
        dr = 0.45 * float(BOX[0, 0]) / n_r
        lags = [0, 3, 50] if loud else [0, 5]
        if entry == "moments":
            return _copy(engine.displacement_moments(BOX, 90 if loud else 33, groups, 1, True))
        if entry == "van_hove":
            return _copy(engine.van_hove_self(BOX, lags, dr, n_r, groups, 2, True))
        if entry == "pair":
            return _copy(engine.pair_histogram(BOX, lags, dr, n_r, groups, 3))
        if entry == "angle":
            return _copy(engine.angle_histogram(BOX, 6.0, 90 if loud else 19, groups, 3))
        return _copy(engine.bond_order(BOX, 6.0, [4, 6] if not loud else [2, 4, 6, 12], 64 if loud else 10, groups, 3, per_atom=True))
    return call


# ---- the table: name -> (entry family, call) -------------------------------------------------------------------------------
# The entry families name what shares device buffers: SHARING lists, per group of buffers, the families whose calls go
# through it; HISTORY[family] is the case that stands for the family in another family's history.
CASES = {
    # SED forms x modifiers: every form and every modifier at least once; the wide and low-rank forms with segments and
    # with an index list
    "sed bf16 K=9 complex chiral": ("sed", sed_case("bf16_K9", chiral=True)),
    "sed float32 K=9 displacements": ("sed", sed_case("bf16_K9", disp=True)),
    "sed planes64 K=24 index list": ("sed", sed_case("planes64_K24", layout="list")),
    "sed planes64 K=24 two calls weights": ("sed", sed_case("planes64_K24", weighted=True, two_calls=True)),
    "sed planes128 K=40 displacements": ("sed", sed_case("planes128_K40", disp=True)),
    "sed planes128 K=40 incoherent two groups": ("sed", sed_case("planes128_K40", layout="two", intensity=True)),
    "sed fly K=40 weights": ("sed", sed_case("fly_K40", weighted=True)),
    "sed fly K=40 segments": ("sed", sed_case("fly_K40", segmented=True)),
    "sed wide K=128 all atoms": ("sed", sed_case("wide_K128")),
    "sed wide K=128 segments index list": ("sed", sed_case("wide_K128", layout="list", segmented=True)),
    "sed wide K=128 incoherent two groups": ("sed", sed_case("wide_K128", layout="two", intensity=True, weighted=True)),
    "sed lw K=40 chiral": ("sed", sed_case("lw_K40", chiral=True)),
    "sed lw K=40 segments two groups": ("sed", sed_case("lw_K40", layout="two", segmented=True)),
    "sed lowrank K=64 all atoms": ("sed", sed_case("lowrank_K64")),
    "sed lowrank K=64 segments index list": ("sed", sed_case("lowrank_K64", layout="list", segmented=True)),
    "sed lowrank pair K=64 weights": ("sed", sed_case("lowrank_pair_K64", weighted=True)),
    "sed lowrank pair K=64 segments index list": ("sed", sed_case("lowrank_pair_K64", layout="list", segmented=True)),
    "sed lowrank pair K=64 displacements two groups": ("sed", sed_case("lowrank_pair_K64", layout="two", disp=True, intensity=True)),
    # other projection paths
    "single_bin": ("single_bin", single_bin),
    "project_upload two chunks": ("upload", project_upload),
    "fs_project fs_read fs_write fs_finish": ("fs", frame_sharded),
    # spectral
    "vdos one group": ("vdos", vdos_case(False, False)),
    "vdos one group segments": ("vdos", vdos_case(False, True)),
    "vdos two groups weights": ("vdos", vdos_case(True, False)),
    "vdos two groups weights segments": ("vdos", vdos_case(True, True)),
    "sed_modes": ("modes", modes_case("modes")),
    "sed_modes_welch": ("modes", modes_case("welch")),
    "sed_covariance": ("covariance", modes_case("covariance")),
    "fit_peaks": ("peaks", fit_peaks),
    "sed_modes_fit": ("modes", modes_case("modes_fit")),
    # reciprocal
    "dynamic_spectra currents": ("dynamic", reciprocal_case("dynamic")),
    "dynamic_spectra density index list": ("dynamic", reciprocal_case("dynamic", currents=False, listed=True)),
    "lattice_spectra per vector": ("lattice", reciprocal_case("lattice", listed=True)),
    "lattice_spectra shells": ("lattice", reciprocal_case("lattice", shell=True)),
    "self_spectra per vector": ("self", reciprocal_case("self")),
    "self_spectra shells": ("self", reciprocal_case("self", shell=True, listed=True)),
    "partial_spectra per vector": ("partial", reciprocal_case("partial")),
    "partial_spectra shells": ("partial", reciprocal_case("partial", shell=True, currents=False)),
    "lattice_correlations": ("correlations", reciprocal_case("lattice_corr", shell=True)),
    "self_correlations": ("correlations", reciprocal_case("self_corr", listed=True)),
    # real space
    "displacement_moments unwrap": ("msd", realspace_case("moments")),
    "van_hove_self": ("msd", realspace_case("van_hove")),
    "pair_histogram one species": ("pair", realspace_case("pair", two=False)),
    "pair_histogram two species": ("pair", realspace_case("pair")),
    "angle_histogram": ("angle", realspace_case("angle")),
    "bond_order per atom": ("order", realspace_case("order")),
}

SHARING = {
    "d_qwork, d_seg, d_modes_work": ("sed", "single_bin", "upload", "fs", "modes", "covariance", "dynamic", "lattice", "self",
                                     "partial", "correlations"),
    "d_rc_*": ("dynamic", "lattice", "self", "partial", "correlations"),
    "d_rs_*": ("msd", "pair", "angle", "order"),
}

HISTORY = {
    "sed": "sed planes128 K=40 incoherent two groups", "single_bin": "single_bin", "upload": "project_upload two chunks",
    "fs": "fs_project fs_read fs_write fs_finish", "modes": "sed_modes_welch", "covariance": "sed_covariance",
    "vdos": "vdos two groups weights segments", "peaks": "fit_peaks",
    "dynamic": "dynamic_spectra currents", "lattice": "lattice_spectra shells", "self": "self_spectra per vector",
    "partial": "partial_spectra per vector", "correlations": "lattice_correlations",
    "msd": "van_hove_self", "pair": "pair_histogram two species", "angle": "angle_histogram", "order": "bond_order per atom",
}

# the contexts of the fresh, armed run (c): one per row of the issue's table
FRESH = {
    "sed": ("sed",), "projection": ("single_bin", "upload", "fs"), "spectral": ("vdos", "modes", "covariance", "peaks"),
    "reciprocal": ("dynamic", "lattice", "self", "partial", "correlations"), "realspace": ("msd", "pair", "angle", "order"),
}


def others_sharing(family):
    """the other entry families that share a group of buffers with `family`, each once, in a fixed order"""
    out = []
    for members in SHARING.values():
        if family in members:
            out += [m for m in members if m != family and m not in out]
    return out
