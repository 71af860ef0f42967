"""The analysis entry points on a resident array past 2^32 elements (tests/bigslot_cases.py has the shape, the zones and
the cases; tests/test_bigslot_host.py the proof that a read through a wrapped index in any zone falls outside the
allowances applied here).  Both slots hold N = 2^20 + 3 atoms x T = 2304 frames of counter-hashed noise, 29.0 GB each,
generated in HBM; every entry point is called with index lists of a few hundred atoms, whose series the host rebuilds
from the same hash, and is compared
  * with the float64 reference of the compact (T, n_g, 3) array inside the allowance of the entry's own GPU test -- no
    tolerance is introduced here --, and
  * with the same entry point on that compact array in a second context: integers equal, floats inside the same allowance.
Where a per-frame debug view exists, the first and the last frame of every zone are checked against the twin one by one, so
that a failure names its zone.  A wrap of the atom-frame index in an unsigned (51.5 GB per slot) and the indices into work
buffers (B n_a 3 > 2^31 needs long lists) are out of scope."""
import ctypes
import time

import numpy as np
import pytest

import bigslot_cases as B
import pair_cases
import pair64
import vdos_cases
from conftest import rel_max
from engine_state import reset

pytestmark = pytest.mark.gpu


def _free_bytes():
    """free device memory as the HIP runtime reports it, or None where it cannot be asked"""
    try:
        free, total = ctypes.c_size_t(0), ctypes.c_size_t(0)
        if ctypes.CDLL("libamdhip64.so").hipMemGetInfo(ctypes.byref(free), ctypes.byref(total)) == 0:
            return int(free.value)
    except OSError:
        pass
    return None


@pytest.fixture(scope="module")
def big(engine):
    """both slots allocated and filled once; released, and the context reset, when the module is done"""
    from psa_amd import _hip
    reset(engine)
    engine.invalidate()
    need, free = 2 * (B.SLOT_BYTES + 1024), _free_bytes()
    if free is not None and free < need:
        pytest.fail(f"the device has {free} bytes free, the two slots need {need}")
    none, rows = np.zeros(0, np.float32), lambda n: np.zeros((0, n), np.float32)
    t0 = time.perf_counter()
    try:
        for slot, seed in ((_hip.SLOT_POSITIONS, B.SEED_POSITIONS), (_hip.SLOT_VELOCITIES, B.SEED_VELOCITIES)):
            try:
                engine.alloc(slot, B.T, B.N)
            except _hip.PsaHipError as e:
                pytest.fail(f"the device has {free} bytes free, the two slots need {need}: {e}")
            engine.fill_synthetic(slot, seed, none, np.zeros(0, np.int32), rows(B.T), rows(B.T), rows(B.N), rows(B.N))
        print(f"\nbig slots: 2 x {B.SLOT_BYTES / 1e9:.1f} GB allocated and filled in {time.perf_counter() - t0:.2f} s")
        yield engine
    finally:
        for slot in (_hip.SLOT_POSITIONS, _hip.SLOT_VELOCITIES):
            engine.release(slot)
        engine.invalidate()
        reset(engine)


@pytest.fixture(scope="module")
def small():
    """a second context for the compact copies"""
    from psa_amd import _hip
    eng = _hip.Engine(0)
    yield eng
    eng.close()


@pytest.fixture(autouse=True)
def _clean(big, small):
    reset(big)
    reset(small)
    yield
    reset(big)
    reset(small)


def _compact_resident(small, atoms, positions=True, velocities=False):
    from psa_amd import _hip
    out = []
    for wanted, slot, seed in ((positions, _hip.SLOT_POSITIONS, B.SEED_POSITIONS), (velocities, _hip.SLOT_VELOCITIES, B.SEED_VELOCITIES)):
        if wanted:
            out.append(B.compact(seed, atoms))
            small.ensure_resident(slot, out[-1])
    return out[0] if len(out) == 1 else out


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _fraction(err, bar):
    with np.errstate(divide="ignore", invalid="ignore"):
        f = np.where(err == 0, 0.0, err / bar)
    return float(np.max(np.where(np.isnan(f), np.inf, f)))


def _by_zone(err, bar, axis):
    """worst fraction of the bar per zone, `axis` the frame axis"""
    zones, bar = B.zone_of(np.arange(B.T)), np.broadcast_to(bar, err.shape)
    part = lambda x, z: np.compress(zones == z, x, axis=axis)             # noqa: E731
    return " ".join(f"Z{z} {_fraction(part(err, z), part(bar, z)):.3f}" for z in range(4))


# ---- everything else rests on this ----------------------------------------------------------------------------------
def test_fill_is_the_twin(big):
    from psa_amd import _hip
    t0 = time.perf_counter()
    everyone = np.arange(B.N)
    for name, slot, seed in (("positions", _hip.SLOT_POSITIONS, B.SEED_POSITIONS), ("velocities", _hip.SLOT_VELOCITIES, B.SEED_VELOCITIES)):
        assert big.shape(slot) == (B.T, B.N)
        for t in B.edge_frames():
            got, want = big.download(slot, t, 1), B.synthetic_atoms(seed, B.N, [t], everyone)
            assert np.array_equal(got, want), f"{name}: frame {t} (Z{B.zone_of([t])[0]}) is not the twin's"
    print(f"fill: 8 zone-edge frames of both slots are the twin's bits ({time.perf_counter() - t0:.2f} s)")


# ---- slot-wide ------------------------------------------------------------------------------------------------------
def test_mean_positions(big, small):
    """the listed atoms' rows bit for bit against the sequential float32 mean include/psa_hip.h promises"""
    from psa_amd import _hip
    atoms = B.MEAN["atoms"]
    t0 = time.perf_counter()
    got = big.mean_positions(_hip.SLOT_POSITIONS)
    took = time.perf_counter() - t0
    data = _compact_resident(small, atoms)
    want = B.mean32(data)
    assert got.shape == (B.N, 3) and _same_bits(got[atoms], want)
    assert _same_bits(small.mean_positions(_hip.SLOT_POSITIONS), want)
    print(f"mean_positions: {atoms.size} listed rows equal the float32 chain bit for bit, error / bound 0 / 0 ({took:.2f} s)")


# ---- the real-space self dynamics -----------------------------------------------------------------------------------
def test_displacement_moments_and_van_hove_self(big, small):
    c = B.MSD
    atoms, box = c["atoms"], B.BOXES["cubic"]
    groups = B.species(atoms, c["parts"])
    data = _compact_resident(small, atoms)
    inside = B.compact_groups(groups)
    ref, bar, counts, allowed, borderline, total = B.msd_reference(data)
    assert borderline <= 1e-3 * total

    # the unwrap pass with the positions taken as they are: u = r(t) - r(0) exactly, every frame of every zone
    t0 = time.perf_counter()
    u, img = big.debug_unwrap(box, atoms, unwrap=False)
    want = data.astype(np.float64) - data[:1].astype(np.float64)
    for t in B.edge_frames():
        assert np.array_equal(u[t], want[t]), f"debug_unwrap: frame {t} (Z{B.zone_of([t])[0]})"
    assert np.array_equal(u, want) and not img.any()
    print(f"debug_unwrap: {atoms.size} atoms x {B.T} frames equal r(t) - r(0), error / bound 0 / 0 ({time.perf_counter() - t0:.2f} s)")

    t0 = time.perf_counter()
    got = big.displacement_moments(box, c["n_lags"], groups, origin_step=c["step"], unwrap=False)
    took = time.perf_counter() - t0
    assert got.shape == ref.shape and got.dtype == np.float64 and np.all(np.abs(got - ref) <= bar)
    twin = small.displacement_moments(box, c["n_lags"], inside, origin_step=c["step"], unwrap=False)
    assert np.all(np.abs(twin - ref) <= bar)
    print(f"displacement_moments: groups {[g.size for g in groups]}, {c['n_lags']} lags, origin step {c['step']}: error / bar "
          f"{_fraction(np.abs(got - ref), bar):.3f}, compact copy {_fraction(np.abs(twin - ref), bar):.3f}, "
          f"same bits {_same_bits(got, twin)} ({took:.2f} s)")

    t0 = time.perf_counter()
    hist = big.van_hove_self(box, c["vh_lags"], c["dr"], c["n_r"], groups, origin_step=c["step"], unwrap=False)
    took = time.perf_counter() - t0
    assert hist.dtype == np.uint64 and hist.shape == counts.shape
    assert np.array_equal(hist.astype(np.int64).sum(axis=2), counts.sum(axis=2))                  # exact totals
    assert np.all(np.abs(hist.astype(np.int64) - counts) <= allowed)
    assert np.array_equal(hist, small.van_hove_self(box, c["vh_lags"], c["dr"], c["n_r"], inside, origin_step=c["step"], unwrap=False))
    print(f"van_hove_self: lags {c['vh_lags']}: {borderline} borderline of {total}, {int(np.abs(hist.astype(np.int64) - counts).sum())} "
          f"counts moved of {int(allowed.sum())} allowed; equal to the compact copy ({took:.2f} s)")


# ---- the pair distributions -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("box,parts", B.PAIR["layouts"])
def test_pair_histogram(big, small, box, parts):
    c = B.PAIR
    atoms, H = c["atoms"], B.BOXES[box]
    groups = B.species(atoms, parts)
    data = _compact_resident(small, atoms)
    inside = B.compact_groups(groups)
    ref, allowed, borderline, total = B.pair_reference(data, box, parts)
    assert borderline <= pair_cases.cap(c["n_r"]) * total                  # the borderline condition, before anything else

    # the fraction pass, frame by frame: the bound of tests/test_gpu_pair.py::test_fractions
    t0 = time.perf_counter()
    frac = big.debug_pair_fractions(H, atoms)
    want = pair64.fractions64(data, H)
    lim = 2.0 ** -26 + 4.0 * 2.0 ** -53 * (np.abs(data.astype(np.float64)) @ np.abs(pair64.box64(H)[1]))
    d = frac.astype(np.float64) - want
    d -= np.rint(d)
    for t in B.edge_frames():
        assert np.all(np.abs(d[t]) <= lim[t]), f"debug_pair_fractions: frame {t} (Z{B.zone_of([t])[0]})"
    assert frac.dtype == np.float32 and np.all(np.abs(frac) <= 0.5) and np.all(np.abs(d) <= lim)
    assert _same_bits(frac, small.debug_pair_fractions(H, np.arange(atoms.size, dtype=np.int32)))
    print(f"debug_pair_fractions {box}: error / bound per zone {_by_zone(np.abs(d), lim, 0)}; equal to the compact copy "
          f"({time.perf_counter() - t0:.2f} s)")

    t0 = time.perf_counter()
    got = big.pair_histogram(H, c["lags"], c["dr"], c["n_r"], groups, origin_step=c["step"])
    took = time.perf_counter() - t0
    assert got.dtype == np.uint64 and got.shape == ref.shape
    got64 = got.astype(np.int64)
    assert np.array_equal(got64.sum(axis=3), pair_cases.expected_totals(B.T, inside, c["lags"], c["step"]))
    assert np.all(np.abs(got64 - ref) <= allowed)
    assert np.array_equal(got, small.pair_histogram(H, c["lags"], c["dr"], c["n_r"], inside, origin_step=c["step"]))
    print(f"pair_histogram {box}: species {[g.size for g in groups]}, lags {c['lags']}, origin step {c['step']}: {borderline} borderline "
          f"of {total}, {int(np.abs(got64 - ref).sum())} counts moved of {int(allowed.sum())} allowed; equal to the compact copy ({took:.2f} s)")


# ---- the density of states ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["whole", "z3", "spanning"])
def test_vdos(big, small, layout):
    from psa_amd import _hip
    c = B.VDOS
    atoms = c["atoms"]
    groups = B.species(atoms, c["parts"])
    lay = B.segment_layouts()[layout]
    full, listed = B.listed_weights(atoms, 6)
    data = _compact_resident(small, atoms, positions=False, velocities=True)
    ref, bound = B.vdos_reference(data, lay, listed)
    t0 = time.perf_counter()
    big.set_atom_weights(full)
    big.set_segments(lay)
    got = big.vdos(_hip.SLOT_VELOCITIES, None, groups, 0)
    took = time.perf_counter() - t0
    small.set_atom_weights(listed)
    small.set_segments(lay)
    twin = small.vdos(_hip.SLOT_VELOCITIES, None, B.compact_groups(groups), 0)
    r, at = vdos_cases.ratio(got, ref, bound)
    r2, _ = vdos_cases.ratio(twin, ref, bound)
    print(f"vdos {layout}: groups {[g.size for g in groups]} -> {got.shape}: {r:.3f} x bound at {at}, rel_max {rel_max(got, ref):.2e}; "
          f"compact copy {r2:.3f} x bound, same bits {_same_bits(got, twin)} ({took:.2f} s)")
    assert got.dtype == np.float32 and np.all(np.isfinite(got)) and r <= 1.0 and r2 <= 1.0


# ---- the dynamic structure factor -----------------------------------------------------------------------------------
def test_dynamic_projection_and_spectra(big, small):
    c = B.DYNAMIC
    atoms, k = c["atoms"], B.dynamic_k()
    full, listed = B.listed_weights(atoms, 7)
    pos, vel = _compact_resident(small, atoms, velocities=True)
    everyone = np.arange(atoms.size, dtype=np.int32)
    ref, bound = B.dynamic_reference(pos, vel, listed)
    big.set_atom_weights(full)
    small.set_atom_weights(listed)

    t0 = time.perf_counter()
    got = big.debug_dynamic_project(k, atoms, True)
    took = time.perf_counter() - t0
    assert got.shape == ref.shape == (len(k), 4, B.T)
    err = np.abs(got.astype(np.complex128) - ref)
    for t in B.edge_frames():
        assert np.all(err[:, :, t] <= bound[None, :, t]), f"debug_dynamic_project: frame {t} (Z{B.zone_of([t])[0]})"
    twin = small.debug_dynamic_project(k, everyone, True)
    print(f"debug_dynamic_project: {atoms.size} atoms, {len(k)} k-vectors: error / bound per zone {_by_zone(err, bound[None], 2)}; "
          f"compact copy {_fraction(np.abs(twin.astype(np.complex128) - ref), bound[None]):.3f}, same bits {_same_bits(got, twin)} ({took:.2f} s)")
    assert np.all(err <= bound[None]) and np.all(np.abs(twin.astype(np.complex128) - ref) <= bound[None])

    lay = B.segment_layouts()["spanning"]
    want = B.dynamic_spectra_reference(pos, vel, listed, lay)
    big.set_segments(lay)
    small.set_segments(lay)
    t0 = time.perf_counter()
    one = big.dynamic_spectra(k, atoms, True)
    took = time.perf_counter() - t0
    two = small.dynamic_spectra(k, everyone, True)
    worst = max(rel_max(one[i], want[i]) for i in range(3))
    worst2 = max(rel_max(two[i], want[i]) for i in range(3))
    print(f"dynamic_spectra: Hann segments of {lay.length} at hop {lay.hop}: rel_max / bar {worst / B.DYNAMIC_SPECTRA_BAR:.3f}, compact "
          f"copy {worst2 / B.DYNAMIC_SPECTRA_BAR:.3f}, same bits {_same_bits(one, two)} ({took:.2f} s)")
    assert worst <= B.DYNAMIC_SPECTRA_BAR and worst2 <= B.DYNAMIC_SPECTRA_BAR


# ---- the spectra on the box's reciprocal lattice --------------------------------------------------------------------
def test_lattice_and_partial_spectra(big, small):
    c = B.LATTICE
    atoms, ind, inv = c["atoms"], c["indices"], B.box_inverse(c)
    groups = B.species(atoms, c["parts"])
    inside = [g.astype(np.int32) for g in B.compact_groups(groups)]
    full, listed = B.listed_weights(atoms, 8)
    pos, vel = _compact_resident(small, atoms, velocities=True)
    everyone = np.arange(atoms.size, dtype=np.int32)
    ref, bound = B.lattice_reference(pos, vel, listed)
    big.set_atom_weights(full)
    small.set_atom_weights(listed)

    t0 = time.perf_counter()
    got = big.debug_lattice_project(inv, ind, atoms, True)
    took = time.perf_counter() - t0
    assert got.shape == ref.shape == (len(ind), 4, B.T)
    err = np.abs(got.astype(np.complex128) - ref)
    for t in B.edge_frames():
        assert np.all(err[:, :, t] <= bound[None, :, t]), f"debug_lattice_project: frame {t} (Z{B.zone_of([t])[0]})"
    twin = small.debug_lattice_project(inv, ind, everyone, True)
    print(f"debug_lattice_project: {atoms.size} atoms, {len(ind)} vectors: error / bound per zone {_by_zone(err, bound[None], 2)}; "
          f"compact copy {_fraction(np.abs(twin.astype(np.complex128) - ref), bound[None]):.3f}, same bits {_same_bits(got, twin)} ({took:.2f} s)")
    assert np.all(err <= bound[None]) and np.all(np.abs(twin.astype(np.complex128) - ref) <= bound[None])

    # the species form is the lattice kernel per species, bit for bit (tests/test_gpu_partial.py), in every frame
    t0 = time.perf_counter()
    per = big.debug_partial_project(inv, ind, groups, True)
    for a, g in enumerate(groups):
        want = big.debug_lattice_project(inv, ind, g, True)
        for t in B.edge_frames():
            assert _same_bits(np.ascontiguousarray(per[:, a, :, t]), np.ascontiguousarray(want[:, :, t])), \
                f"debug_partial_project: species {a}, frame {t} (Z{B.zone_of([t])[0]})"
        assert _same_bits(np.ascontiguousarray(per[:, a]), want)
    assert _same_bits(per, small.debug_partial_project(inv, ind, inside, True))
    print(f"debug_partial_project: species {[g.size for g in groups]} equal the lattice kernel's bits and the compact copy's, error / "
          f"bound 0 / 0 ({time.perf_counter() - t0:.2f} s)")

    lay = B.segment_layouts()["spanning"]
    big.set_segments(lay)
    small.set_segments(lay)
    want = B.lattice_spectra_reference(ref, lay)
    t0 = time.perf_counter()
    one = big.lattice_spectra(inv, ind, None, 0, atoms, True)
    took = time.perf_counter() - t0
    two = small.lattice_spectra(inv, ind, None, 0, everyone, True)
    worst, worst2 = (max(rel_max(x[i], want[i]) for i in range(3)) for x in (one, two))
    print(f"lattice_spectra: Hann segments of {lay.length} at hop {lay.hop}: rel_max / bar {worst / B.SPECTRA_BAR:.3f}, compact copy "
          f"{worst2 / B.SPECTRA_BAR:.3f}, same bits {_same_bits(one, two)} ({took:.2f} s)")
    assert worst <= B.SPECTRA_BAR and worst2 <= B.SPECTRA_BAR

    want = B.partial_spectra_reference(pos, vel, listed, lay)
    t0 = time.perf_counter()
    one = big.partial_spectra(inv, ind, groups, None, 0, True)
    took = time.perf_counter() - t0
    two = small.partial_spectra(inv, ind, inside, None, 0, True)
    worst, worst2 = (max(B.pair_errors(x[i], want[i]) for i in range(3)) for x in (one, two))
    print(f"partial_spectra: species {[g.size for g in groups]}: pair error / bar {worst / B.SPECTRA_BAR:.3f}, compact copy "
          f"{worst2 / B.SPECTRA_BAR:.3f}, same bits {_same_bits(one, two)} ({took:.2f} s)")
    assert worst <= B.SPECTRA_BAR and worst2 <= B.SPECTRA_BAR

    box, n_lags = B.correlation_layout(), B.CORRELATION["n_lags"]
    big.set_segments(box)
    small.set_segments(box)
    want = B.lattice_correlations_reference(ref)
    t0 = time.perf_counter()
    one = big.lattice_correlations(inv, ind, n_lags, None, 0, atoms, True)
    took = time.perf_counter() - t0
    two = small.lattice_correlations(inv, ind, n_lags, None, 0, everyone, True)
    worst, worst2 = (max(B.correlation_fraction(x[i], want[i]) for i in range(3)) for x in (one, two))
    print(f"lattice_correlations: boxcar segments of {box.length} at hop {box.hop}, {n_lags} lags: error / bar {worst:.3f}, compact copy "
          f"{worst2:.3f}, same bits {_same_bits(one, two)} ({took:.2f} s)")
    assert one.dtype == np.float32 and worst <= 1.0 and worst2 <= 1.0


def test_self_spectra(big, small):
    c = B.SELF
    atoms, ind, inv = c["atoms"], c["indices"], B.box_inverse(c)
    full, listed = B.listed_weights(atoms, 9)
    pos = _compact_resident(small, atoms)
    everyone = np.arange(atoms.size, dtype=np.int32)
    ref, bound = B.self_reference(pos, listed)
    big.set_atom_weights(full)
    small.set_atom_weights(listed)

    t0 = time.perf_counter()
    got = big.debug_self_series(inv, ind, atoms)
    took = time.perf_counter() - t0
    assert got.shape == ref.shape == (atoms.size, len(ind), B.T) and got.dtype == np.complex64
    err = np.abs(got.astype(np.complex128) - ref)
    for t in B.edge_frames():
        assert np.all(err[:, :, t] <= bound[:, :, 0]), f"debug_self_series: frame {t} (Z{B.zone_of([t])[0]})"
    twin = small.debug_self_series(inv, ind, everyone)
    print(f"debug_self_series: {atoms.size} atoms, {len(ind)} vectors: error / bound per zone {_by_zone(err, bound, 2)}; same bits as the "
          f"compact copy {_same_bits(got, twin)} ({took:.2f} s)")
    assert np.all(err <= bound) and np.all(np.abs(twin.astype(np.complex128) - ref) <= bound)

    lay = B.segment_layouts()["spanning"]
    big.set_segments(lay)
    small.set_segments(lay)
    want = B.self_spectra_reference(pos, listed, lay)
    t0 = time.perf_counter()
    one = big.self_spectra(inv, ind, None, 0, atoms)
    took = time.perf_counter() - t0
    two = small.self_spectra(inv, ind, None, 0, everyone)
    worst, worst2 = B.column_rel_max(one, want), B.column_rel_max(two, want)
    print(f"self_spectra: Hann segments of {lay.length} at hop {lay.hop}: rel_max per column / bar {worst / B.SPECTRA_BAR:.3f}, compact copy "
          f"{worst2 / B.SPECTRA_BAR:.3f}, same bits {_same_bits(one, two)} ({took:.2f} s)")
    assert worst <= B.SPECTRA_BAR and worst2 <= B.SPECTRA_BAR

    box, n_lags = B.correlation_layout(), B.CORRELATION["n_lags"]
    big.set_segments(box)
    small.set_segments(box)
    want = B.self_correlations_reference(pos, listed)
    t0 = time.perf_counter()
    one = big.self_correlations(inv, ind, n_lags, None, 0, atoms)
    took = time.perf_counter() - t0
    two = small.self_correlations(inv, ind, n_lags, None, 0, everyone)
    worst, worst2 = B.correlation_fraction(one, want), B.correlation_fraction(two, want)
    print(f"self_correlations: boxcar segments of {box.length} at hop {box.hop}, {n_lags} lags: error / bar {worst:.3f}, compact copy "
          f"{worst2:.3f}, same bits {_same_bits(one, two)} ({took:.2f} s)")
    assert one.dtype == np.float32 and worst <= 1.0 and worst2 <= 1.0


# ---- the SED projection on an index-list group ----------------------------------------------------------------------
def _select(engine, form, K):
    from test_gpu_dense_envelope import _select as select
    select(engine, form, K)


@pytest.mark.parametrize("form,K,planes", B.SED["forms"], ids=[f"{f}_K{K}" for f, K, _ in B.SED["forms"]])
def test_sed_projection(big, small, form, K, planes):
    """Engine.debug_project_only, the per-frame view of Engine.calculate: every dense kernel's gather form on the fly, then
    the list's split planes, per element in units of B inside the form's bound (tests/dense_cases.py)"""
    import dense_cases
    from psa_amd import _hip
    from ref64 import gamma
    atoms = B.SED["atoms"]
    r_all, r, k = B.sed_inputs()
    k = k[:K]
    full, listed = B.listed_weights(atoms, 10)
    vel = _compact_resident(small, atoms, positions=False, velocities=True)
    ref, scale = B.sed_reference(vel, r, k, listed)
    bound = dense_cases.bound(form, atoms.size)
    for eng, w in ((big, full), (small, listed)):
        _select(eng, form, K)
        eng.set_atom_weights(w)
    t0 = time.perf_counter()
    got = big.debug_project_only(_hip.SLOT_VELOCITIES, r_all, k, atoms, 0)
    took = time.perf_counter() - t0
    sets = big.plane_cache()[0]
    assert (sets > 0) == planes, f"{form}: {sets} plane sets cached"
    zones = B.zone_of(np.arange(B.T))
    for t in B.edge_frames():
        assert gamma(got[:, :, t:t + 1], ref[:, :, t:t + 1], scale[:, t:t + 1]) <= bound, f"{form}: frame {t} (Z{zones[t]})"
    per_zone = " ".join(f"Z{z} {gamma(got[:, :, zones == z], ref[:, :, zones == z], scale[:, zones == z]) / bound:.3f}" for z in range(4))
    twin = small.debug_project_only(_hip.SLOT_VELOCITIES, r, k, np.arange(atoms.size, dtype=np.int32), 0)
    g, g2 = gamma(got, ref, scale), gamma(twin, ref, scale)
    print(f"debug_project_only {form}: K={K} n_g={atoms.size} (a repeated atom), {sets} plane sets: gamma / bound per zone {per_zone}; "
          f"compact copy {g2 / bound:.3f}, same bits {_same_bits(got, twin)} ({took:.2f} s)")
    assert np.all(np.isfinite(got)) and g <= bound and g2 <= bound


@pytest.mark.parametrize("planes", [False, True], ids=["gather", "planes"])
def test_calculate_and_single_bin(big, small, planes):
    """Engine.calculate (incoherent, two index-list groups) and Engine.single_bin on the list, on the gather kernels and with
    the lists' split planes built, against float64 inside the bars of tests/test_gpu_dense_envelope.py and
    tests/test_gpu_spectral.py"""
    import spectral_cases
    from psa_amd import _hip
    from ref64 import intensity64, row_rel
    atoms = B.SED["atoms"]
    r_all, r, k = B.sed_inputs()
    full, listed = B.listed_weights(atoms, 10)
    groups = B.species(atoms, B.SED["parts"])
    inside = [g.astype(np.int32) for g in B.compact_groups(groups)]
    vel = _compact_resident(small, atoms, positions=False, velocities=True)
    for eng, w in ((big, full), (small, listed)):
        _select(eng, "planes128" if planes else "pair", len(k))
        eng.set_atom_weights(w)
    want = intensity64(vel, r, k, inside, listed)
    t0 = time.perf_counter()
    got = big.calculate(_hip.SLOT_VELOCITIES, r_all, k, groups, _hip.F_INTENSITY)
    took = time.perf_counter() - t0
    assert (big.plane_cache()[0] > 0) == planes
    twin = small.calculate(_hip.SLOT_VELOCITIES, r, k, inside, _hip.F_INTENSITY)
    err, rows = rel_max(got, want), float(row_rel(got, want).max())
    err2, rows2 = rel_max(twin, want), float(row_rel(twin, want).max())
    print(f"calculate {'planes' if planes else 'gather'}: groups {[g.size for g in groups]}, K={len(k)}: rel_max / bar {err / B.E2E_TOL:.3f}, "
          f"worst row / bar {rows / B.E2E_TOL_ROW:.3f}; compact copy {err2 / B.E2E_TOL:.3f}, {rows2 / B.E2E_TOL_ROW:.3f}, same bits "
          f"{_same_bits(got, twin)} ({took:.2f} s)")
    assert np.all(np.isfinite(got)) and err <= B.E2E_TOL and rows <= B.E2E_TOL_ROW and err2 <= B.E2E_TOL and rows2 <= B.E2E_TOL_ROW

    # one bin of one k-vector: the form is the one a one-vector list takes, with planes where the call built them
    ref, scale = B.sed_reference(vel, r, k[:1], listed)
    everyone = np.arange(atoms.size, dtype=np.int32)
    for eng in (big, small):
        _select(eng, "planes32" if planes else "bf16x3", 1)
    worst = worst2 = 0.0
    t0 = time.perf_counter()
    before, built = big.plane_cache()[0], None
    for b in B.SED["bins"]:
        one = big.single_bin(_hip.SLOT_VELOCITIES, r_all, k[0], atoms, b)
        if built is None:                                                  # the first call builds the list's planes, or none does
            built = big.plane_cache()[0] > before
        assert planes or big.plane_cache()[0] == 0
        two = small.single_bin(_hip.SLOT_VELOCITIES, r, k[0], everyone, b)
        dft = spectral_cases.single_bin_ref64(ref[0], b)
        bar = spectral_cases.single_bin_bar("planes32" if built else "bf16x3", atoms.size, scale, dft)
        e1, e2 = (np.maximum(np.abs(x.real.astype(np.float64) - dft.real), np.abs(x.imag.astype(np.float64) - dft.imag)) for x in (one, two))
        worst, worst2 = max(worst, float(np.max(e1 / bar))), max(worst2, float(np.max(e2 / bar)))
        assert np.all(e1 <= bar) and np.all(e2 <= bar), f"single_bin: bin {b}"
    print(f"single_bin {'planes' if planes else 'gather'}: bins {B.SED['bins']}, planes used {built}: error / bar {worst:.3f}, compact copy "
          f"{worst2:.3f} ({time.perf_counter() - t0:.2f} s)")

# ---- the neighbour-shell passes: their one read of the slot is the fraction pass (test_pair_histogram's per-frame view) -----
def test_angle_histogram(big, small):
    import angle_cases
    import angle64
    c = B.ANGLE
    atoms, H, rc, n_theta, step = c["atoms"], B.BOXES[c["box"]], c["r_cut"], c["n_theta"], c["step"]
    groups = B.species(atoms, c["parts"])
    inside = [g.astype(np.int32) for g in B.compact_groups(groups)]
    data = _compact_resident(small, atoms)
    ref = B.angle_reference(data)
    assert ref["borderline"] <= angle_cases.cap(n_theta) * max(ref["triplets"], 1)     # the borderline condition, before anything else

    # the neighbour lists of the zone-edge frames: every sure neighbour there, nothing but sure and leg-borderline ones
    t0 = time.perf_counter()
    edge = B.angle_reference(data, frames=B.edge_frames())
    for j, f in enumerate(B.edge_frames()):
        count, lst = big.debug_neighbour_lists(H, rc, f, groups)
        count2, lst2 = small.debug_neighbour_lists(H, rc, f, inside)
        assert np.array_equal(count, count2) and np.array_equal(lst, lst2), f"debug_neighbour_lists: frame {f} (Z{B.zone_of([f])[0]})"
        for a, (sure, maybe) in enumerate(edge["lists"][j]):
            mine = lst[a, :min(count[a], 64)]
            assert np.all(np.diff(mine) > 0) and np.all(lst[a, count[a]:] == -1)
            assert np.all(np.isin(sure, mine)) and np.all(np.isin(mine, np.concatenate([sure, maybe]))), \
                f"debug_neighbour_lists: frame {f} (Z{B.zone_of([f])[0]}), centre {a}"
    print(f"debug_neighbour_lists: 8 zone-edge frames, {atoms.size} centres each, the reference's lists and the compact copy's "
          f"({time.perf_counter() - t0:.2f} s)")

    t0 = time.perf_counter()
    got = big.angle_histogram(H, rc, n_theta, groups, origin_step=step)
    took = time.perf_counter() - t0
    assert all(g.dtype == np.uint64 for g in got)
    assert angle_cases.check(got, ref, f"angle_histogram: species {[g.size for g in groups]}, origin step {step}")
    assert angle_cases.identities(got, [g.size for g in groups], angle64.n_origins(B.T, step))
    twin = small.angle_histogram(H, rc, n_theta, inside, origin_step=step)
    assert all(np.array_equal(a, b) for a, b in zip(got, twin))
    moved, allowed = int(np.abs(got[0].astype(np.int64) - ref["angles"]).sum()), int(ref["angles_allowed"].sum())
    print(f"angle_histogram: {moved} angle counts moved of {allowed} allowed; equal to the compact copy ({took:.2f} s)")


# ---- the mode-projected SED, its Welch average and the spectral covariance ------------------------------------------
def test_modes_welch_modes_and_covariance(big, small):
    from psa_amd import _hip
    c = B.MODES
    atoms = c["atoms"]
    groups = B.species(atoms, c["parts"])
    inside = [g.astype(np.int32) for g in B.compact_groups(groups)]
    r_all, r, k, eig, g = B.modes_inputs()
    full, listed = B.listed_weights(atoms, 11)
    vel = _compact_resident(small, atoms, positions=False, velocities=True)
    lay = B.segment_layouts()["spanning"]
    phi, welch, cov = B.modes_references(vel, listed, lay)
    big.set_atom_weights(full)
    small.set_atom_weights(listed)
    slot = _hip.SLOT_VELOCITIES

    t0 = time.perf_counter()
    one = big.sed_modes(slot, r_all, k, groups, eig)
    took = time.perf_counter() - t0
    two = small.sed_modes(slot, r, k, inside, eig)
    e1, e2 = rel_max(one, phi), rel_max(two, phi)
    print(f"sed_modes: sites {[x.size for x in groups]}, K={len(k)}, M={eig.shape[1]}: rel_max / bar {e1 / B.MODES_BAR:.3f}, compact copy "
          f"{e2 / B.MODES_BAR:.3f}, same bits {_same_bits(one, two)} ({took:.2f} s)")
    assert one.shape == phi.shape and e1 <= B.MODES_BAR and e2 <= B.MODES_BAR

    t0 = time.perf_counter()
    one = big.sed_covariance(slot, r_all, k, groups, g)
    took = time.perf_counter() - t0
    two = small.sed_covariance(slot, r, k, inside, g)
    e1, e2 = B.matrix_rel_max(one, cov), B.matrix_rel_max(two, cov)
    print(f"sed_covariance: moments -2 and 0: worst k-point matrix rel_max / bar {e1 / B.MODES_BAR:.3f}, compact copy {e2 / B.MODES_BAR:.3f}, "
          f"same bits {_same_bits(one, two)} ({took:.2f} s)")
    assert one.shape == cov.shape and e1 <= B.MODES_BAR and e2 <= B.MODES_BAR

    big.set_segments(lay)
    small.set_segments(lay)
    t0 = time.perf_counter()
    one = big.sed_modes_welch(slot, r_all, k, groups, eig)
    took = time.perf_counter() - t0
    two = small.sed_modes_welch(slot, r, k, inside, eig)
    e1, e2 = rel_max(one, welch), rel_max(two, welch)
    print(f"sed_modes_welch: Hann segments of {lay.length} at hop {lay.hop}: rel_max / bar {e1 / B.MODES_BAR:.3f}, compact copy "
          f"{e2 / B.MODES_BAR:.3f}, same bits {_same_bits(one, two)} ({took:.2f} s)")
    assert one.shape == welch.shape and e1 <= B.MODES_BAR and e2 <= B.MODES_BAR


def test_bond_order(big, small):
    """per-atom n^2 q_l^2 and neighbour counts held to the reference as tests/test_gpu_order.py holds them, the histogram to the
    integer bin rule, everything equal to the compact copy"""
    import angle64
    import order_cases
    c = B.ORDER
    atoms, H, rc, ls, n_q, step = c["atoms"], B.BOXES[c["box"]], c["r_cut"], c["ls"], c["n_q"], c["step"]
    groups = B.species(atoms, c["parts"])
    inside = [g.astype(np.int32) for g in B.compact_groups(groups)]
    data = _compact_resident(small, atoms)
    ref = B.order_reference(data)
    assert order_cases.excluded_share(ref) <= order_cases.EXCLUDED_CAP          # the excluded share, before anything else
    t0 = time.perf_counter()
    got = big.bond_order(H, rc, ls, n_q, groups, origin_step=step, per_atom=True)
    took = time.perf_counter() - t0
    hist, trunc, iso, undef, x, n = got
    n_o, sizes = angle64.n_origins(B.T, step), [g.size for g in groups]
    assert x.shape == (n_o, atoms.size, len(ls)) and n.shape == (n_o, atoms.size)
    assert order_cases.check(x, n, ref, f"bond_order: species {sizes}, orders {ls}, origin step {step}")
    want, out = order_cases.histogram_of(x, n, sizes, n_q)
    assert np.array_equal(hist.astype(np.int64), want) and np.array_equal((trunc + iso + undef).astype(np.int64), out)
    twin = small.bond_order(H, rc, ls, n_q, inside, origin_step=step, per_atom=True)
    assert all(np.array_equal(a, b) for a, b in zip(got, twin))
    print(f"bond_order: histogram by the integer bin rule, all six outputs equal to the compact copy ({took:.2f} s)")


def test_local_order(big, small):
    """held as tests/test_gpu_local_order.py holds it: per-atom values inside qlm_cases' allowances, the bin rules exactly, Q of
    the zone-edge frames by debug_qlm; every output equal to the compact copy's"""
    import angle64
    import qlm_cases
    from psa_amd import local_order
    c = B.LOCAL
    atoms, H, rc, ls, step = c["atoms"], B.BOXES[c["box"]], c["r_cut"], c["ls"], c["step"]
    n_q, n_w, w_range, thr = c["n_q"], c["n_w"], c["w_range"], c["threshold"]
    groups = B.species(atoms, c["parts"])
    inside = [g.astype(np.int32) for g in B.compact_groups(groups)]
    data = _compact_resident(small, atoms)
    ref = B.local_reference(data)
    assert qlm_cases.excluded_share(ref) <= qlm_cases.EXCLUDED_CAP and qlm_cases.loose_share(ref) <= qlm_cases.EXCLUDED_CAP
    names = ("hist", "qbar2", "w", "wbar", "xi", "n")
    table = local_order.w3j_blocks(ls)

    t0 = time.perf_counter()
    edge = B.local_reference(data, frames=B.edge_frames())
    for j, f in enumerate(B.edge_frames()):
        q = big.debug_qlm(H, rc, f, ls, groups)
        assert q.dtype == np.int64 and qlm_cases.check_q(q, edge, j, f"debug_qlm frame {f} (Z{B.zone_of([f])[0]})")
        assert np.array_equal(q, small.debug_qlm(H, rc, f, ls, inside)), f"debug_qlm: frame {f} (Z{B.zone_of([f])[0]})"
    print(f"debug_qlm: 8 zone-edge frames inside the allowance and equal to the compact copy ({time.perf_counter() - t0:.2f} s)")

    t0 = time.perf_counter()
    raw = big.local_order(H, rc, ls, n_q, n_w, table, groups, step, w_range, ls[-1], thr, True)
    took = time.perf_counter() - t0
    got = dict(zip(names, raw))
    sizes, n_l, n_o = [g.size for g in groups], len(ls), angle64.n_origins(B.T, step)
    assert qlm_cases.check(got, ref, f"local_order: species {sizes}, orders {ls}, origin step {step}")
    assert np.array_equal(qlm_cases.fold_left_out(got["hist"], n_l, n_q, n_w), qlm_cases.rows_of(got, sizes, n_l, n_q, n_w, w_range))
    assert qlm_cases.identities(got["hist"], sizes, n_o, n_l, n_q, n_w)
    twin = small.local_order(H, rc, ls, n_q, n_w, table, inside, step, w_range, ls[-1], thr, True)
    assert all(np.array_equal(a, b, equal_nan=a.dtype.kind == "f") for a, b in zip(raw, twin))
    print(f"local_order: the bin rules exactly, all six outputs equal to the compact copy ({took:.2f} s)")


@pytest.mark.parametrize("link", B.CLUSTER["links"])
def test_solid_clusters(big, small, link):
    """equal to the cluster twin (tests/cluster_cases.py) in every key, as tests/test_gpu_cluster.py asks, and to the compact copy"""
    import cluster_cases
    c = B.CLUSTER
    atoms, H = c["atoms"], B.BOXES[c["box"]]
    groups = B.species(atoms, c["parts"])
    inside = [g.astype(np.int32) for g in B.compact_groups(groups)]
    data = _compact_resident(small, atoms)
    want = B.cluster_twin(data, link)
    args = (H, c["r_cut"], c["solid_l"], c["threshold"], c["min_connections"], link, c["n_sizes"])
    t0 = time.perf_counter()
    got = big.solid_clusters(*args, groups, c["step"], True)
    took = time.perf_counter() - t0
    assert cluster_cases.differs(got, want, B.CLUSTER_KEYS) == []
    assert np.array_equal(cluster_cases.fold_left_out(got["species_rows"]), want["species_rows"]) and cluster_cases.identities(got)
    twin = small.solid_clusters(*args, inside, c["step"], True)
    assert cluster_cases.differs(got, twin, B.CLUSTER_KEYS + ("species_rows",)) == []
    print(f"solid_clusters link {link}: {int(np.asarray(got['n_solid']).sum())} solid atoms in {int(np.asarray(got['n_clusters']).sum())} "
          f"clusters over {len(got['labels'])} origins: every key equal to the twin and to the compact copy ({took:.2f} s)")
