"""Host side of the index-width tests (tests/bigslot_cases.py; the GPU side is tests/test_gpu_bigslot.py): the twin of
the generator for chosen atoms, the zone limits, the borderline conditions of the chosen cases, and the sensitivity
proof -- for every reference the GPU test compares with and every zone past a 32-bit limit, the reference of data read
through a wrapped index lies outside the allowance the GPU test applies to the clean data.  So a kernel that forms a slot
address in 32 bits in any zone cannot pass."""
import numpy as np
import pytest

import bigslot_cases as B
import pair_cases
from conftest import rel_max
from psa_amd import synth


# ---- the twin and the zones -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("cells,n_frames,seed", [((2, 1, 1), 7, 0), ((3, 2, 1), 5, 77), ((2, 2, 2), 3, B.SEED_POSITIONS)])
def test_twin_is_velocities_block(cells, n_frames, seed):
    spec = synth.SyntheticSpec(cells, n_frames, seed=seed)
    r0, _, _ = synth.lattice(cells)
    whole = synth.velocities_block(spec, synth.mode_tables(spec, r0), 0, n_frames)
    n = spec.n_atoms
    assert np.array_equal(B.synthetic_atoms(seed, n, np.arange(n_frames), np.arange(n)), whole)
    frames, atoms = np.array([n_frames - 1, 0, 2]), np.array([n - 1, 3, 0, 3])
    assert np.array_equal(B.synthetic_atoms(seed, n, frames, atoms), whole[frames][:, atoms])


def test_zone_limits():
    N, T = B.N, B.T
    assert N % 2 == 1 and N % 4 != 0 and T == 2 ** 8 * 3 ** 2
    assert T * N > 2 ** 31 and 3 * T * N > 2 ** 32 and T * N < 2 ** 32
    assert B.zone_starts() == (0, 683, 1366, 2048)
    assert B.edge_frames() == [0, 682, 683, 1365, 1366, 2047, 2048, 2303]
    z1, z2, z3 = B.zone_starts()[1:]
    assert 3 * (z1 - 1) * N < 2 ** 31 <= 3 * z1 * N                        # the first element of the row
    assert 3 * (z2 - 1) * N < 2 ** 32 <= 3 * z2 * N
    assert (z3 - 1) * N < 2 ** 31 <= z3 * N
    assert list(B.zone_of([0, 682, 683, 1365, 1366, 2047, 2048, 2303])) == [0, 0, 1, 1, 2, 2, 3, 3]
    # the last element of the array is where every width has wrapped
    last = int(B.element_index(N, [T - 1], [N - 1])[0, 0, 2])
    assert last == 3 * T * N - 1 and last > 2 ** 32


def test_origins_lags_and_segments_reach_every_zone():
    origins = np.arange(0, B.T, B.ORIGIN_STEP)
    assert set(B.zone_of(origins)) == {0, 1, 2, 3}
    assert list(B.zone_of(np.arange(0, B.T, B.SPARSE_STEP))) == [0, 1, 2, 3]
    far = origins[origins + B.LAG_FAR <= B.T - 1]
    assert list(B.zone_of(far)) == [0] and list(B.zone_of(far + B.LAG_FAR)) == [3]
    lay = B.segment_layouts()
    support = np.nonzero(lay["z3"].window_array())[0]
    assert support.size and set(B.zone_of(support)) == {3}
    sp = lay["spanning"]
    starts = np.arange(0, B.T - sp.length + 1, sp.hop)
    assert set(B.zone_of(starts)) == {0, 1, 2, 3} and set(B.zone_of(starts + sp.length - 1)) == {0, 1, 2, 3}


@pytest.mark.parametrize("case", [B.MSD, B.PAIR, B.VDOS, B.DYNAMIC, B.MEAN], ids=["msd", "pair", "vdos", "dynamic", "mean"])
def test_atom_lists(case):
    a = case["atoms"]
    assert 100 <= a.size <= 600 and np.unique(a).size == a.size and a.min() == 0
    assert set(range(B.N - 10, B.N)) <= set(a.tolist())
    assert np.any(np.diff(a) < 0)                                          # unsorted
    assert np.all(np.bincount(a // (B.N // 8 + 1), minlength=8) > 0)       # members in every eighth of the range
    d = B.with_duplicate(a)
    assert d.size == a.size + 1 and np.unique(d).size == a.size


def test_fault_changes_its_zone_alone():
    atoms = B.MEAN["atoms"]
    clean = B.compact(B.SEED_POSITIONS, atoms)
    assert np.abs(clean).max() < 3.5 and abs(float(clean.std()) - 1.0) < 0.01
    for zone, kinds in B.FAULTS.items():
        for kind in kinds:
            bad = B.fault(clean, zone, kind, B.SEED_POSITIONS, atoms)
            moved = np.nonzero(np.any(bad != clean, axis=(1, 2)))[0]
            assert set(B.zone_of(moved)) == {zone} and moved.size >= 0.99 * B.zone_frames(zone).size
    # below 2^32 an unsigned index has not wrapped: nothing to plant in Z1 but in its last row, which crosses 2^32 on its
    # way (the zones go by the first element of a row)
    moved = np.nonzero(np.any(B.fault(clean, 1, "u32", B.SEED_POSITIONS, atoms) != clean, axis=(1, 2)))[0]
    assert list(moved) == [B.zone_starts()[2] - 1]


# ---- the borderline conditions: met by the references alone ----------------------------------------------------------
def test_displacement_case_conditions():
    _, bar, counts, allowed, borderline, total = B.msd_reference(B.compact(B.SEED_POSITIONS, B.MSD["atoms"]))
    assert borderline <= 1e-3 * total                                     # as tests/test_gpu_msd.py asks of its histogram
    assert counts[..., :B.MSD["n_r"]].sum() > 0.9 * counts[1:].sum() and np.all(bar[1:] > 0)
    print(f"van Hove: {borderline} borderline of {total}")


@pytest.mark.parametrize("box,parts", B.PAIR["layouts"])
def test_pair_case_conditions(box, parts):
    from psa_amd import max_pair_radius
    assert B.PAIR["dr"] * B.PAIR["n_r"] <= max_pair_radius(B.BOXES[box])
    _, _, borderline, total = B.pair_reference(B.compact(B.SEED_POSITIONS, B.PAIR["atoms"]), box, parts)
    print(f"pairs {box}: {borderline} borderline of {total} (cap {pair_cases.cap(B.PAIR['n_r']) * total:.0f})")
    assert borderline <= pair_cases.cap(B.PAIR["n_r"]) * total


# ---- sensitivity ----------------------------------------------------------------------------------------------------
def _faulted(seed, atoms):
    clean = B.compact(seed, atoms)
    for zone, kinds in B.FAULTS.items():
        for kind in kinds:
            yield zone, kind, B.fault(clean, zone, kind, seed, atoms)


def _report(entry, ratios):
    """ratios: {(zone, kind): largest error over its allowance}; every one must exceed 1"""
    worst = min(ratios, key=ratios.get)
    print(f"{entry}: smallest error / allowance {ratios[worst]:.3g} (Z{worst[0]} {worst[1]}); per zone " +
          ", ".join(f"Z{z} {k} {r:.3g}" for (z, k), r in ratios.items()))
    assert all(r > 1.0 for r in ratios.values()), (entry, ratios)


def _float_ratio(bad, ref, bar):
    err = np.abs(bad - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.max(np.where(err == 0, 0.0, err / bar)))


def _count_ratio(bad, ref, allowed):
    """integers are outside where they differ by more than `allowed`: the ratio is taken to allowed + 1/2"""
    return float(np.max(np.abs(bad - ref) / (allowed + 0.5)))


def test_sensitivity_displacements():
    atoms = B.MSD["atoms"]
    ref, bar, counts, allowed, _, _ = B.msd_reference(B.compact(B.SEED_POSITIONS, atoms))
    moments, hist = {}, {}
    for zone, kind, bad in _faulted(B.SEED_POSITIONS, atoms):
        m, _, c, _, _, _ = B.msd_reference(bad)
        moments[zone, kind], hist[zone, kind] = _float_ratio(m, ref, bar), _count_ratio(c, counts, allowed)
    _report("displacement_moments (msd64)", moments)
    _report("van_hove_self (msd64)", hist)


@pytest.mark.parametrize("box,parts", B.PAIR["layouts"])
def test_sensitivity_pairs(box, parts):
    atoms = B.PAIR["atoms"]
    ref, allowed, _, _ = B.pair_reference(B.compact(B.SEED_POSITIONS, atoms), box, parts)
    ratios = {(zone, kind): _count_ratio(B.pair_reference(bad, box, parts)[0], ref, allowed)
              for zone, kind, bad in _faulted(B.SEED_POSITIONS, atoms)}
    _report(f"pair_histogram {box} (pair64)", ratios)


@pytest.mark.parametrize("layout", ["whole", "z3", "spanning"])
def test_sensitivity_vdos(layout):
    atoms = B.VDOS["atoms"]
    lay = B.segment_layouts()[layout]
    _, w = B.listed_weights(atoms, 6)
    ref, bound = B.vdos_reference(B.compact(B.SEED_VELOCITIES, atoms), lay, w)
    ratios = {(zone, kind): _float_ratio(B.vdos_reference(bad, lay, w)[0], ref, bound)
              for zone, kind, bad in _faulted(B.SEED_VELOCITIES, atoms) if layout != "z3" or zone == 3}
    _report(f"vdos {layout} (vdos64)", ratios)


SLOTS = [("positions", B.SEED_POSITIONS), ("velocities", B.SEED_VELOCITIES)]


@pytest.mark.parametrize("slot,seed", SLOTS)
def test_sensitivity_dynamic(slot, seed):
    """a fault in the positions and a fault in the velocities, each alone: the two slots are addressed separately"""
    atoms = B.DYNAMIC["atoms"]
    pos, vel = B.compact(B.SEED_POSITIONS, atoms), B.compact(B.SEED_VELOCITIES, atoms)
    _, w = B.listed_weights(atoms, 7)
    lay = B.segment_layouts()["spanning"]
    ref, bound = B.dynamic_reference(pos, vel, w)
    spectra = B.dynamic_spectra_reference(pos, vel, w, lay)
    project, power = {}, {}
    for zone, kind, bad in _faulted(seed, atoms):
        p, v = (bad, vel) if slot == "positions" else (pos, bad)
        project[zone, kind] = _float_ratio(B.dynamic_reference(p, v, w)[0], ref, bound[None])
        got = B.dynamic_spectra_reference(p, v, w, lay)
        fields = (0, 1, 2) if slot == "positions" else (1, 2)          # the density reads no velocity
        power[zone, kind] = min(rel_max(got[i], spectra[i]) for i in fields) / B.DYNAMIC_SPECTRA_BAR
    _report(f"debug_dynamic_project, faulted {slot} (dynamic64.project64)", project)
    _report(f"dynamic_spectra, faulted {slot} (dynamic64)", power)


def test_sensitivity_mean_positions():
    """the mean is compared bit for bit: any changed bit is outside"""
    atoms = B.MEAN["atoms"]
    ref = B.mean32(B.compact(B.SEED_POSITIONS, atoms))
    ratios = {(zone, kind): float(np.count_nonzero(B.mean32(bad) != ref)) / 0.5     # allowance 0: as for the counts
              for zone, kind, bad in _faulted(B.SEED_POSITIONS, atoms)}
    assert all(r > 0.95 * ref.size / 0.5 for r in ratios.values())         # nearly every listed element changes
    _report("mean_positions (sequential float32 mean)", ratios)


@pytest.mark.parametrize("slot,seed", SLOTS)
def test_sensitivity_lattice_and_partial(slot, seed):
    """the lattice stager reads both slots: a fault in either, each alone"""
    atoms = B.LATTICE["atoms"]
    pos, vel = B.compact(B.SEED_POSITIONS, atoms), B.compact(B.SEED_VELOCITIES, atoms)
    _, w = B.listed_weights(atoms, 8)
    lay = B.segment_layouts()["spanning"]
    ref, bound = B.lattice_reference(pos, vel, w)
    spectra = B.lattice_spectra_reference(ref, lay)
    partial = B.partial_spectra_reference(pos, vel, w, lay)
    correlations = B.lattice_correlations_reference(ref)
    project, power, pairs, lagged = {}, {}, {}, {}
    fields = (0, 1, 2) if slot == "positions" else (1, 2)              # the density reads no velocity
    for zone, kind, bad in _faulted(seed, atoms):
        p, v = (bad, vel) if slot == "positions" else (pos, bad)
        q = B.lattice_reference(p, v, w)[0]
        project[zone, kind] = _float_ratio(q, ref, bound[None])
        got = B.lattice_spectra_reference(q, lay)
        power[zone, kind] = min(rel_max(got[i], spectra[i]) for i in fields) / B.SPECTRA_BAR
        got = B.partial_spectra_reference(p, v, w, lay)
        pairs[zone, kind] = min(B.pair_errors(got[i], partial[i]) for i in fields) / B.SPECTRA_BAR
        got = B.lattice_correlations_reference(q)
        lagged[zone, kind] = min(B.correlation_fraction(got[i], correlations[i]) for i in fields)
    _report(f"debug_lattice_project / debug_partial_project, faulted {slot} (lattice64.project64)", project)
    _report(f"lattice_spectra, faulted {slot} (lattice64)", power)
    _report(f"partial_spectra, faulted {slot} (partial64)", pairs)
    _report(f"lattice_correlations, faulted {slot} (correlation64)", lagged)


def test_sensitivity_self():
    atoms = B.SELF["atoms"]
    pos = B.compact(B.SEED_POSITIONS, atoms)
    _, w = B.listed_weights(atoms, 9)
    lay = B.segment_layouts()["spanning"]
    ref, bound = B.self_reference(pos, w)
    spectra = B.self_spectra_reference(pos, w, lay)
    lagged_ref = B.self_correlations_reference(pos, w)
    series, power, lagged = {}, {}, {}
    for zone, kind, bad in _faulted(B.SEED_POSITIONS, atoms):
        series[zone, kind] = _float_ratio(B.self_reference(bad, w)[0], ref, bound)
        lagged[zone, kind] = B.correlation_fraction(B.self_correlations_reference(bad, w), lagged_ref)
        power[zone, kind] = B.column_rel_max(B.self_spectra_reference(bad, w, lay), spectra) / B.SPECTRA_BAR
    _report("debug_self_series (self64.series64)", series)
    _report("self_spectra (self64)", power)
    _report("self_correlations (correlation64)", lagged)


def test_sensitivity_sed_projection():
    """ref64.project64, the reference of Engine.calculate, Engine.single_bin and the mode and covariance entry points: per
    element in units of B against the largest bound of any form; the intensity and one bin against their bars"""
    import dense_cases
    import ref64
    import spectral_cases
    atoms = B.SED["atoms"]
    vel = B.compact(B.SEED_VELOCITIES, atoms)
    _, r, k = B.sed_inputs()
    _, w = B.listed_weights(atoms, 10)
    groups = B.compact_groups(B.species(atoms, B.SED["parts"]))
    ref, scale = B.sed_reference(vel, r, k, w)
    widest = max(dense_cases.bound(form, atoms.size) for form, _, _ in B.SED["forms"])
    inten = ref64.intensity64(vel, r, k, groups, w)
    project, e2e, one_bin = {}, {}, {}
    for zone, kind, bad in _faulted(B.SEED_VELOCITIES, atoms):
        q = B.sed_reference(bad, r, k, w)[0]
        project[zone, kind] = ref64.gamma(q, ref, scale) / widest
        got = ref64.intensity64(bad, r, k, groups, w)
        e2e[zone, kind] = min(rel_max(got, inten) / B.E2E_TOL, float(ref64.row_rel(got, inten).max()) / B.E2E_TOL_ROW)
        worst = np.inf
        for b in B.SED["bins"]:
            want, moved = spectral_cases.single_bin_ref64(ref[0], b), spectral_cases.single_bin_ref64(q[0], b)
            bar = spectral_cases.single_bin_bar("bf16x3", atoms.size, scale, want)
            worst = min(worst, float(np.max(np.maximum(np.abs(moved.real - want.real), np.abs(moved.imag - want.imag)) / bar)))
        one_bin[zone, kind] = worst
    _report("debug_project_only (ref64.project64, gamma over the widest bound)", project)
    _report("Engine.calculate, two groups (ref64.intensity64)", e2e)
    _report("Engine.single_bin, every listed bin (float64 DFT of ref64.project64)", one_bin)


def test_angle_case_conditions_and_sensitivity():
    """the borderline cap of tests/angle_cases.py is met by the reference alone, no centre comes near 64 neighbours, and a
    fault in any zone moves the angle counts beyond what they may differ by"""
    import angle_cases
    atoms, n_theta = B.ANGLE["atoms"], B.ANGLE["n_theta"]
    ref = B.angle_reference(B.compact(B.SEED_POSITIONS, atoms))
    print(f"angles: {ref['borderline']} borderline of {ref['triplets']} triplets, most neighbours {ref['most']}")
    assert ref["triplets"] > 1000 and ref["borderline"] <= angle_cases.cap(n_theta) * ref["triplets"]
    assert ref["most"] <= 32 and not ref["truncated"].any()
    ratios = {}
    for zone, kind, bad in _faulted(B.SEED_POSITIONS, atoms):
        got = B.angle_reference(bad)
        ratios[zone, kind] = max(_count_ratio(got["angles"], ref["angles"], ref["angles_allowed"]),
                                 _count_ratio(got["coord"], ref["coord"], ref["coord_allowed"]))
    _report("angle_histogram (angle64)", ratios)


def test_sensitivity_modes_and_covariance():
    atoms = B.MODES["atoms"]
    vel = B.compact(B.SEED_VELOCITIES, atoms)
    _, w = B.listed_weights(atoms, 11)
    lay = B.segment_layouts()["spanning"]
    phi, welch, cov = B.modes_references(vel, w, lay)
    modes, averaged, matrices = {}, {}, {}
    for zone, kind, bad in _faulted(B.SEED_VELOCITIES, atoms):
        a, b, c = B.modes_references(bad, w, lay)
        modes[zone, kind] = rel_max(a, phi) / B.MODES_BAR
        averaged[zone, kind] = rel_max(b, welch) / B.MODES_BAR
        matrices[zone, kind] = B.matrix_rel_max(c, cov) / B.MODES_BAR
    _report("sed_modes (modes64)", modes)
    _report("sed_modes_welch (modes_welch64)", averaged)
    _report("sed_covariance (cov64)", matrices)


def test_order_case_conditions_and_sensitivity():
    """the excluded share of tests/order_cases.py is met by the reference alone; a fault in any zone changes neighbour counts
    (outside whatever the allowance: the ratio is infinite) or moves n^2 q_l^2 beyond its allowance"""
    import order_cases
    atoms = B.ORDER["atoms"]
    ref = B.order_reference(B.compact(B.SEED_POSITIONS, atoms))
    assert order_cases.excluded_share(ref) <= order_cases.EXCLUDED_CAP and (ref["why"] == 0).sum() > 500
    ratios = {}
    for zone, kind, bad in _faulted(B.SEED_POSITIONS, atoms):
        got = B.order_reference(bad)
        keep = ~ref["excluded"]
        if not np.array_equal(got["n"][keep], ref["n"][keep]):
            ratios[zone, kind] = np.inf
            continue
        both = keep & (ref["why"] == 0)
        ratios[zone, kind] = float(np.max(np.abs(got["xq"][both] - ref["xq"][both]) / ref["allowed"][both]))
    _report("bond_order (order64)", ratios)


def test_local_order_case_conditions_and_sensitivity():
    """qlm_cases' excluded and loose shares are met by the reference alone; a fault in any zone changes the neighbour counts
    (outside whatever the allowance) or moves q-bar^2 beyond its allowance"""
    import qlm_cases
    atoms = B.LOCAL["atoms"]
    ref = B.local_reference(B.compact(B.SEED_POSITIONS, atoms))
    print(f"local order: excluded share {qlm_cases.excluded_share(ref):.2e}, loose share {qlm_cases.loose_share(ref):.2e}")
    assert qlm_cases.excluded_share(ref) <= qlm_cases.EXCLUDED_CAP and qlm_cases.loose_share(ref) <= qlm_cases.EXCLUDED_CAP
    ratios = {}
    for zone, kind, bad in _faulted(B.SEED_POSITIONS, atoms):
        got = B.local_reference(bad)
        keep = ~ref["excluded"]
        same = np.array_equal(got["n"][keep], ref["n"][keep]) and np.array_equal(got["xi"][keep], ref["xi"][keep])
        ratios[zone, kind] = 0.0 if same else np.inf
    _report("local_order (qlm64)", ratios)


@pytest.mark.parametrize("link", B.CLUSTER["links"])
def test_cluster_case_and_sensitivity(link):
    """the twin finds solid atoms and clusters in the case; a fault in any zone changes labels, counts or connections, which
    the GPU test compares exactly"""
    import cluster_cases
    atoms = B.CLUSTER["atoms"]
    want = B.cluster_twin(B.compact(B.SEED_POSITIONS, atoms), link)
    assert np.asarray(want["n_solid"]).sum() > 20 and np.asarray(want["n_clusters"]).sum() > 5 and cluster_cases.identities(want)
    ratios = {(zone, kind): len(cluster_cases.differs(B.cluster_twin(bad, link), want, B.CLUSTER_KEYS)) / 0.5
              for zone, kind, bad in _faulted(B.SEED_POSITIONS, atoms)}
    _report(f"solid_clusters link {link} (the cluster twin; keys that differ over an allowance of none)", ratios)
