"""Host-side tests of the pair distributions: the NumPy twin of the arithmetic stated in psa_amd/csrc/pair.hip stays inside
the allowance of tests/pair_cases.py on every input family, with exact totals; each planted fault leaves it on at least
one family; the references' borderline share is under the cap the GPU tests assert first; `max_pair_radius` against a
searched minimum image on a strongly tilted box; the result types and every Python-side refusal."""
import functools
import itertools

import numpy as np
import pytest

import pair64 as R
import pair_cases as P

BOXES = {"cubic": P.CUBIC, "triclinic": P.TRICLINIC}
N, T = 60, 6
LAGS = [0, 3]
GROUPS = [np.arange(0, 25), np.arange(25, N)]


@functools.lru_cache(maxsize=None)
def _family(box, family):
    if family == "frozen":
        return P.frozen(N, T, seed=2, box=BOXES[box])
    return P.walk(N, T, seed=1, box=BOXES[box])[family]


@functools.lru_cache(maxsize=None)
def _reference(box, family, n_r):
    from psa_amd import max_pair_radius
    dr = max_pair_radius(BOXES[box]) / n_r
    return (dr,) + P.reference(_family(box, family), BOXES[box], GROUPS, LAGS, 1, dr, n_r)


FAMILIES = ("wrapped", "unwrapped", "shifted", "frozen")


@pytest.mark.parametrize("n_r", [64, 1024])
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("box", BOXES)
def test_twin_inside_the_allowance(box, family, n_r):
    dr, ref, allowed, borderline, total = _reference(box, family, n_r)
    assert borderline <= P.cap(n_r) * total                                 # the borderline condition
    got = P.histogram_model(_family(box, family), BOXES[box], GROUPS, LAGS, 1, dr, n_r)
    moved = int(np.abs(got - ref).sum())
    print(f"{box} {family} n_r {n_r}: {borderline} borderline of {total}, {moved} moved")
    assert np.array_equal(got.sum(axis=3), P.expected_totals(T, GROUPS, LAGS, 1))
    assert np.array_equal(ref.sum(axis=3), P.expected_totals(T, GROUPS, LAGS, 1))
    assert np.all(np.abs(got - ref) <= allowed)
    assert np.array_equal(got[0], got[0].transpose(1, 0, 2))                # tau = 0: (a, b) = (b, a)


@pytest.mark.parametrize("box", P.LATTICE_BOXES)
def test_twin_on_the_simple_cubic_lattice(box):
    """the lattice family on the cubic and on the sheared cell, bins of 0.65 with the shells (x = 8.35, 11.81, 14.47) away
    from every edge: no borderline sample at all, the twin equal to the reference, 6, 12 and 8 neighbours"""
    from psa_amd import max_pair_radius
    H = P.LATTICE_BOXES[box]
    pos, a = P.simple_cubic(4, box)
    n_r, dr, groups, lags = 16, 0.65, [np.arange(0, 20), np.arange(20, 64)], [0, 2]
    assert n_r * dr <= max_pair_radius(H) and n_r * dr < 2 * a
    ref, allowed, borderline, total = P.reference(pos, H, groups, lags, 1, dr, n_r)
    assert borderline <= P.cap(n_r) * total and borderline == 0
    got = P.histogram_model(pos, H, groups, lags, 1, dr, n_r)
    assert np.array_equal(got.sum(axis=3), P.expected_totals(4, groups, lags, 1))
    assert np.all(np.abs(got - ref) <= allowed) and np.array_equal(got, ref)
    per_atom = ref[0, :, :, :n_r].sum(axis=1) / (4.0 * np.array([20, 44])[:, None])
    assert np.array_equal(per_atom[:, [8, 11, 14]], [[6, 12, 8]] * 2) and per_atom.sum() == 2 * 26
    for fault in ("no_image", "orthogonal_only"):                          # the sheared cell needs both the image and the tilt
        bad = P.histogram_model(pos, H, groups, lags, 1, dr, n_r, fault=fault)
        assert np.any(np.abs(bad - ref) > allowed) or (fault == "orthogonal_only" and box == "cubic")


# ---- the host's item table ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sym", [True, False])
def test_an_items_samples_stay_below_2_to_32(sym):
    """psa_debug_pair_plan over sizes that give runs of 1 .. 256 beta-tiles (runs that are and are not powers of two) and
    origin blocks at and around the multiples of 65535 / run: the most samples of an item stay below 2^32"""
    from psa_amd import _hip
    tile = _hip.PAIR_TILE
    for tiles in (1, 3, 64, 91, 128, 170, 256, 340, 512, 1024):
        sizes = [tiles * tile - 5]
        for n_ob in (1, 2, 255, 256, 257, 511, 512, 9362, 9363, 32767, 32768, 65535):
            plan = _hip.Engine.debug_pair_plan(sizes, sym, n_ob)
            assert plan["most_samples"] < 2 ** 32, (tiles, n_ob, plan)
            assert 1 <= plan["run"] <= 256 and 1 <= plan["slabs"] <= n_ob
            per_slab = -(-n_ob // plan["slabs"])
            assert per_slab * plan["run"] <= 65535
    two = _hip.Engine.debug_pair_plan([0, 700, 3], sym, 40)
    assert two["items"] > 0 and two["most_samples"] < 2 ** 32
    assert _hip.Engine.debug_pair_plan([0, 0], sym, 5)["items"] == 0
    for bad in (([5] * 9, 3), ([-1], 3), ([5], 0), ([5], 65536)):
        with pytest.raises(_hip.PsaHipError):
            _hip.Engine.debug_pair_plan(bad[0], sym, bad[1])


# the family on which each fault must show:# the family on which each fault must show: frac32 moves counts only far from the origin, orthogonal_only only where the box
# is tilted
FAULT_FAMILY = {"no_image": ("cubic", "wrapped"), "frac32": ("triclinic", "shifted"), "orthogonal_only": ("triclinic", "wrapped"),
                "same_frame": ("cubic", "wrapped"), "self_included": ("cubic", "wrapped"), "diagonal_doubled": ("cubic", "wrapped"),
                "bin_shift": ("cubic", "frozen")}


@pytest.mark.parametrize("fault", P.FAULTS)
def test_faults_leave_the_allowance(fault):
    box, family = FAULT_FAMILY[fault]
    dr, ref, allowed, _, _ = _reference(box, family, 64)
    got = P.histogram_model(_family(box, family), BOXES[box], GROUPS, LAGS, 1, dr, 64, fault=fault)
    broken = int((np.abs(got - ref) > allowed).sum())
    print(f"{fault} on {box} {family}: {broken} bins outside the allowance")
    assert broken >= 1


def test_frac32_shows_only_far_from_the_origin():
    dr, ref, allowed, _, _ = _reference("cubic", "wrapped", 64)
    got = P.histogram_model(_family("cubic", "wrapped"), P.CUBIC, GROUPS, LAGS, 1, dr, 64, fault="frac32")
    assert np.all(np.abs(got - ref) <= allowed)


def test_reference_min_image_is_invariant_under_box_moves():
    """the brute force on the wrapped and on the moved input: the moves are whole box vectors up to the float32 rounding"""
    box = P.TRICLINIC
    w = P.walk(20, 4, seed=5, box=box)
    ra = R.pair_samples(w["wrapped"], box, np.arange(20), np.arange(20), 1)[2]
    rb = R.pair_samples(w["moved"], box, np.arange(20), np.arange(20), 1)[2]
    assert np.all(np.abs(ra - rb) <= 4 * np.sqrt(3.0) * 2.0 ** -24 * np.abs(w["moved"]).max())


# ---- the served radius ------------------------------------------------------------------------------------------------
def test_max_pair_radius_on_a_strongly_tilted_box():
    from psa_amd import max_pair_radius
    box = np.array([[10.0, 0.0, 0.0], [7.0, 9.0, 0.0], [-6.0, 5.0, 8.0]], np.float32)
    H = box.astype(np.float64)
    a, b, c = H
    vol = abs(np.linalg.det(H))
    widths = [vol / np.linalg.norm(np.cross(b, c)), vol / np.linalg.norm(np.cross(c, a)), vol / np.linalg.norm(np.cross(a, b))]
    r_max = max_pair_radius(box)
    assert np.isclose(r_max, (0.5 - 2.0 ** -12) * min(widths), rtol=1e-12) and r_max < 0.5 * min(np.linalg.norm(H, axis=1))
    # rounding the fractional difference against a search over n in {-3..3}^3: equal wherever the searched image is
    # within r_max, and not everywhere beyond half the least width
    f = np.random.default_rng(0).uniform(-0.5, 0.5, (200000, 3))
    images = np.array(list(itertools.product(range(-3, 4), repeat=3)), np.float64)
    best = np.full(f.shape[0], np.inf)
    for lo in range(0, images.shape[0], 49):
        best = np.minimum(best, np.linalg.norm((f[:, None, :] + images[None, lo:lo + 49, :]) @ H, axis=2).min(axis=1))
    rounded = np.linalg.norm((f - np.rint(f)) @ H, axis=1)
    inside = best <= r_max
    assert inside.sum() > 1000 and np.array_equal(rounded[inside], best[inside])
    assert np.any(rounded > best * (1 + 1e-9))                              # the tilt does make rounding miss, farther out
    for bad in (np.zeros((3, 3)), np.ones((2, 3)), [[1, 0, 0], [0, 1, 0], [0, 0, np.nan]], [[1, 0, 0], [0, 1, 0], [1, 1, 0]]):
        with pytest.raises(ValueError):
            max_pair_radius(bad)


# ---- the result types -------------------------------------------------------------------------------------------------
def _gas(n, T, box, seed=3):
    H = np.asarray(box, np.float32).astype(np.float64)
    return (np.random.default_rng(seed).uniform(0.0, 1.0, (T, n, 3)) @ H).astype(np.float32)


def test_radial_distribution_of_a_uniform_gas():
    """g of an ideal gas is 1 - delta_ab / N_b within counting statistics: every bin, the outer half together and the
    coordination number at r_max within five standard deviations of their Poisson expectation (an unordered pair of one
    species is counted twice: the variance is twice the mean)"""
    from psa_amd import RadialDistribution, max_pair_radius
    box, n, frames, n_r = P.TRICLINIC, 150, 8, 20
    groups = [np.arange(0, 50), np.arange(50, n)]
    r_max = max_pair_radius(box)
    dr = r_max / n_r
    pos = _gas(n, frames, box)
    out = R.counts64(pos, box, groups, [0], 1, dr, n_r)[0]
    sizes = np.array([50, 100], np.int64)
    samples = P.expected_totals(frames, groups, [0], 1)[0]
    edges = dr * np.arange(n_r + 1)
    vol = abs(np.linalg.det(np.asarray(box, np.float64)))
    rd = RadialDistribution(out[:, :, :n_r].astype(np.uint64), out[:, :, n_r].astype(np.uint64), samples, edges,
                            0.5 * (edges[1:] + edges[:-1]), vol, groups, sizes, frames)
    assert np.array_equal(rd.counts.sum(axis=2) + rd.overflow, samples.astype(np.uint64))
    shell = 4 * np.pi / 3 * (edges[1:] ** 3 - edges[:-1] ** 3)
    for a in range(2):
        for b in range(2):
            ideal = 1.0 - (a == b) / sizes[b]
            expect = frames * sizes[a] * (sizes[b] - (a == b)) * shell / vol            # counts of the ideal gas
            assert np.all(np.abs(rd.counts[a, b] - expect) <= 5.0 * np.sqrt(2.0 * expect) + 1.0)
            outer = slice(n_r // 2, None)
            assert abs(float(rd.counts[a, b, outer].sum()) - expect[outer].sum()) <= 5.0 * np.sqrt(2.0 * expect[outer].sum())
            assert abs((rd.g[a, b, outer] * shell[outer]).sum() / shell[outer].sum() - ideal) <= 5.0 * ideal * np.sqrt(2.0 / expect[outer].sum())
            assert np.allclose(rd.g[a, b] * expect / ideal, rd.counts[a, b], rtol=1e-12)
            assert np.array_equal(rd.pair(a, b), rd.g[a, b])
            # the coordination number: cumsum of counts per a-atom and frame; -> rho_b times the volume of the sphere
            assert np.allclose(rd.coordination[a, b], np.cumsum(out[a, b, :n_r]) / (frames * sizes[a]), rtol=1e-14)
            assert abs(rd.coordination[a, b, -1] / ((sizes[b] - (a == b)) / vol * 4 * np.pi / 3 * r_max ** 3) - 1.0) \
                <= 5.0 * np.sqrt(2.0 / expect.sum())


def test_van_hove_distinct_normalisations():
    from psa_amd import VanHoveDistinct
    box, n, frames, n_r, dr = P.CUBIC, 40, 9, 16, 0.6
    groups = [np.arange(0, 15), np.zeros(0, np.int64), np.arange(15, n)]
    lags, step = np.array([0, 2, 8]), 2
    out = R.counts64(_gas(n, frames, box), box, groups, lags, step, dr, n_r)
    sizes = np.array([15, 0, 25], np.int64)
    samples = P.expected_totals(frames, groups, lags, step)
    n_o = np.array([R.n_origins(frames, int(t), step) for t in lags])
    edges = dr * np.arange(n_r + 1)
    vol = float(np.float64(box[0, 0]) ** 3)
    vh = VanHoveDistinct(out[..., :n_r].astype(np.uint64), out[..., n_r].astype(np.uint64), samples, edges, 0.5 * (edges[1:] + edges[:-1]),
                         vol, groups, sizes, n_o, lags, lags * 0.002, 0.002)
    assert np.array_equal(vh.counts.sum(axis=3) + vh.overflow, samples.astype(np.uint64))
    assert not vh.g_d[:, 1].any() and not vh.g_d[:, :, 1].any() and np.all(np.isfinite(vh.g_d))        # the empty species: zeros
    per = n_o[:, None, None, None] * sizes[None, :, None, None]
    live = [0, 2]
    assert np.allclose(vh.radial_density[:, live] * dr, out[:, live, :, :n_r] / per[:, live], rtol=1e-14)
    shell = 4 * np.pi / 3 * (edges[1:] ** 3 - edges[:-1] ** 3)
    assert np.allclose(vh.g_d[:, 0, 2], out[:, 0, 2, :n_r] / (n_o[:, None] * 15 * (25 / vol) * shell), rtol=1e-14)
    assert np.allclose(vh.coordination[:, 2, 0, -1], out[:, 2, 0, :n_r].sum(axis=1) / (n_o * 25), rtol=1e-14)
    assert np.array_equal(vh.pair(0, 2), vh.g_d[:, 0, 2])


# ---- the calculator's host side ---------------------------------------------------------------------------------------
def _calculator(pos, box, types=None):
    from psa_amd import SEDCalculator, Trajectory
    n_t, n = pos.shape[:2]
    box = np.asarray(box, np.float32)
    tr = Trajectory(pos, np.zeros_like(pos), np.ones(n, np.int32) if types is None else types, np.arange(n_t, dtype=np.float32), box,
                    np.diag(box).copy(), np.zeros(3, np.float32), 0.002)
    return SEDCalculator(tr, 1, 1, 1)


def test_zero_result_path(caplog):
    from psa_amd import RadialDistribution, VanHoveDistinct, max_pair_radius
    calc = _calculator(np.zeros((0, 5, 3), np.float32), P.CUBIC)
    rd = calc.calculate_rdf(n_r=10)
    assert isinstance(rd, RadialDistribution) and rd.counts.shape == (1, 1, 10) and not rd.counts.any() and not rd.g.any()
    assert not rd.coordination.any() and rd.origins == 0 and np.isclose(rd.r_edges[-1], max_pair_radius(P.CUBIC))
    vh = calc.calculate_distinct_van_hove([0, 4], 5.0, 8)
    assert isinstance(vh, VanHoveDistinct) and vh.counts.shape == (2, 1, 1, 8) and not vh.g_d.any() and not vh.radial_density.any()
    assert np.array_equal(vh.lag_frames, [0, 4]) and "0 frames or 0 atoms" in caplog.text


def test_python_side_refusals():
    from psa_amd import max_pair_radius
    pos = _gas(12, 5, P.TRICLINIC)
    calc = _calculator(pos, P.TRICLINIC, (np.arange(12) % 2 + 1).astype(np.int32))
    served = max_pair_radius(P.TRICLINIC)
    for kw in (dict(r_max=served * 1.001), dict(r_max=0.0), dict(r_max=-1.0), dict(r_max=float("nan")), dict(r_max=float("inf")),
               dict(n_r=0), dict(n_r=1025), dict(n_r=2.5), dict(n_r=True), dict(origin_step=0), dict(origin_step=1.5),
               dict(basis_atom_indices=[[0, 1], [1, 2]]), dict(basis_atom_indices=[[i] for i in range(9)]), dict(max_atoms=0)):
        with pytest.raises(ValueError):
            calc.calculate_rdf(**kw)
        with pytest.raises(ValueError):
            calc.calculate_distinct_van_hove([0, 1], **kw)
    for lags in ([], list(range(65)), [0.5], [-1], [5], [[0, 1]]):
        with pytest.raises(ValueError):
            calc.calculate_distinct_van_hove(lags, 3.0, 8)

    class Sharded:
        nranks = 2
    calc._shard = Sharded()
    with pytest.raises(NotImplementedError):
        calc.calculate_rdf()
    with pytest.raises(NotImplementedError):
        calc.calculate_distinct_van_hove([1])
