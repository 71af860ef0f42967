"""The low-rank route for k-paths on the GPU (k1_planes_diff.hip): configuration 3's full trajectory against the dense
planes kernels and split over calls (bit-identical rows), and odd shapes -- frame and atom tails, a tiny atom axis,
several 512-row D blocks, index lists with duplicates, displacement mode -- with the route forced on."""
import numpy as np
import pytest

from conftest import rel_max
from engine_state import reset

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def c3(engine):
    from psa_amd import SEDCalculator, Trajectory, _hip, synth
    spec, req = synth.baseline_spec("C3")
    r0, types, box = synth.lattice(spec.cells)
    tables = synth.mode_tables(spec, r0)
    synth.fill_device(engine, _hip.SLOT_VELOCITIES, spec, tables)
    stub = np.zeros((1, spec.n_atoms, 3), np.float32)
    calc = SEDCalculator(Trajectory(stub, stub, types, np.zeros(1, np.float32), box, np.diag(box).copy(),
                                    np.zeros(3, np.float32), spec.dt_ps), *spec.cells)
    _, vecs = calc.get_k_path(req["direction"], req["bz_coverage"], req["n_k"])
    yield dict(spec=spec, r0=r0, types=types, vecs=np.asarray(vecs, np.float32))
    reset(engine)
    engine.release(_hip.SLOT_VELOCITIES)


def _sed(engine, c3, parts, lowrank, min_local=128):
    """The complex result of the parts [lo, hi) of the list, projected one call each; and the launches that took the route"""
    from psa_amd import _hip
    T, K = c3["spec"].n_frames, len(c3["vecs"])
    engine.set_option(_hip.OPT_K1_LOWRANK, 1 if lowrank else 0)
    engine.set_option(_hip.OPT_K1_LOWRANK_MIN_LOCAL, min_local)
    n0 = engine.lowrank_launches()
    for lo, hi in parts:
        engine.project(_hip.SLOT_VELOCITIES, c3["r0"], c3["vecs"][lo:hi], None, 0, K_total=K, k_offset=lo)
    out = engine.finalize(T, K, False)
    return out, engine.lowrank_launches() - n0


def test_config3_lowrank_against_dense_and_split(engine, c3):
    K = len(c3["vecs"])
    dense, n = _sed(engine, c3, [(0, K)], False)
    assert n == 0
    whole, n = _sed(engine, c3, [(0, K)], True)
    assert n == 1                                                      # the route was taken
    err = rel_max(whole, dense)
    print(f"lowrank vs dense rel_max {err:.3e}")
    assert err <= 1e-6
    inten_dense = np.sum(np.abs(dense) ** 2, axis=-1)
    del dense
    bits = whole.view(np.uint32)
    # three splits, every part on the route: bit-identical rows (a 96-vector part needs the per-launch minimum lowered)
    for parts, min_local in (([(0, K // 2), (K // 2, K)], 128), ([(K // 2, K), (0, K // 2)], 128), ([(0, 96), (96, K)], 64)):
        got, n = _sed(engine, c3, parts, True, min_local)
        assert n == len(parts), parts
        assert np.array_equal(got.view(np.uint32), bits), parts
    # the setting of a k-sharded multi-rank run: 128-vector shards stay on the dense kernels, split-invariant there
    got, n = _sed(engine, c3, [(0, K // 2), (K // 2, K)], True, 256)
    assert n == 0
    np.testing.assert_allclose(np.sum(np.abs(got) ** 2, axis=-1), inten_dense, rtol=1e-6, atol=0)
    assert rel_max(got, whole) <= 1e-6
    reset(engine)


def test_config3_incoherent_two_groups(engine, c3):
    """Two type groups, intensity summed over them: the route plans each group on its own x-range."""
    from psa_amd import _hip
    T, K = c3["spec"].n_frames, len(c3["vecs"])
    types = np.asarray(c3["types"])
    groups = [np.flatnonzero(types == t).astype(np.int32) for t in np.unique(types)]
    out = {}
    for lr in (0, 1):
        engine.set_option(_hip.OPT_K1_LOWRANK, lr)
        n0 = engine.lowrank_launches()
        engine.project(_hip.SLOT_VELOCITIES, c3["r0"], c3["vecs"], groups, _hip.F_INTENSITY)
        out[lr] = engine.finalize(T, K, True)
        assert engine.lowrank_launches() - n0 == (2 if lr else 0)
    err = rel_max(out[1], out[0])
    print(f"incoherent lowrank vs dense rel_max {err:.3e}")
    assert err <= 2e-6
    reset(engine)


@pytest.mark.parametrize("case", ["all_atoms", "index_dups", "displacements"])
def test_odd_shapes_against_dense(engine, case):
    """T = 1000 (a frame tail), 1000 atoms (an atom tail) or an index list of 40 with duplicates (two atom stages),
    300 k-vectors on [100] from Gamma (two 512-row D blocks), with the route forced on: against the dense route."""
    from psa_amd import _hip
    rng = np.random.default_rng(11)
    T, N, K = 1000, 1000, 300
    r0 = (rng.random((N, 3)) * 28.0).astype(np.float32)
    vecs = (np.linspace(0.0, 1.9, K)[:, None] * np.array([1.0, 0.0, 0.0])).astype(np.float32)
    x = (rng.standard_normal((T, N, 3)) * 0.3).astype(np.float32)
    groups, flags, slot = None, 0, _hip.SLOT_POSITIONS
    if case == "index_dups":
        idx = rng.integers(0, N, 40).astype(np.int32)
        idx[5] = idx[6] = idx[30]
        groups = [idx]
    if case == "displacements":
        flags = _hip.F_DISPLACEMENTS
        x = x + r0[None]
    try:
        engine.ensure_resident(slot, x)
        engine.set_option(_hip.OPT_PLANES_EAGER, 1)
        engine.set_option(_hip.OPT_K1_LOWRANK_MIN_K, 1)
        engine.set_option(_hip.OPT_K1_LOWRANK_MIN_LOCAL, 1)
        out, taken = {}, {}
        for lr in (0, 1):
            engine.set_option(_hip.OPT_K1_LOWRANK, lr)
            n0 = engine.lowrank_launches()
            engine.project(slot, r0, vecs, groups, flags)
            out[lr] = engine.finalize(T, K, False)
            taken[lr] = engine.lowrank_launches() - n0
        assert taken[0] == 0
        # displacement mode too: group_source takes the group's planes of positions - mean (get_planes builds them here:
        # all atoms, 300 k-vectors >= PSA_OPT_PLANES_MIN_K, finite data, room in HBM), the launch is a planes launch and
        # prepare_lowrank serves it like any other.  Only without that plane set -- the float32 displacement array or the
        # subtract-while-staging kernel -- does displacement mode stay off the route.
        assert taken[1] == 1
        err = rel_max(out[1], out[0])
        print(f"{case}: route taken {taken[1]}, lowrank vs dense rel_max {err:.3e}")
        assert err <= 1e-6
    finally:
        reset(engine)
        engine.release(slot)
