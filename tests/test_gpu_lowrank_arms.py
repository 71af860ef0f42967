"""The packed combine of the low-rank k-path route (lowrank_combine.hip) gives the bits of the scalar one
(k1_planes_diff.hip) at configuration 3 and on a tail shape (frame and atom tails, two 512-row D blocks, an odd last
row pair).  The arm is chosen when an engine is created (PSA_K1_COMBINE), so each arm gets an engine of its own."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ARMS = ["0", "1"]                  # PSA_K1_COMBINE: the scalar combine, the packed one


def _engine(arm):
    from psa_amd import _hip
    old = os.environ.get("PSA_K1_COMBINE")
    os.environ["PSA_K1_COMBINE"] = arm
    try:
        return _hip.Engine(0)
    finally:
        if old is None:
            os.environ.pop("PSA_K1_COMBINE", None)
        else:
            os.environ["PSA_K1_COMBINE"] = old


def _assert_same_bits(out):
    ref = out[ARMS[0]].view(np.uint32)
    for arm in ARMS[1:]:
        diff = np.count_nonzero(out[arm].view(np.uint32) != ref)
        assert diff == 0, f"arm {arm}: {diff} of {ref.size} words differ from the scalar combine"


def test_config3_arms_bit_identical():
    from psa_amd import SEDCalculator, Trajectory, _hip, synth
    spec, req = synth.baseline_spec("C3")
    r0, types, box = synth.lattice(spec.cells)
    tables = synth.mode_tables(spec, r0)
    stub = np.zeros((1, spec.n_atoms, 3), np.float32)
    calc = SEDCalculator(Trajectory(stub, stub, types, np.zeros(1, np.float32), box, np.diag(box).copy(),
                                    np.zeros(3, np.float32), spec.dt_ps), *spec.cells)
    _, vecs = calc.get_k_path(req["direction"], req["bz_coverage"], req["n_k"])
    vecs = np.asarray(vecs, np.float32)
    T, K = spec.n_frames, len(vecs)
    out = {}
    for arm in ARMS:
        eng = _engine(arm)
        try:
            synth.fill_device(eng, _hip.SLOT_VELOCITIES, spec, tables)
            n0 = eng.lowrank_launches()
            eng.project(_hip.SLOT_VELOCITIES, r0, vecs, None, 0)
            out[arm] = eng.finalize(T, K, False)
            assert eng.lowrank_launches() - n0 == 1                  # the route was taken
        finally:
            eng.close()
    _assert_same_bits(out)


def test_tail_shape_arms_bit_identical():
    """T = 1000, 1000 atoms, 301 k-vectors on [100] from Gamma: 602 rows = two D blocks, 301 rows = an odd last pair."""
    from psa_amd import _hip
    rng = np.random.default_rng(5)
    T, N, K = 1000, 1000, 301
    r0 = (rng.random((N, 3)) * 28.0).astype(np.float32)
    vecs = (np.linspace(0.0, 1.9, K)[:, None] * np.array([1.0, 0.0, 0.0])).astype(np.float32)
    x = (rng.standard_normal((T, N, 3)) * 0.3).astype(np.float32)
    out = {}
    for arm in ARMS:
        eng = _engine(arm)
        try:
            eng.ensure_resident(_hip.SLOT_POSITIONS, x)
            eng.set_option(_hip.OPT_PLANES_EAGER, 1)
            eng.set_option(_hip.OPT_K1_LOWRANK_MIN_K, 1)
            eng.set_option(_hip.OPT_K1_LOWRANK_MIN_LOCAL, 1)
            n0 = eng.lowrank_launches()
            eng.project(_hip.SLOT_POSITIONS, r0, vecs, None, 0)
            out[arm] = eng.finalize(T, K, False)
            assert eng.lowrank_launches() - n0 == 1
        finally:
            eng.close()
    _assert_same_bits(out)
