"""A destroyed context leaves no device buffer behind: the process-wide count of live allocations
(_hip.device_buffers) is back where it was after a context that used the weights, the Welch segments and the low-rank
route has been closed -- also when it is closed with the FFT primer still running, and after the route's early release."""
import numpy as np
import pytest

import lowrank_env_cases as E
from test_gpu_lowrank_envelope import _force

pytestmark = pytest.mark.gpu

LR_BUFFERS = 5                              # d_lr_diff, d_lr_qn, d_lr_L, d_lr_phi, d_lr_f64


@pytest.fixture(scope="module")
def inputs():
    """the default case of tests/lowrank_env_cases.py (K = 40, n_g = 257, T = 96) as velocities; positions around its
    mean positions in the cubic box of its edge; two species' weights; a handful of lattice vectors"""
    c = E.case("quiet_frames")
    n = c["r"].shape[0]
    pos = (c["r"][None] + np.float32(0.05) * c["data"]).astype(np.float32)
    weights = np.where(np.arange(n) % 2 == 0, 1.0, 2.0).astype(np.float32)
    indices = np.array([[1, 0, 0], [0, 2, 0], [1, 1, 0], [2, -1, 3], [0, 0, 1]], np.int32)
    return dict(vel=c["data"], pos=pos, r=c["r"], k=c["k"], weights=weights, indices=indices, inv=np.eye(3) / E.EDGE)


def _on_the_route(eng, x):
    """one intensity calculation on the k-path, by the forced low-rank route; the launches that took it"""
    from psa_amd import _hip
    _force(eng)
    n0 = eng.lowrank_launches()
    sed = eng.calculate(_hip.SLOT_VELOCITIES, x["r"], x["k"], None, _hip.F_INTENSITY)
    assert sed.shape == (eng.segment_length or x["vel"].shape[0], len(x["k"])) and np.all(np.isfinite(sed)) and sed.any()
    return eng.lowrank_launches() - n0


@pytest.mark.parametrize("cycle", [0, 1])
def test_full_cycle_returns_every_buffer(inputs, cycle):
    from psa_amd import Segments, _hip
    x = inputs
    base = _hip.device_buffers()
    eng = _hip.Engine(0)
    try:
        eng.ensure_resident(_hip.SLOT_POSITIONS, x["pos"])
        eng.ensure_resident(_hip.SLOT_VELOCITIES, x["vel"])
        eng.set_atom_weights(x["weights"])
        eng.set_segments(Segments(32, 16, "hann"))
        assert _on_the_route(eng, x) > 0
        assert eng.vdos(_hip.SLOT_VELOCITIES, None).shape == (17, 1, 3)
        assert eng.lattice_spectra(x["inv"], x["indices"]).shape == (3, 32, len(x["indices"]))
        held = _hip.device_buffers()
        print(f"cycle {cycle}: the context holds {held[0] - base[0]} buffers, {held[1] - base[1]} bytes")
        assert held[0] > base[0] and held[1] > base[1]
    finally:
        eng.close()
    assert _hip.device_buffers() == base


def test_close_with_the_primer_in_flight():
    from psa_amd import _hip
    base = _hip.device_buffers()
    eng = _hip.Engine(0)
    eng.alloc(_hip.SLOT_VELOCITIES, 1000, 8)            # starts the FFT primer for a length no other test uses
    assert _hip.device_buffers()[0] == base[0] + 1
    eng.close()
    assert _hip.device_buffers() == base


def test_route_switched_off_releases_its_buffers(inputs):
    from psa_amd import _hip
    x = inputs
    base = _hip.device_buffers()
    eng = _hip.Engine(0)
    try:
        eng.ensure_resident(_hip.SLOT_VELOCITIES, x["vel"])
        assert _on_the_route(eng, x) > 0
        on = _hip.device_buffers()
        eng.set_option(_hip.OPT_K1_LOWRANK, 0)
        off = _hip.device_buffers()
        assert on[0] - off[0] == LR_BUFFERS and off[1] < on[1]
        assert off[0] > base[0]
    finally:
        eng.close()
    assert _hip.device_buffers() == base
