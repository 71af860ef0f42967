"""The density of states on the GPU (psa_vdos: vdos.hip, api_vdos.hip) against the float64 restatement
(tests/vdos64.py), element by element, at the edges of its pair packing, tiles, blocks, chunks, fold and hops.

Straight through Engine.vdos on the arrays of tests/vdos_cases.py.  Every element D[o, g, c] of every case is held to
that module's bound -- 2 eta (D + sqrt(D R)) + eta^2 (sqrt D + sqrt R)^2 + the float64 and cast terms, eta =
(3 + log2 L) 2^-24, R the (group, component)'s mean power per bin -- which is derived from the arithmetic stated in
vdos.hip, with the FFT constant fixed on the CPU by a float32 twin (tests/test_vdos_envelope_host.py; the same file shows
that nine planted faults exceed the bound, seven of them while passing the older rel_max <= 1e-5).  The rows of empty
groups must be exactly zero.  One axis at a time around T = 256, Segments(64, 32, hann), groups of 45 and 111 atoms of
N = 300, each on noise and on a line 10^3 over the floor: atoms of one group, group layouts, segment lengths and runs
without segments, hops, work budgets (also bit for bit against the default budget), chunk counts of the power pass,
input families, displacement mode and weights.  Each case prints its shape, its worst ratio to the bound and rel_max.

Not reachable at these sizes (N <= 300, T <= 1100): the cap of 4096 bin tiles per row of the power pass (L > 2^20) and
the cap of 65535 tiles per block.  psa_set_segments refuses L = 1; that length runs without segments on T = 1.

Measured on one MI355X, worst ratio to the bound per axis (worst rel_max in brackets; the module prints this line):
    atoms 0.163 (1.3e-7)   groups 0.155 (1.4e-7)   lengths 0.174 (3.3e-7)   hops 0.077 (8.3e-8)   budgets 0.070 (1.1e-7)
    chunks 0.329 (3.8e-7)  families 0.060 (1.1e-7)  modes 0.051 (9.9e-8)
The largest, 0.329, is the line at L = 513 in the group of 5 atoms (the twin: 0.287 on the same case); one atom or one
pair on the line gives 0.16 .. 0.20, everything else is below 0.1.  Every budget case has the default budget's bits.
The tightened tests of tests/test_gpu_vdos.py lie at 0.037 .. 0.103.
"""
import numpy as np
import pytest

import vdos_cases as V
from conftest import rel_max
from engine_state import reset

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def worst(engine):
    """axis -> [worst ratio, worst rel_max]; printed when the module is done"""
    table = {}
    reset(engine)
    yield table
    reset(engine)
    for slot in (0, 1):
        engine.release(slot)
    engine.invalidate()
    print("\nworst ratio to the bound per axis: " +
          ", ".join(f"{axis} {r:.3f} ({e:.1e})" for axis, (r, e) in table.items()))


def _run(engine, inp, budget):
    from psa_amd import Segments, _hip
    disp = inp["mean"] is not None
    slot = _hip.SLOT_POSITIONS if disp else _hip.SLOT_VELOCITIES
    engine.ensure_resident(slot, inp["data"])
    engine.set_option(_hip.OPT_VDOS_WORK_BYTES, budget)
    engine.set_atom_weights(inp["weights"])
    engine.set_segments(None if inp["L"] is None else Segments(inp["L"], inp["H"], inp["window"]))
    try:
        groups = None if inp["groups"][0] is None else inp["groups"]
        return engine.vdos(slot, inp["mean"], groups, _hip.F_DISPLACEMENTS if disp else 0)
    finally:
        reset(engine)


def _check(engine, worst, axis, name):
    c, inp, ref, bar = V.reference(name)
    got = _run(engine, inp, inp["budget"])
    assert got.shape == ref.shape and got.dtype == np.float32, (got.shape, got.dtype, ref.shape)
    for gi, g in enumerate(inp["groups"]):
        if g is not None and len(g) == 0:
            assert not got[:, gi, :].any(), f"{name}: group {gi} is empty, its rows must be exactly zero"
    r, at = V.ratio(got, ref, bar)
    err = rel_max(got, ref)
    sizes = "all" if inp["groups"][0] is None else ",".join(str(len(g)) for g in inp["groups"])
    msg = (f"{name}: T={c['T']} N={c['N']} L={c['L']} H={c['H']} {c['window']} groups ({sizes}) budget {inp['budget']} -> "
           f"{got.shape}: {r:.3f} x bound at {at}, rel_max {err:.2e}")
    print(msg)
    w = worst.setdefault(axis, [0.0, 0.0])
    w[0], w[1] = max(w[0], r), max(w[1], err)
    assert np.all(np.isfinite(got)), msg
    assert r <= 1.0, msg
    return got, inp


def _names(axis):
    return [c["name"] for c in V.TABLES[axis]]


@pytest.mark.parametrize("name", _names("atoms"))
def test_atoms_of_one_group(engine, worst, name):
    """1 .. 129 atoms, listed unsorted and with atom N - 1: a lone atom, a lone pair, an odd last pair, the edges of the
    64-atom tile; all atoms of an odd and an even N as groups=None"""
    _check(engine, worst, "atoms", name)


@pytest.mark.parametrize("name", _names("groups"))
def test_group_layouts(engine, worst, name):
    """lone atoms, empty groups first, between and last, a tile with rows of seven groups, a group boundary on a tile
    boundary and one pair to either side"""
    _check(engine, worst, "groups", name)


@pytest.mark.parametrize("name", _names("lengths"))
def test_segment_lengths(engine, worst, name):
    """H = L around the 64-frame gather tile and the 256-bin stride of the power pass, odd, even and prime; runs without
    segments down to one frame"""
    _check(engine, worst, "lengths", name)


@pytest.mark.parametrize("name", _names("hops"))
def test_hops(engine, worst, name):
    """H = 1, overlap, none, gaps (frames no segment reads), two segments, frames left over after the last segment"""
    _check(engine, worst, "hops", name)


@pytest.mark.parametrize("name", _names("budgets"))
def test_budgets(engine, worst, name):
    """blocks of one tile x one segment, a ragged last segment block, two tiles per block with a group boundary inside
    the block, on a block's first pair and on its last: the float64 reference, and the default budget's bits"""
    got, inp = _check(engine, worst, "budgets", name)
    whole = _run(engine, inp, V.DEFAULT_BUDGET)
    assert np.array_equal(got.view(np.uint32), whole.view(np.uint32)), f"{name}: differs from the default budget's result"


@pytest.mark.parametrize("name", _names("chunks"))
def test_chunk_counts(engine, worst, name):
    """1, 21, 64 and 29 chunks of the power pass; in the last, groups with fewer rows than chunks"""
    _check(engine, worst, "chunks", name)


@pytest.mark.parametrize("name", _names("families"))
def test_families(engine, worst, name):
    got, inp = _check(engine, worst, "families", name)
    if inp["budget"] != V.DEFAULT_BUDGET:
        assert np.array_equal(got.view(np.uint32), _run(engine, inp, V.DEFAULT_BUDGET).view(np.uint32))


@pytest.mark.parametrize("name", _names("modes"))
def test_modes(engine, worst, name):
    """displacement mode and weights, together and apart, boxcar and hann"""
    _check(engine, worst, "modes", name)


def test_segments_of_one_frame_are_refused(engine, worst):
    """why the length axis starts at 2"""
    from psa_amd import _hip
    w = np.ones(1, np.float32)
    assert engine._lib.psa_set_segments(engine._h, 1, 1, w.ctypes.data_as(_hip._f32p)) == -1
    assert engine.segment_length == 0
