"""The D image of the low-rank route's pair launch (pd16_pair_index, k1_lowrank_pair.h; through psa_lowrank_pair_image, host
only): for M = 512 rows and 1, 2, 5 and 41 atom stages the index is a bijection onto its image, rows 0..63 land only in
role A's units and rows 64..511 only in role B's, and the byte size includes both parts' padding stages."""
import numpy as np
import pytest

UNIT = 16 * 32                  # float16 elements of a one-KiB unit: 16 rows x 32 atoms
A_UNITS, B_UNITS, PAD = 4, 28, 4   # units per stage of role A (64 rows) and role B (448 rows); padding stages per part


@pytest.mark.parametrize("n_stage", [1, 2, 5, 41])
def test_pair_image(n_stage):
    from psa_amd import _hip
    index, nbytes = _hip.lowrank_pair_image(n_stage)
    assert index.shape == (512, 32 * n_stage)
    # the size: each part carries its stages and four more of padding
    a_part, b_part = (n_stage + PAD) * A_UNITS, (n_stage + PAD) * B_UNITS
    assert nbytes == (a_part + b_part) * UNIT * 2
    # a bijection onto the image: every element once, and together exactly the data stages of the two parts
    flat = np.sort(index.ravel())
    assert flat[0] >= 0 and np.all(np.diff(flat) > 0), "two (row, atom) share an element"
    unit = index // UNIT
    a_units = np.arange(n_stage * A_UNITS)
    b_units = a_part + np.arange(n_stage * B_UNITS)
    want = (np.concatenate([a_units, b_units])[:, None] * UNIT + np.arange(UNIT)[None, :]).ravel()
    assert np.array_equal(flat, want), "the image is not exactly the data stages of role A's and role B's parts"
    assert (int(flat[-1]) + 1) * 2 == nbytes - PAD * B_UNITS * UNIT * 2, "role B's padding stages end the image"
    # rows 0..63 only in role A's units, rows 64..511 only in role B's
    assert np.all(np.isin(unit[:64], a_units)) and np.all(np.isin(unit[64:], b_units))
    # one unit = 16 consecutive rows x the 32 atoms of one stage; the stage's units follow each other
    for m0 in range(0, 512, 16):
        for s in range(n_stage):
            u = np.unique(unit[m0:m0 + 16, 32 * s:32 * s + 32])
            assert u.size == 1, (m0, s)
            first = s * A_UNITS if m0 < 64 else a_part + s * B_UNITS
            assert first <= u[0] < first + (A_UNITS if m0 < 64 else B_UNITS), (m0, s, int(u[0]))
