"""The D image of the low-rank route's 48-node pair launch (pd16_n48_index, k1_lowrank_n48.h; through
psa_lowrank_n48_image, host only): for M = 512 rows and 1, 2, 5 and 41 atom stages the index is a bijection onto its data
units, rows 0..159 land only in role A's units and rows 160..511 only in role B's, the padding stages of either part are
never indexed, a wavefront's row half and row tile sit where the kernel reads them (unit 2 mt + h), and the byte size is
the entry's."""
import numpy as np
import pytest

UNIT = 16 * 32                  # float16 elements of a one-KiB unit: 16 rows x 32 atoms
A_ROWS, A_MT, B_MT, PAD = 160, 5, 11, 4   # role A: 160 rows, 5 row tiles per row half; role B: 352 rows, 11; padding stages per part
A_UNITS, B_UNITS = 2 * A_MT, 2 * B_MT


@pytest.mark.parametrize("n_stage", [1, 2, 5, 41])
def test_n48_image(n_stage):
    from psa_amd import _hip
    index, nbytes = _hip.lowrank_n48_image(n_stage)
    assert index.shape == (512, 32 * n_stage)
    # the size: each part carries its stages and four more of padding; the same bytes as the other images of one D block
    a_part, b_part = (n_stage + PAD) * A_UNITS, (n_stage + PAD) * B_UNITS
    assert nbytes == (a_part + b_part) * UNIT * 2 == _hip.lowrank_fold_image(n_stage)[1] == _hip.lowrank_pair_image(n_stage)[1]
    # a bijection onto the data stages of the two parts: every element once, no padding unit ever
    flat = np.sort(index.ravel())
    assert flat[0] >= 0 and np.all(np.diff(flat) > 0), "two (row, atom) share an element"
    unit = index // UNIT
    a_units = np.arange(n_stage * A_UNITS)
    b_units = a_part + np.arange(n_stage * B_UNITS)
    want = (np.concatenate([a_units, b_units])[:, None] * UNIT + np.arange(UNIT)[None, :]).ravel()
    assert np.array_equal(flat, want), "the image is not exactly the data stages of role A's and role B's parts"
    pad_units = np.concatenate([np.arange(n_stage * A_UNITS, a_part), np.arange(a_part + n_stage * B_UNITS, a_part + b_part)])
    assert not np.isin(unit, pad_units).any(), "a padding stage is indexed"
    assert (int(flat[-1]) + 1) * 2 == nbytes - PAD * B_UNITS * UNIT * 2, "role B's padding stages end the image"
    # rows 0..159 only in role A's units, rows 160..511 only in role B's
    assert np.all(np.isin(unit[:A_ROWS], a_units)) and np.all(np.isin(unit[A_ROWS:], b_units))
    # one unit = 16 consecutive rows x the 32 atoms of one stage, at 2 mt + h of its stage: role A's row half h holds rows
    # [80 h, +80), role B's rows [160 + 176 h, +176)
    for m0 in range(0, 512, 16):
        for s in range(n_stage):
            u = np.unique(unit[m0:m0 + 16, 32 * s:32 * s + 32])
            assert u.size == 1, (m0, s)
            if m0 < A_ROWS:
                h, mt = divmod(m0 // 16, A_MT)
                assert u[0] == s * A_UNITS + 2 * mt + h, (m0, s, int(u[0]))
            else:
                h, mt = divmod((m0 - A_ROWS) // 16, B_MT)
                assert u[0] == a_part + s * B_UNITS + 2 * mt + h, (m0, s, int(u[0]))
    # inside a unit: row r at 32 r, the atoms' 16-byte slots permuted within the row
    inner = index[:16, :32] % UNIT
    assert np.array_equal(np.sort(inner, axis=1), 32 * np.arange(16)[:, None] + np.arange(32)[None, :])
