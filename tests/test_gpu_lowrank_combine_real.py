"""The real-weights combine of the low-rank k-path route (lowrank_combine_r_kernel) on shapes where its staging can go
wrong: 96 atoms, T = 80 (shorter than a 256-frame block) and 300 (no multiple of it), K = 129 (odd, a last group of one
row out of four, a last 64-row stage of one row) and 256 (four stages), a path from +Gamma and one from -Gamma, one
case with per-atom weights; the route's minimums lowered through its options.

Each case holds the rows to the float64 reference within the bound of tests/test_gpu_lowrank_envelope.py (its _check,
TOL and TOL_ROW, imported), asserts that the launches took the route, and asserts that the list projected whole, as
halves in either order and cut at row 96 gives bit-identical complex rows.  The rows are those of Engine.project +
finalize, as in the envelope suite: Engine.debug_project_only never takes the low-rank route (api_debug.hip), so the
launch count could not go up with it."""
import time

import numpy as np
import pytest

from lowrank_cases import box, mass_weights, path
from test_gpu_lowrank_envelope import _check, _data, _project, _refs, forced  # noqa: F401  (forced: the fixture)

pytestmark = pytest.mark.gpu

N_ATOMS = 96
# (T, K, direction of the list away from Gamma, per-atom weights)
CASES = [(80, 129, +1, False), (80, 256, -1, False), (300, 129, -1, True), (300, 256, +1, False)]


def _case(T, K, sign, weighted):
    r = box(N_ATOMS, 40.0, 7, -20.0)
    k = path([sign, sign, 0], 0.0, 1.5, K)
    w = mass_weights(N_ATOMS, 8) if weighted else None
    return k, r, w, _data(T, N_ATOMS, 31)


@pytest.mark.parametrize("T,K,sign,weighted", CASES)
def test_real_weights_combine(forced, T, K, sign, weighted):
    t0 = time.perf_counter()
    k, r, w, x = _case(T, K, sign, weighted)
    forced.set_atom_weights(w)
    whole, n = _project(forced, x, r, k)
    _check(f"T={T}, K={K}, sign {sign:+d}" + (", weighted" if weighted else ""), whole, _refs(x, r, k, weights=w), n, t0=t0)
    cut = 96
    for parts in ([(0, K // 2), (K // 2, K)], [(K // 2, K), (0, K // 2)], [(0, cut), (cut, K)]):
        got, n = _project(forced, x, r, k, parts=parts)
        assert n == len(parts), parts
        assert np.array_equal(got.view(np.uint32), whole.view(np.uint32)), parts
