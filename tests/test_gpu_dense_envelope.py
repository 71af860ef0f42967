"""The dense projection kernels (k1_pair, k1_planes 32 / 64 / 128 rows, k1_planes_lw, k1_planes_wide, k1_split, k1_mfma,
k1_wave) against a float64 reference, element by element.

Before the FFT, through Engine.debug_project_only (it never takes the low-rank route).  The metric is gamma
(tests/ref64.py): the largest error of any output element q[k, c, t] in units of that element's own scale
B[c, t] = sum_a |w_a d[t, a, c]|, so a kernel that is wrong only where the output is small -- quiet frames, slow atoms,
the incoherent rows beside a coherent one -- cannot hide behind the global maximum.  Every case asserts
gamma <= bound(form, n_g), the bounds of tests/dense_cases.py: they are derived from DESIGN.md and k1_f16.h, not
measured.  tests/test_dense_envelope_host.py shows on the CPU that a kernel which loses the second piece of d on the
quiet frames exceeds them at least 5 x while it passes the older rel_max bars.

One axis at a time around K = 40, n_g = 1000, T = 96 on the quiet-frames input (rows, atoms, frames, frame ranges, index
lists), then every input family on every form.  Options select the forms; the planes forms also check that the group's
planes exist, the others that none do.  Which kernel instantiations really ran is in
profiles/dense_envelope_kernel_stats.csv (this file under rocprofv3 --kernel-trace --stats).  Each case prints form,
shape, gamma, gamma / bound, the worst row's relative error and rel_max.  Two end-to-end checks through Engine.calculate
close the file."""
import time

import numpy as np
import pytest

import dense_cases as D
from conftest import rel_max
from ref64 import gamma, intensity64, project64, row_rel, scale_B, sed64
from engine_state import reset

pytestmark = pytest.mark.gpu

ROWS = [1, 8, 16, 17, 32, 33, 64, 65, 127, 128, 129, 192, 256]
ATOMS = [1, 31, 32, 33, 255, 256, 257, 319, 320, 321, 641]
FRAMES = [1, 15, 16, 17, 63, 64, 65, 130]
# the k-list length a form takes at the base shape, and the lengths it can take at all
BASE_K = {"pair": 40, "planes32": 16, "planes64": 32, "planes128": 40, "planes_lw": 40, "planes_wide": 100, "bf16x3": 16,
          "mfma32": 40, "wave": 40}
PLANES = ("planes32", "planes64", "planes128", "planes_lw", "planes_wide")


def _wide(K):
    return K > 32 and ((2 * K + 127) // 128) % 2 == 0


CAN_TAKE = {"pair": lambda K: K >= 17, "planes32": lambda K: K <= 16, "planes64": lambda K: 17 <= K <= 32,
            "planes128": lambda K: K >= 33, "planes_lw": lambda K: K >= 33, "planes_wide": _wide,
            "bf16x3": lambda K: True, "mfma32": lambda K: True, "wave": lambda K: True}


def _select(engine, form, K):
    """the options that send a list of K k-vectors to the form"""
    from psa_amd import _hip
    assert CAN_TAKE[form](K), (form, K)
    planes = form in PLANES
    sel = {"mfma32": _hip.K1_MFMA32, "wave": _hip.K1_WAVE}.get(form, _hip.K1_AUTO)
    if form == "bf16x3" and K > 16:
        sel = _hip.K1_SPLIT_BF16
    engine.set_k1(sel)
    # a group's cached planes are taken before the selector is looked at: switching them off also empties the cache
    for opt, val in ((_hip.OPT_PLANES, int(planes)), (_hip.OPT_PLANES_EAGER, 1), (_hip.OPT_PLANES_MIN_K, 1),
                     (_hip.OPT_K1_WIDE, int(form == "planes_wide")), (_hip.OPT_K1_LOADER_WAVES, int(form == "planes_lw"))):
        engine.set_option(opt, val)


@pytest.fixture
def forced(engine):
    try:
        yield engine
    finally:
        reset(engine)
        for slot in (0, 1):
            engine.release(slot)
        engine.invalidate()


_CASES = {}                                 # the inputs and their float64 references, per shape


def _case(family="quiet_frames", K=None, n=None, T=None, idx=None):
    key = (family, K, n, T, None if idx is None else tuple(idx))
    if key not in _CASES:
        c = D.case(family, K=K, n=n, T=T)
        if idx is not None:
            c = D.with_idx(c, idx)
        args = (c["data"], c["r"])
        c["ref"] = project64(*args, c["k"], c["idx"], c["weights"], c["disp"])
        c["B"] = scale_B(*args, c["idx"], c["weights"], c["disp"])
        _CASES[key] = c
    return _CASES[key]


def _run(engine, form, c, frames=None):
    """the case's projection (K, 3, T) by the form"""
    from psa_amd import _hip
    K = len(c["k"])
    _select(engine, form, K)
    engine.set_atom_weights(c["weights"])
    slot = 1 if c["disp"] else 0
    engine.ensure_resident(slot, c["data"])
    got = engine.debug_project_only(slot, c["r"], c["k"], c["idx"], _hip.F_DISPLACEMENTS if c["disp"] else 0, frames)
    n_sets = engine.plane_cache()[0]
    assert (n_sets > 0) == (form in PLANES), f"{form}: {n_sets} plane sets cached"
    return got


def _check(form, c, got, frames=None, t0=None):
    K, T = got.shape[0], got.shape[2]
    ref, B = c["ref"], c["B"]
    tag = ""
    if frames is not None:
        lo, hi = frames[0], frames[0] + frames[1]
        outside = np.ones(T, bool)
        outside[lo:hi] = False
        assert not np.any(got[:, :, outside]), f"{form}: columns outside frames [{lo}, {hi}) are not zero"
        got, ref, B = got[:, :, lo:hi], ref[:, :, lo:hi], B[:, lo:hi]
        tag = f" frames [{lo}, {hi})"
    bound = D.bound(form, c["n_g"])
    g = gamma(got, ref, B)
    zero = not ref.any()
    rows = 0.0 if zero else float(row_rel(got.transpose(2, 0, 1), ref.transpose(2, 0, 1)).max())
    msg = (f"{form} {c['name']} K={K} n_g={c['n_g']}{'' if c['idx'] is None else ' (index list)'} N={c['data'].shape[1]} "
           f"T={T}{tag}: gamma {g:.3e} = {g / bound:.3f} x bound {bound:.2e}, worst row {rows:.2e}, "
           f"rel_max {0.0 if zero else rel_max(got, ref):.2e}" + (f", {time.perf_counter() - t0:.2f} s" if t0 else ""))
    print(msg)
    assert np.all(np.isfinite(got)), msg
    assert g <= bound, msg


def _forms_and_values(values, axis):
    out = []
    for form in D.FORMS:
        for v in values:
            if axis != "K" or CAN_TAKE[form](v):
                out.append((form, v))
    return out


# ---- rows: the edges of the 32-, 64-, 128- and 256-row blocks and of the even / odd rule of the wide form ------------
@pytest.mark.parametrize("form,K", _forms_and_values(ROWS, "K"))
def test_rows(forced, form, K):
    t0 = time.perf_counter()
    c = _case(K=K)
    _check(form, c, _run(forced, form, c), t0=t0)


# ---- atoms: stage (32), fold (8 x 32, 10 x 32) and wide-period (20 x 32) edges; most of them N % 4 != 0 ----------------
@pytest.mark.parametrize("form,n", _forms_and_values(ATOMS, "n"))
def test_atoms(forced, form, n):
    t0 = time.perf_counter()
    c = _case(K=BASE_K[form], n=n)
    _check(form, c, _run(forced, form, c), t0=t0)


# ---- frames: the edges of the 16-frame groups and the 64-frame tiles ---------------------------------------------------
@pytest.mark.parametrize("form,T", _forms_and_values(FRAMES, "T"))
def test_frames(forced, form, T):
    t0 = time.perf_counter()
    c = _case(K=BASE_K[form], T=T)
    _check(form, c, _run(forced, form, c), t0=t0)


# ---- frame ranges: the planes start on a 16-frame group (the ABI requires it), the others anywhere; ragged counts ------
def _ranges():
    return [(form, fr) for form in D.FORMS
            for fr in ([(16, 37), (64, 31)] if form in PLANES else [(16, 37), (5, 37), (33, 63)])]


@pytest.mark.parametrize("form,frames", _ranges(), ids=lambda v: v if isinstance(v, str) else f"{v[0]}+{v[1]}")
def test_frame_ranges(forced, form, frames):
    t0 = time.perf_counter()
    c = _case(K=BASE_K[form])
    _check(form, c, _run(forced, form, c, frames), frames, t0=t0)


def test_planes_refuse_a_range_inside_a_frame_group(forced):
    from psa_amd import _hip
    _select(forced, "planes128", 40)
    c = _case(K=40)
    forced.ensure_resident(0, c["data"])
    with pytest.raises(_hip.PsaHipError, match="groups of 16 frames"):
        forced.debug_project_only(0, c["r"], c["k"], None, 0, (5, 37))


# ---- index lists: the gather forms, duplicates counted twice ------------------------------------------------------------
def _dup_list(n_tot, n_g, seed):
    idx = np.random.default_rng(seed).integers(0, n_tot, n_g)
    idx[5] = idx[6] = idx[n_g - 1]
    return idx.tolist()


@pytest.mark.parametrize("n_g", [40, 333])
@pytest.mark.parametrize("form", D.FORMS)
def test_index_list_with_duplicates(forced, form, n_g):
    t0 = time.perf_counter()
    c = _case(K=BASE_K[form], idx=_dup_list(D.BASE["n"], n_g, 31))
    _check(form, c, _run(forced, form, c), t0=t0)


@pytest.mark.parametrize("form,K", [("pair", 24), ("pair", 50), ("bf16x3", 24), ("bf16x3", 50), ("mfma32", 8), ("mfma32", 24),
                                    ("mfma32", 50), ("mfma32", 140)])
def test_gather_forms_at_every_block_size(forced, form, K):
    """N % 4 != 0 and an index list, at the k-list lengths of each row block of the kernels that read the float32 array"""
    t0 = time.perf_counter()
    c = _case(K=K, n=321)
    _check(form, c, _run(forced, form, c), t0=t0)
    c = _case(K=K, idx=_dup_list(D.BASE["n"], 333, 32))
    _check(form, c, _run(forced, form, c), t0=t0)


# ---- every input family on every form at the base shape ----------------------------------------------------------------
@pytest.mark.parametrize("family", D.FAMILIES)
@pytest.mark.parametrize("form", D.FORMS)
def test_families(forced, form, family):
    t0 = time.perf_counter()
    c = _case(family, K=BASE_K[form])
    got = _run(forced, form, c)
    if family == "zeros":
        assert not got.any(), f"{form}: an all-zero array must give exactly zero"
    _check(form, c, got, t0=t0)


# ---- displacement mode on the float32 kernels' own loaders, at every row block ------------------------------------------
@pytest.mark.parametrize("K", [8, 24, 50, 140])
@pytest.mark.parametrize("form", ["mfma32", "wave"])
def test_displacements_subtracted_while_staging(forced, form, K):
    t0 = time.perf_counter()
    c = _case("displacements", K=K)
    _check(form, c, _run(forced, form, c), t0=t0)


# ---- end to end: Engine.calculate on k-lists that are not on one line, so that the dense kernels serve ------------------
TOL, TOL_ROW = 1e-6, 2e-6               # the low-rank suite's bars: global max-norm, worst k-row against its own maximum


def _check_e2e(name, got, ref, tol, tol_row, t0):
    err, rows = rel_max(got, ref), row_rel(got, ref)
    msg = (f"{name}: rel_max {err:.2e}, worst row {rows.max():.2e} (k {int(np.argmax(rows))}), "
           f"{time.perf_counter() - t0:.2f} s")
    print(msg)
    assert np.all(np.isfinite(got)), msg
    assert err <= tol and rows.max() <= tol_row, msg


@pytest.mark.parametrize("family", ["quiet_frames", "coherent"])
def test_calculate_complex(forced, family):
    t0 = time.perf_counter()
    c = D.case(family)
    forced.ensure_resident(0, c["data"])
    n0 = forced.lowrank_launches()
    got = forced.calculate(0, c["r"], c["k"])
    assert forced.lowrank_launches() == n0
    _check_e2e(f"complex {family}", got, sed64(c["data"], c["r"], c["k"]), TOL, TOL_ROW, t0)


@pytest.mark.parametrize("family", ["quiet_frames", "coherent"])
def test_calculate_incoherent_two_groups(forced, family):
    from psa_amd import _hip
    t0 = time.perf_counter()
    c = D.case(family)
    n = c["data"].shape[1]
    groups = [np.arange(0, n, 2, dtype=np.int32), np.arange(1, n, 2, dtype=np.int32)]
    forced.ensure_resident(0, c["data"])
    n0 = forced.lowrank_launches()
    got = forced.calculate(0, c["r"], c["k"], groups, _hip.F_INTENSITY)
    assert forced.lowrank_launches() == n0
    _check_e2e(f"incoherent {family}", got, intensity64(c["data"], c["r"], c["k"], groups), 2 * TOL, 2 * TOL_ROW, t0)
