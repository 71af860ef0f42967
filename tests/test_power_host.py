"""Host proof for tests/power_cases.py: the float32 twins of the power, shell, finish, self-power and reduce passes stay
inside every bar on every case, with plain and with fused multiply-adds; the exact items hold for them bit for bit; every
planted fault -- the transverse formula the kernels used before among them -- breaks an exact item or a bar.  Prints the
worst fraction of each bar.  No GPU."""
import numpy as np
import pytest

import power64 as R
import power_cases as P

ROWS = ("density", "longitudinal", "transverse")


@pytest.fixture(scope="module")
def refs():
    return P.references()


def _run(kind, c, args, fused=False, fault=None):
    if kind == "dynamic":
        return P.dynamic_model(*args, k_block=c["k_block"], seg_block=c["seg_block"], fused=fused, fault=fault)
    if kind == "shell":
        return P.shell_model(*args, k_block=c["k_block"], seg_block=c["seg_block"], fused=fused, fault=fault)
    return P.self_model(*args, c["mirror"], n_chunks=c["n_chunks"], atom_block=c["atom_block"], vec_block=c["vec_block"],
                        seg_block=c["seg_block"], fused=fused, fault=fault)


_worst = P.worst


@pytest.mark.parametrize("fused", [False, True], ids=["plain", "fused"])
@pytest.mark.parametrize("kind", ["dynamic", "shell", "self"])
def test_twins_inside_every_bar(refs, kind, fused):
    worst = {}
    for name, (c, args, ref, bars) in refs[kind].items():
        got = _run(kind, c, args, fused=fused)
        assert not np.isnan(got).any(), name                               # every element written
        for r, (f, at) in enumerate(_worst(got, ref, bars)):
            assert f <= 1.0, (kind, name, ROWS[r], f, at)
            if f > worst.get(ROWS[r], (0.0,))[0] or ROWS[r] not in worst:
                worst[ROWS[r]] = (f, name, at)
        if got.ndim == 3 and got.shape[0] == 3:
            assert (got[2] >= 0).all(), (kind, name)
    for row, (f, name, at) in worst.items():
        print(f"{kind} {'fused' if fused else 'plain'} {row}: worst fraction of the bar {f:.3f} ({name} at {at})")


def _exact_items(fused=False, fault=None, kinds=("dynamic", "shell", "self")):
    """(label, twin's result, the one right answer) of every exact item"""
    for L in P.EXACT_L:
        if "dynamic" in kinds:
            seg, k, scale = P.exact_dynamic(L)
            ref = R.dynamic64(seg, k, scale)["out"]
            assert np.array_equal(ref.astype(np.float32).astype(np.float64), ref)      # nothing to round
            for kb, sb in P.DYNAMIC_CUTS:
                yield f"dynamic L{L} cut {kb},{sb}", P.dynamic_model(seg, k, scale, kb, sb, fused, fault), ref.astype(np.float32)
            yield f"dynamic L{L} zero", P.dynamic_model(0 * seg, k, scale, 2, 3, fused, fault), np.zeros(ref.shape, np.float32)
        if "shell" in kinds:
            seg, k, bin_of, n_bins, norm = P.exact_shell(L)
            ref = R.shell64(seg, k, bin_of, n_bins, norm)["out"].astype(np.float32)
            assert not ref[:, :, [0, 3, 5]].any() and ref[:, :, [1, 2, 4]].all()     # the empty bins: rows of zeros
            for kb, sb in P.SHELL_CUTS:
                yield f"shell L{L} cut {kb},{sb}", P.shell_model(seg, k, bin_of, n_bins, norm, kb, sb, fused, fault), ref
            yield f"shell L{L} zero", P.shell_model(0 * seg, k, bin_of, n_bins, norm, 3, 3, fused, fault), np.zeros_like(ref)
        if "self" in kinds:
            for mirror in (True, False):
                work, grp, cols, scale = P.exact_self(L, mirror)
                ref = R.self64(work, grp, cols, scale, mirror).astype(np.float32)
                for cut in P.SELF_CUTS:
                    yield (f"self L{L} mirror {mirror} cut {cut}", P.self_model(work, grp, cols, scale, mirror, fused=fused, fault=fault, **cut),
                           ref)


@pytest.mark.parametrize("fused", [False, True], ids=["plain", "fused"])
def test_exact_items_hold_for_the_twins(fused):
    n = 0
    for label, got, ref in _exact_items(fused):
        assert np.array_equal(P.bits(got), P.bits(ref)), label
        n += 1
    assert n == 2 * (4 + 4 + 6)


def test_cells_are_distinct_and_no_cell_is_anothers_conjugate_or_negation():
    c = P.gaussian_cells((7, 4, 4, 64)).ravel()
    assert np.unique(c).size == c.size and np.abs(c.real).max() <= 512 and np.abs(c.imag).max() <= 512
    assert (c.real > 0).all() and (c.imag < 0).all()                       # conj and negation leave the quadrant
    assert np.array_equal(c.real, np.rint(c.real)) and np.array_equal(c.imag, np.rint(c.imag))
    assert (P.khat32(P.axis_vectors(8)) == np.sign(P.AXES)).all()          # k / |k| exactly a unit vector or zero


@pytest.mark.parametrize("fault", list(P.FAULTS))
def test_every_planted_fault_is_caught(refs, fault):
    caught = []
    for kind in P.FAULTS[fault]:
        for label, got, ref in _exact_items(fault=fault, kinds=(kind,)):
            if not np.array_equal(P.bits(got), P.bits(ref)):
                caught.append(label)
        for name, (c, args, ref, bars) in refs[kind].items():
            if max(c["L"], c.get("K", 0)) > 4096 or len(c.get("counts", ())) > 64:
                continue                                                   # the small cases are enough
            got = _run(kind, c, args, fault=fault)
            bad = any(f > 1.0 for f, _ in _worst(got, ref, bars))
            if got.ndim == 3 and got.shape[0] == 3 and (got[2] < 0).any():
                bad = True
            if bad:
                caught.append(f"{kind} {name}")
        assert any(x.startswith(kind) for x in caught), (fault, kind)
    print(f"{fault}: caught by {len(caught)} items, first {caught[0]}")


def test_parent_transverse_goes_negative_and_breaks_the_bar_where_the_transverse_part_is_small(refs):
    c, args, ref, bars = refs["dynamic"]["families_ns2"]
    old = P.dynamic_model(*args, fault="parent_transverse")
    new = P.dynamic_model(*args)
    fam = np.array([c["families"][i % len(c["families"])] for i in range(c["K"])])
    with np.errstate(divide="ignore", invalid="ignore"):
        f_old = np.abs(old[2] - ref["out"][2]) / bars[2]
    assert (old[2][:, fam == "long"] < 0).any() and (new[2] >= 0).all()
    for name in ("long", "1e-4"):
        assert f_old[:, fam == name].max() > 1.0, name
    assert P.fraction(new[2], ref["out"][2], bars[2])[0] <= 1.0
