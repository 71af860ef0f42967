"""The reciprocal-space families (dynamic, lattice, partial, self, correlation) work in one set of device buffers that a
call fills before it reads it (psa_ctx.h: d_rc_*).  So a call's result may not depend on what another family's larger call
left there: every public entry, in its per-vector and its shell form, and two debug companions give the bits they gave
before, whichever other family ran in between with more vectors, more bins, more atoms, more species and longer rows --
under the default budget and under one that leaves q a handful of vectors.  The kernels use no atomics, so identical calls
give identical bits and no case is left out."""
import numpy as np
import pytest

import lattice64 as L64
import lattice_cases as LC
import partial_cases as C
from engine_state import reset

pytestmark = pytest.mark.gpu

EDGES = np.array([0.05, 0.2, 0.45, 0.65, 0.85, 1.0, 1.15])
SMALL = 256 << 10       # bytes: 28 vectors of q with currents (8 KiB each), 14 of two species; one or two units of the self part


@pytest.fixture(autouse=True)
def _clean(engine):
    reset(engine)
    yield
    reset(engine)


@pytest.fixture(scope="module", autouse=True)
def _forget(engine):
    yield
    engine.invalidate()


@pytest.fixture(scope="module")
def wave():
    """T = 256, N = 130, the triclinic box, the half-space of |k| < 1.15 in 6 shells; the entries under test see the first 40
    vectors and 55 atoms in two species, the calls in between all vectors in 50 bins and all atoms in three species"""
    from psa_amd import commensurate_vectors, shell_bins
    box = LC.TRICLINIC
    inv = LC.inverse(box)
    half, _, q = commensurate_vectors(box, EDGES[-1], EDGES[0])
    b, sel, _, _ = shell_bins(q, EDGES)
    half, b = half[sel], b[sel]
    assert 100 <= half.shape[0] <= 300
    order = np.random.default_rng(7).permutation(130)
    pos, vel = C.lagged_wave(130, 256, box, half[np.flatnonzero(b == 2)[3]], 20, order[64:129].tolist(), 1.1)
    return dict(inv=inv, pos=pos, vel=vel, w=LC.weights("sqrt_mass", 130, seed=23),
                few=half[:40], few_bins=b[:40], two=[order[:30].tolist(), order[30:55].tolist()], some=order[:55],
                many=half, many_bins=(np.arange(half.shape[0]) % 50).astype(np.int32),
                three=[order[:64].tolist(), order[64:129].tolist(), order[129:].tolist()], everyone=order)


def _entries(engine, w):
    """name -> (family, call): the entries under test, Segments(64, 32): hann for the spectra, boxcar for the correlations"""
    from psa_amd import Segments
    inv, few, bins, two, some = w["inv"], w["few"], w["few_bins"], w["two"], w["some"]
    k_few = L64.lattice_k(few, inv)
    turns = np.linspace(-2.0, 2.0, 1001)

    def with_segments(window, call):
        def run():
            engine.set_segments(Segments(64, 32, window))
            return call()
        return run

    spectra = {
        "dynamic_spectra": ("dynamic", lambda: engine.dynamic_spectra(k_few, some, True)),
        "debug_dynamic_sincos": ("dynamic", lambda: engine.debug_dynamic_sincos(turns)),
        "lattice_spectra": ("lattice", lambda: engine.lattice_spectra(inv, few, None, 0, some, True)),
        "lattice_spectra shell": ("lattice", lambda: engine.lattice_spectra(inv, few, bins, 6, some, True)),
        "partial_spectra": ("partial", lambda: engine.partial_spectra(inv, few, two, None, 0, True)),
        "partial_spectra shell": ("partial", lambda: engine.partial_spectra(inv, few, two, bins, 6, True)),
        "debug_partial_project": ("partial", lambda: engine.debug_partial_project(inv, few, two, True)),
        "self_spectra": ("self", lambda: engine.self_spectra(inv, few, None, 0, some)),
        "self_spectra shell": ("self", lambda: engine.self_spectra(inv, few, bins, 6, some)),
    }
    correlations = {
        "lattice_correlations": ("correlation", lambda: engine.lattice_correlations(inv, few, 32, None, 0, some, True)),
        "lattice_correlations shell": ("correlation", lambda: engine.lattice_correlations(inv, few, 32, bins, 6, some, True)),
        "self_correlations": ("correlation", lambda: engine.self_correlations(inv, few, 32, None, 0, some)),
        "self_correlations shell": ("correlation", lambda: engine.self_correlations(inv, few, 32, bins, 6, some)),
    }
    out = {n: (f, with_segments("hann", c)) for n, (f, c) in spectra.items()}
    out.update({n: (f, with_segments("boxcar", c)) for n, (f, c) in correlations.items()})
    return out


def _larger(engine, w):
    """family -> a call of it, in both forms, that needs more of every shared buffer than any entry under test: all vectors,
    50 bins, all atoms listed, three species, currents, one segment of all 256 frames (the correlations: 512 padded)"""
    inv, many, bins, three, everyone = w["inv"], w["many"], w["many_bins"], w["three"], w["everyone"]
    k_many = L64.lattice_k(many, inv)

    def whole(*calls):
        def run():
            engine.set_segments(None)
            for call in calls:
                assert np.isfinite(call()).all()
        return run

    return {
        "dynamic": whole(lambda: engine.dynamic_spectra(k_many, everyone, True)),
        "lattice": whole(lambda: engine.lattice_spectra(inv, many, None, 0, everyone, True),
                         lambda: engine.lattice_spectra(inv, many, bins, 50, everyone, True)),
        "partial": whole(lambda: engine.partial_spectra(inv, many, three, None, 0, True),
                         lambda: engine.partial_spectra(inv, many, three, bins, 50, True)),
        "self": whole(lambda: engine.self_spectra(inv, many, None, 0, everyone),
                      lambda: engine.self_spectra(inv, many, bins, 50, everyone)),
        "correlation": whole(lambda: engine.lattice_correlations(inv, many, 256, None, 0, everyone, True),
                             lambda: engine.lattice_correlations(inv, many, 256, bins, 50, everyone, True),
                             lambda: engine.self_correlations(inv, many, 256, None, 0, everyone),
                             lambda: engine.self_correlations(inv, many, 256, bins, 50, everyone)),
    }


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype.itemsize == 8 else np.uint32)


@pytest.mark.parametrize("budget", [4 << 30, SMALL], ids=["default", "small"])
def test_another_familys_larger_call_leaves_no_trace(engine, wave, budget):
    from psa_amd import _hip
    engine.ensure_resident(_hip.SLOT_POSITIONS, wave["pos"])
    engine.ensure_resident(_hip.SLOT_VELOCITIES, wave["vel"])
    engine.set_atom_weights(wave["w"])
    entries, larger = _entries(engine, wave), _larger(engine, wave)

    def under_test(call):                                    # (the calls in between always get the whole budget)
        engine.set_option(_hip.OPT_DYNAMIC_WORK_BYTES, budget)
        try:
            return call()
        finally:
            engine.set_option(_hip.OPT_DYNAMIC_WORK_BYTES, 4 << 30)

    stale = []
    for name, (family, call) in entries.items():
        under_test(call)
        ref = under_test(call)                               # twice in a row: the second
        assert np.isfinite(ref).all() and ref.any(), name
        for other, pollute in larger.items():
            if other == family:
                continue
            pollute()
            got = under_test(call)
            if got.shape != ref.shape or not np.array_equal(_bits(got), _bits(ref)):
                stale.append((name, other))
    assert not stale, f"results that changed after another family's call: {stale}"
