"""No result depends on what the context's scratch memory held before the call.

psa_ctx owns some eighty grow-only device buffers that are never cleared, and the kernels read past what a call wrote,
by design.  Every case of tests/scratch_cases.py -- one entry-point call at the smallest ragged shape that reaches its
code path -- is held to four statements, bit for bit over every returned array, and finite wherever the first result is:

  a. repeat      r0 = call(); call() again equals r0
  b. poisoned    scratch_fill(0x00), call() equals r0; scratch_fill(0xFF) (a NaN in every float format), call() equals r0
  c. fresh       on a new context, armed with scratch_fill(0xFF) before anything is resident, call() equals r0: every
                 buffer and every plane set comes from the allocator filled with NaNs (one context per family)
  d. history     a loud larger call of the same case (257 atoms, 160 frames, longer lists, data x 2^20, another group
                 layout), then one call of every other entry family that shares device buffers with this one, then call()
                 equals r0 -- through the public API alone: the hook only ever puts zeros into index buffers, a
                 predecessor leaves valid-looking indices there

The module has a context of its own.  Every case prints its name, the buffers and bytes the hook filled, and "equal" or
the first element that differs.  What was found with it is in DESIGN.md (section "Scratch history")."""
import time

import pytest

import scratch_cases as S

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def own_engine():
    from psa_amd import _hip
    eng = _hip.Engine(0)
    yield eng
    eng.close()


_R0 = {}


def _first(engine, name):
    """r0 of the case, from the module's context, whatever ran on it before"""
    if name not in _R0:
        _R0[name] = S.CASES[name][1](engine)
    return _R0[name]


@pytest.mark.parametrize("name", list(S.CASES))
def test_repeat_poisoned_history(own_engine, name):
    t0 = time.perf_counter()
    family, call = S.CASES[name]
    eng = own_engine
    r0 = _first(eng, name)
    assert r0 and all(a.size for a in r0), f"{name}: the case returns nothing"
    # a.
    S.compare(name, "repeated", r0, call(eng))
    # b.
    S.check_poisoned(eng, name, call, r0)
    eng.scratch_fill(-1)
    # d.
    call(eng, loud=True)
    others = S.others_sharing(family)
    for other in others:
        S.CASES[S.HISTORY[other]][1](eng)
    S.compare(name, f"after a loud call and {len(others)} other families", r0, call(eng))
    print(f"{name}: {time.perf_counter() - t0:.2f} s")


@pytest.mark.parametrize("row", list(S.FRESH))
def test_fresh_armed_context(own_engine, row):
    """c.  r0 comes from the module's context, which is not armed"""
    from psa_amd import _hip
    t0 = time.perf_counter()
    names = [n for n, (family, _) in S.CASES.items() if family in S.FRESH[row]]
    wants = [_first(own_engine, n) for n in names]
    fresh = _hip.Engine(0)
    try:
        assert fresh.scratch_fill(0xFF) == (0, 0), "a new context holds no scratch buffer"
        before = _hip.device_buffers()
        for n, want in zip(names, wants):
            S.compare(n, "on a fresh context armed with 0xFF", want, S.CASES[n][1](fresh))
        assert _hip.device_buffers()[1] > before[1], "the fresh context allocated nothing"
        n_buf, n_bytes = fresh.scratch_fill(0xFF)
        print(f"{row}: {len(names)} cases, the context ends with {n_buf} real and index buffers of {n_bytes} bytes, "
              f"{time.perf_counter() - t0:.2f} s")
        assert n_buf > 0 and n_bytes > 0
    finally:
        fresh.close()


def test_the_hook_fills_what_it_says(own_engine):
    """scratch_fill reaches the device: the result resident before it is gone (finalize refuses as on a new context), the
    counts are those of the buffers the table calls real or index, and -1 disarms without filling"""
    from psa_amd import _hip
    eng = own_engine
    S.CASES["sed planes128 K=40 incoherent two groups"][1](eng)
    n_buf, n_bytes = eng.scratch_fill(0xFF)
    table = dict(_hip.scratch_table())
    assert 0 < n_buf <= sum(c != "state" for c in table.values())
    assert 0 < n_bytes <= _hip.device_buffers()[1]
    with pytest.raises(_hip.PsaHipError):
        eng.finalize(100, 40, True)
    with pytest.raises(_hip.PsaHipError):
        eng.result_intensity(100, 40)
    assert eng.scratch_fill(-1) == (0, 0)
