"""Per-atom weights without a GPU: `mass_weights`, the validation of `atom_weights`, the rule that the engine hears
of weights only when they are given (and is cleared afterwards, whatever happens), and two-rank `KShardGroup` runs in
modes "k" and "frames" against the single-process weighted oracle.  The engine is the CPU test double with weights."""
import socket
import sys
from pathlib import Path

import numpy as np
import pytest
import torch.multiprocessing as mp

HERE = Path(__file__).resolve().parent
for p in (str(HERE.parent), str(HERE), str(HERE / "golden")):
    if p not in sys.path:
        sys.path.insert(0, p)

from oracle_engine import OracleEngine          # noqa: E402
from psa_amd import _hip                         # noqa: E402


class WeightedOracleEngine(OracleEngine):
    """The oracle double with psa_set_atom_weights: velocity-mode projections see w[None, :, None] * v."""

    def __init__(self, *args, **kw):
        super().__init__(*args, **kw)
        self.weights, self.weight_calls = None, []

    def set_atom_weights(self, w):
        self.weight_calls.append(None if w is None else np.array(w))
        if w is not None:
            assert isinstance(w, np.ndarray) and w.dtype == np.float32 and w.ndim == 1 and w.flags.c_contiguous
        self.weights = w

    def _weighted(self, slot, flags, run):
        if self.weights is None:
            return run()
        assert not flags & _hip.F_DISPLACEMENTS, "the double weights velocity-mode projections only"
        data = self.slots[slot]
        assert data.shape[1] == len(self.weights), "weights of another atom count than the slot's"
        self.slots[slot] = data * self.weights[None, :, None]
        try:
            return run()
        finally:
            self.slots[slot] = data

    def project(self, slot, mean_pos_all, k_vectors, groups=None, flags=0, K_total=None, k_offset=0):
        return self._weighted(slot, flags, lambda: super(WeightedOracleEngine, self).project(
            slot, mean_pos_all, k_vectors, groups, flags, K_total, k_offset))

    def fs_project(self, slot, mean_pos_all, k_vectors, idx, flags, T_total, k_offset, k_count):
        return self._weighted(slot, flags, lambda: super(WeightedOracleEngine, self).fs_project(
            slot, mean_pos_all, k_vectors, idx, flags, T_total, k_offset, k_count))


def _golden(name="a"):
    import conftest
    with np.load(conftest.GOLDEN / f"traj_{name}.npz") as z:
        d = {k: z[k] for k in z.files}
    d["dt_ps"], d["cells"] = float(d["dt_ps"]), tuple(int(v) for v in d["cells"])
    return d


def _weights(n):
    w = np.random.default_rng(5).uniform(-2.0, 20.0, n).astype(np.float32)
    w[::7] = 0.0
    return w


def _weighted_oracle(d, vecs, w, **kw):
    from oracle import psa_oracle as O
    v = d["velocities"] * np.asarray(w, np.float32)[None, :, None]
    return O.calculate(d["positions"], v, d["types"], d["dt_ps"], vecs, **kw)[0]


# ---------------------------------------------------------------------------------------------------------------------
def test_mass_weights():
    from psa_amd import mass_weights
    w = mass_weights(np.array([1, 2, 2, 1, 3]), {1: 1.0, 2: 207.0, 3: 16.0, 9: 5.0})
    assert w.dtype == np.float32 and w.shape == (5,)
    np.testing.assert_array_equal(w, np.float32([1.0, np.sqrt(207.0), np.sqrt(207.0), 1.0, 4.0]))
    assert mass_weights(np.array([], int), {}).shape == (0,)
    with pytest.raises(ValueError, match="type 2"):
        mass_weights(np.array([1, 2]), {1: 12.0})
    with pytest.raises(ValueError):
        mass_weights(np.array([1]), {1: -1.0})


def test_atom_weights_validation():
    import conftest
    d = _golden()
    calc = conftest.make_calculator(d).attach(engine=WeightedOracleEngine())
    mags, vecs = calc.get_k_path("x", 1.0, 4)
    N = calc.traj.n_atoms
    bad = np.ones(N, np.float32)
    bad[2] = np.inf
    for w in (np.ones(N - 1), np.ones((N, 1)), bad, np.full(N, np.nan), np.ones(N, np.complex64), np.full(N, 1e300)):
        with pytest.raises(ValueError):
            calc.calculate(mags, vecs, atom_weights=w)
    assert calc.engine.weight_calls == []                       # nothing reached the engine
    with pytest.raises(TypeError):                              # keyword only: positional drop-in calls are unaffected
        calc.calculate(mags, vecs, None, None, "coherent", None, 500, np.ones(N))


def test_engine_hears_of_weights_only_when_given():
    import conftest
    d = _golden()
    plain = conftest.make_calculator(d).attach(engine=OracleEngine())          # no set_atom_weights at all
    mags, vecs = plain.get_k_path("x", 1.0, 4)
    plain.calculate(mags, vecs)
    plain.calculate_kpath_sed("x", 1.0, 4)

    eng = WeightedOracleEngine()
    calc = conftest.make_calculator(d).attach(engine=eng)
    calc.calculate(mags, vecs)
    calc.calculate_kgrid_sed("xy", (-1, 1, -1, 1), 2, 2)
    assert eng.weight_calls == []
    w = _weights(calc.traj.n_atoms)
    calc.calculate(mags, vecs, atom_weights=w.astype(np.float64))
    assert len(eng.weight_calls) == 2 and eng.weight_calls[1] is None and eng.weights is None
    np.testing.assert_array_equal(eng.weight_calls[0], w)
    # composites pass the keyword on; the chiral phase comes from the weighted result
    for sed in (calc.calculate_kpath_sed("x", 1.0, 4, atom_weights=w),
                calc.calculate_kgrid_sed("xy", (-1, 1, -1, 1), 2, 2, atom_weights=w),
                calc.calculate_chiral_sed("x", 1.0, 4, atom_weights=w)):
        assert sed.sed is not None
    assert len(eng.weight_calls) == 8 and eng.weights is None
    # cleared even when the calculation fails
    eng.project = lambda *a, **k: (_ for _ in ()).throw(RuntimeError("device lost"))
    eng.calculate = eng.project
    with pytest.raises(RuntimeError):
        calc.calculate(mags, vecs, atom_weights=w)
    assert eng.weights is None and eng.weight_calls[-1] is None


@pytest.mark.parametrize("kw", [{}, dict(basis_atom_types=[1, 2, 3], summation_mode="incoherent")])
def test_weighted_calculate_equals_weighted_oracle(kw):
    import conftest
    from psa_amd import mass_weights
    d = _golden()
    calc = conftest.make_calculator(d).attach(engine=WeightedOracleEngine())
    mags, vecs = calc.get_k_path([1, 1, 0], 2.0, 7)
    for w in (_weights(calc.traj.n_atoms), mass_weights(d["types"], {1: 1.0, 2: 207.0, 3: 16.0})):
        got = calc.calculate(mags, vecs, atom_weights=w, **kw)
        assert conftest.rel_max(got.sed, _weighted_oracle(d, vecs, w, **kw)) <= 1e-6
    unweighted = calc.calculate(mags, vecs, **kw)
    from oracle import psa_oracle as O
    ref, _, _ = O.calculate(d["positions"], d["velocities"], d["types"], d["dt_ps"], vecs, **kw)
    assert conftest.rel_max(unweighted.sed, ref) <= 1e-6


# ---------------------------------------------------------------------------------------------------------------------
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _weighted_rank(rank, world, port, backend, mode, results):
    """One rank of a 2-process sharded weighted `calculate` (oracle double with weights)."""
    import os
    import conftest
    from psa_amd import dist as D

    if backend == "gloo":
        import torch.distributed as td
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
        td.init_process_group("gloo", rank=rank, world_size=world)
        ex = D.TorchExchange()
    else:
        ex = D.TcpExchange(rank, world, "127.0.0.1", port)

    class ExchangeEngine(WeightedOracleEngine):
        """slab rows and frame blocks travel through the host exchange ("RCCL" of the double)"""
        def gather(self, root, k_offsets, k_counts):
            lo, n = int(k_offsets[self.rank]), int(k_counts[self.rank])
            parts = ex.allgather(self._slab[lo:lo + n])
            if root < 0 or root == self.rank:
                for r, rows in enumerate(parts):
                    self._slab[int(k_offsets[r]):int(k_offsets[r] + k_counts[r])] = rows

        def fs_exchange(self, t_off, t_cnt, k_off, k_cnt):
            parts = ex.allgather(self._fs["q"])
            lo, n = int(k_off[self.rank]), int(k_cnt[self.rank])
            for r, q in enumerate(parts):
                self.fs_write(int(t_off[r]), np.asarray(q)[lo:lo + n])

    d = _golden()
    eng = ExchangeEngine(rank=rank)
    group = D.KShardGroup(eng, ex, gather="all", root=0, mode=mode)
    calc = conftest.make_calculator(d).attach(shard_group=group)
    mags, vecs = calc.get_k_path([1, 1, 0], 2.0, 7)
    w = _weights(calc.traj.n_atoms)
    out = {}
    for name, kw in (("coh", {}), ("inc", dict(basis_atom_types=[1, 2], summation_mode="incoherent"))):
        out[name] = np.array(calc.calculate(mags, vecs, atom_weights=w, **kw).sed)
    out["plain"] = np.array(calc.calculate(mags, vecs).sed)
    out["mode"] = group.last_mode
    out["frames"] = eng.slots[0].shape[0]
    out["cleared"] = eng.weights is None and eng.weight_calls[-1] is None and len(eng.weight_calls) == 4
    ex.barrier()
    results[rank] = out
    group.close()
    if backend == "gloo":
        import torch.distributed as td
        td.destroy_process_group()


@pytest.mark.parametrize("backend, mode", [("tcp", "k"), ("gloo", "frames")])
def test_two_rank_sharded_weighted_equals_single_process(backend, mode):
    import conftest
    from oracle import psa_oracle as O
    world, port = 2, _free_port()
    ctx = mp.get_context("spawn")
    with ctx.Manager() as mgr:
        results = mgr.dict()
        procs = [ctx.Process(target=_weighted_rank, args=(r, world, port, backend, mode, results)) for r in range(world)]
        for p in procs:
            p.start()
        for p in procs:
            p.join(120)
            assert p.exitcode == 0, f"rank exited with {p.exitcode}"
        res = {r: dict(results[r]) for r in range(world)}
    d = _golden()
    calc = conftest.make_calculator(d)
    _, vecs = calc.get_k_path([1, 1, 0], 2.0, 7)
    w = _weights(calc.traj.n_atoms)
    ref_c = _weighted_oracle(d, vecs, w)
    ref_i = _weighted_oracle(d, vecs, w, basis_atom_types=[1, 2], summation_mode="incoherent")
    ref_p, _, _ = O.calculate(d["positions"], d["velocities"], d["types"], d["dt_ps"], vecs)
    for rank in range(world):
        r = res[rank]
        assert r["mode"] == mode and r["cleared"]
        assert r["frames"] == (64 if mode == "frames" else 128)
        assert conftest.rel_max(r["coh"], ref_c) <= 2e-6
        assert conftest.rel_max(r["inc"], ref_i) <= 2e-6
        assert conftest.rel_max(r["plain"], ref_p) <= 2e-6
        assert conftest.rel_max(r["coh"], ref_p) > 1e-2                 # (the weights did something)
