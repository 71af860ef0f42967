#!/usr/bin/env python3
"""The local-order call beside the bond-order call at size (GPU box), on the workload of tools/order_timing.py: 8 `cells`^3
atoms as one species at `--cells` 8 (4096 atoms) and 16 (32768 atoms) x `--frames` frames, placed uniformly at random in the
box of the synthetic lattice, uploaded once and resident in HBM before anything is timed; r_cut the radius that holds
`--neighbours` atoms at the mean density.  Both calls run in the same process on the same resident trajectory, alternating:
`Engine.local_order` with `--ls` (default 4 6), `--n-q` and `--n-w` bins -- what `calculate_local_order` runs --, with and
without the per-atom output, and `Engine.bond_order` with the same orders and `--n-q` bins.
After `--warmup` rounds, medians of `--runs` rounds of the stage times (psa_last_timings: fraction pass, neighbour pass, the
q_lm pass and the local-order pass -- the second is timed inside the span of both --, or the order pass, reduce, D2H) and of
each call end to end (host clock around a call that ends in a synchronise); per size the two new passes over the neighbour
pass and over the order pass.
    python tools/local_order_timing.py [--runs 5] [--warmup 2] [--out profiles/local_order_timing.json]"""
import argparse
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import numpy as np                                                       # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--cells", type=int, nargs="+", default=[8, 16])
ap.add_argument("--frames", type=int, default=16)
ap.add_argument("--ls", type=int, nargs="+", default=[4, 6])
ap.add_argument("--n-q", type=int, default=200)
ap.add_argument("--n-w", type=int, default=200)
ap.add_argument("--neighbours", type=float, default=12.0)
ap.add_argument("--runs", type=int, default=5)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--out", default=None)
args = ap.parse_args()


def summary(runs):
    return dict(median_ms={k: float(np.median([r[k] for r in runs])) for k in runs[0]},
                min_ms={k: float(min(r[k] for r in runs)) for k in runs[0]}, max_ms={k: float(max(r[k] for r in runs)) for k in runs[0]})


def measure_all():
    from psa_amd import _hip, local_order, synth
    eng = _hip.Engine(0)
    table = local_order.w3j_blocks(args.ls)
    res = dict(device=eng.device_info()["name"], runs=args.runs, warmup=args.warmup, frames=args.frames, ls=args.ls, n_q=args.n_q,
               n_w=args.n_w)
    for cells in args.cells:
        spec = synth.SyntheticSpec((cells,) * 3, args.frames)
        box = synth.lattice(spec.cells)[2]
        H = np.asarray(box, np.float32).astype(np.float64)
        n_atoms = spec.n_atoms
        pos = (np.random.default_rng(cells).uniform(0.0, 1.0, (args.frames, n_atoms, 3)) @ H).astype(np.float32)
        eng.ensure_resident(_hip.SLOT_POSITIONS, pos)
        r_cut = float((args.neighbours / n_atoms * abs(np.linalg.det(H)) * 3.0 / (4.0 * np.pi)) ** (1.0 / 3.0))
        kept = {}

        def timed(name, call, local):
            eng.timings()
            t0 = time.perf_counter()
            kept[name] = call()
            ms = 1e3 * (time.perf_counter() - t0)
            st = eng.timings()
            out = {"e2e": ms, "fractions": st["gather"], "neighbours": st["transpose"], "reduce": st["epilogue"], "d2h": st["d2h"]}
            if local:
                out.update(qlm=st["phase"] - st["project"], local=st["project"])
            else:
                out.update(order=st["phase"])
            return out

        def local_call(per_atom):
            return lambda: eng.local_order(H, r_cut, args.ls, args.n_q, args.n_w, table, None, 1, 0.2, args.ls[-1], 0.7, per_atom)
        calls = {"local_call": (local_call(False), True), "local_call_per_atom": (local_call(True), True),
                 "order_call": (lambda: eng.bond_order(H, r_cut, args.ls, args.n_q), False)}
        runs = {name: [] for name in calls}
        for i in range(args.warmup + args.runs):                          # the calls alternate: every round runs each once
            for name, (call, local) in calls.items():
                one = timed(name, call, local)
                if i >= args.warmup:
                    runs[name].append(one)
        out = {name: summary(r) for name, r in runs.items()}
        hist, qbar2, w, wbar, xi, n = kept["local_call_per_atom"]
        assert np.array_equal(kept["local_call"][0], hist)
        parts = local_order.split_row(hist, len(args.ls), args.n_q, args.n_w)
        lo, o = out["local_call"]["median_ms"], out["order_call"]["median_ms"]
        both = lo["qlm"] + lo["local"]
        kept_rows = xi >= 0
        res[f"{n_atoms}_atoms"] = dict(
            r_cut=r_cut, mean_neighbours=float(n.mean()), legs=float(n.astype(np.int64).sum()),
            left_out={k: int(parts[k][0]) for k in ("truncated", "isolated", "undefined", "incomplete")},
            mean_qbar={str(l): float(np.sqrt(qbar2[kept_rows][:, j]).mean()) for j, l in enumerate(args.ls)},
            mean_connections=float(xi[kept_rows].mean()), **out,
            qlm_pass_ns_per_leg=1e6 * lo["qlm"] / float(n.astype(np.int64).sum()), local_pass_ns_per_leg=1e6 * lo["local"] / float(n.astype(np.int64).sum()),
            two_passes_over_neighbour_pass=both / lo["neighbours"], two_passes_over_order_pass=both / o["order"],
            local_call_over_order_call=lo["e2e"] / o["e2e"], two_passes_share_of_call=both / lo["e2e"])
    eng.close()
    return res


text = json.dumps(measure_all(), indent=1)
print(text)
if args.out:
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(text + "\n")
