#!/usr/bin/env python3
"""The bond-order call beside the bond-angle call at size (GPU box), on the workload of tools/angle_timing.py: 8 `cells`^3
atoms as one species at `--cells` 8 (4096 atoms) and 16 (32768 atoms) x `--frames` frames, placed uniformly at random in the
box of the synthetic lattice, uploaded once and resident in HBM before anything is timed; r_cut the radius that holds
`--neighbours` atoms at the mean density.  Both calls run in the same process on the same resident trajectory, alternating:
`Engine.bond_order` with `--ls` (default 4 6) and `--n-q` bins -- what `calculate_bond_order` runs --, with and without the
per-atom output, and `Engine.angle_histogram` with `--n-theta` bins -- what `calculate_bond_angles` runs.
After `--warmup` rounds, medians of `--runs` rounds of the stage times (psa_last_timings: fraction pass, neighbour pass,
order or angle pass, reduce, D2H) and of each call end to end (host clock around a call that ends in a synchronise); per
size the ratio of the order pass to the angle pass and to the neighbour pass, the pairs of legs the order pass walks and
its ns per pair.
    python tools/order_timing.py [--runs 5] [--warmup 2] [--out profiles/order_timing.json]"""
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
ap.add_argument("--n-theta", type=int, default=180)
ap.add_argument("--neighbours", type=float, default=12.0)
ap.add_argument("--runs", type=int, default=5)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--out", default=None)
args = ap.parse_args()


def summary(runs):
    return dict(median_ms={k: float(np.median([r[k] for r in runs])) for k in runs[0]},
                min_ms={k: float(min(r[k] for r in runs)) for k in runs[0]}, max_ms={k: float(max(r[k] for r in runs)) for k in runs[0]})


def measure_all():
    from psa_amd import _hip, synth
    eng = _hip.Engine(0)
    res = dict(device=eng.device_info()["name"], runs=args.runs, warmup=args.warmup, frames=args.frames, ls=args.ls, n_q=args.n_q,
               n_theta=args.n_theta)
    for cells in args.cells:
        spec = synth.SyntheticSpec((cells,) * 3, args.frames)
        box = synth.lattice(spec.cells)[2]
        H = np.asarray(box, np.float32).astype(np.float64)
        n_atoms = spec.n_atoms
        pos = (np.random.default_rng(cells).uniform(0.0, 1.0, (args.frames, n_atoms, 3)) @ H).astype(np.float32)
        eng.ensure_resident(_hip.SLOT_POSITIONS, pos)
        r_cut = float((args.neighbours / n_atoms * abs(np.linalg.det(H)) * 3.0 / (4.0 * np.pi)) ** (1.0 / 3.0))
        kept = {}

        def timed(name, call, pass_name):
            eng.timings()
            t0 = time.perf_counter()
            kept[name] = call()
            ms = 1e3 * (time.perf_counter() - t0)
            st = eng.timings()
            return {"e2e": ms, "fractions": st["gather"], "neighbours": st["transpose"], pass_name: st["phase"], "reduce": st["epilogue"],
                    "d2h": st["d2h"]}
        calls = {"order_call": (lambda: eng.bond_order(H, r_cut, args.ls, args.n_q), "order"),
                 "order_call_per_atom": (lambda: eng.bond_order(H, r_cut, args.ls, args.n_q, per_atom=True), "order"),
                 "angle_call": (lambda: eng.angle_histogram(H, r_cut, args.n_theta), "angles")}
        runs = {name: [] for name in calls}
        for i in range(args.warmup + args.runs):                          # the calls alternate: every round runs each once
            for name, (call, pass_name) in calls.items():
                one = timed(name, call, pass_name)
                if i >= args.warmup:
                    runs[name].append(one)
        out = {name: summary(r) for name, r in runs.items()}
        hist, trunc, iso, undef, x, n = kept["order_call_per_atom"]
        assert all(np.array_equal(a, b) for a, b in zip(kept["order_call"][:4], (hist, trunc, iso, undef)))
        pairs = float((n.astype(np.int64) * (n.astype(np.int64) - 1) // 2).sum())
        o, a = out["order_call"]["median_ms"], out["angle_call"]["median_ms"]
        q = np.sqrt(x[x[..., 0] >= 0] / (n[x[..., 0] >= 0][:, None].astype(np.float64) ** 2 * float(1 << _hip.ORDER_SHIFT)))
        res[f"{n_atoms}_atoms"] = dict(
            r_cut=r_cut, mean_neighbours=float(n.mean()), truncated=int(trunc[0]), isolated=int(iso[0]), undefined=int(undef[0]),
            mean_q={str(l): float(q[:, j].mean()) for j, l in enumerate(args.ls)}, leg_pairs=pairs, **out,
            order_pass_ns_per_leg_pair=1e6 * o["order"] / pairs, order_pass_over_angle_pass=o["order"] / a["angles"],
            order_pass_over_neighbour_pass=o["order"] / o["neighbours"], order_call_over_angle_call=o["e2e"] / a["e2e"],
            order_pass_share_of_call=o["order"] / o["e2e"])
    eng.close()
    return res


text = json.dumps(measure_all(), indent=1)
print(text)
if args.out:
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(text + "\n")
