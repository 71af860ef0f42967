#!/usr/bin/env python3
"""The solid-cluster call at size (GPU box), pass by pass, in the manner of tools/local_order_timing.py: `--cells` 8 (4096
atoms) and 16 (32768 atoms) x `--frames` frames of one species, uploaded once and resident in HBM before anything is timed.
Per size two configurations:
  liquid   the atoms placed uniformly at random in the box of the synthetic lattice, r_cut the radius that holds
           `--neighbours` atoms at the mean density, (`--liquid-threshold`, `--liquid-connections`): few small clusters;
  crystal  a perfect fcc crystal of the same number of atoms (8 x 8 x 16 or 16 x 16 x 32 cells of four), r_cut between the
           first and the second shell, the default criterion (0.7, 7): every atom solid, one cluster per frame -- every
           union of the hook pass ends at one root and every add of the flatten pass at one word, the contention worst case.
`Engine.solid_clusters` (link "neighbours", no per-atom output) alternates with `Engine.local_order` for the one order
`solid_l` and one bin -- the same fraction, neighbour and q_lm passes, which gives the q_lm pass alone.  After `--warmup`
rounds, medians of `--runs` rounds of the stage times (psa_last_timings): fraction pass, neighbour pass, the span of the q_lm,
bonds, hook and flatten passes, inside it the hook and the flatten pass, and the span of the species reduce, the stats pass and
its reduce.  Derived: bonds = span - hook - flatten - the q_lm pass of the local-order call; stats = the reduce span minus the
local-order call's reduce (a row of 76 words against 69).  The four cluster passes together over the neighbour pass of the
same call is the figure DESIGN quotes.
    python tools/cluster_timing.py [--runs 5] [--warmup 2] [--out profiles/cluster_timing.json]"""
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
ap.add_argument("--solid-l", type=int, default=6)
ap.add_argument("--neighbours", type=float, default=12.0)
ap.add_argument("--liquid-threshold", type=float, default=0.5)
ap.add_argument("--liquid-connections", type=int, default=3)
ap.add_argument("--n-sizes", type=int, default=256)
ap.add_argument("--runs", type=int, default=5)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--out", default=None)
args = ap.parse_args()


def summary(runs):
    return dict(median_ms={k: float(np.median([r[k] for r in runs])) for k in runs[0]},
                min_ms={k: float(min(r[k] for r in runs)) for k in runs[0]}, max_ms={k: float(max(r[k] for r in runs)) for k in runs[0]})


def fcc(cells, frames):
    """(positions (frames, 4 c c 2c, 3) float32, box): c x c x 2c cells of fcc, a = 4, frozen"""
    a, reps = 4.0, (cells, cells, 2 * cells)
    basis = np.array([[0, 0, 0], [0, .5, .5], [.5, 0, .5], [.5, .5, 0]])
    grid = np.stack(np.meshgrid(*[np.arange(k) for k in reps], indexing="ij"), -1).reshape(-1, 1, 3)
    pos = ((grid + basis[None]).reshape(-1, 3) * a).astype(np.float32)
    return np.ascontiguousarray(np.broadcast_to(pos, (frames,) + pos.shape)), np.diag(a * np.array(reps, np.float64)), 0.85 * a


def measure_all():
    from psa_amd import _hip, local_order, synth
    eng = _hip.Engine(0)
    table = local_order.w3j_blocks((args.solid_l,))
    res = dict(device=eng.device_info()["name"], runs=args.runs, warmup=args.warmup, frames=args.frames, solid_l=args.solid_l,
               n_sizes=args.n_sizes, link="neighbours")
    for cells in args.cells:
        spec = synth.SyntheticSpec((cells,) * 3, args.frames)
        H = np.asarray(synth.lattice(spec.cells)[2], np.float32).astype(np.float64)
        n_atoms = spec.n_atoms
        liquid = (np.random.default_rng(cells).uniform(0.0, 1.0, (args.frames, n_atoms, 3)) @ H).astype(np.float32)
        r_liquid = float((args.neighbours / n_atoms * abs(np.linalg.det(H)) * 3.0 / (4.0 * np.pi)) ** (1.0 / 3.0))
        crystal, H_fcc, r_fcc = fcc(cells, args.frames)
        assert crystal.shape[1] == n_atoms
        for name, pos, box, r_cut, thr, conn in (("liquid", liquid, H, r_liquid, args.liquid_threshold, args.liquid_connections),
                                                 ("crystal", crystal, H_fcc, r_fcc, 0.7, 7)):
            eng.ensure_resident(_hip.SLOT_POSITIONS, pos)
            kept = {}

            def timed(key, call, clusters):
                eng.timings()
                t0 = time.perf_counter()
                kept[key] = call()
                ms = 1e3 * (time.perf_counter() - t0)
                st = eng.timings()
                out = {"e2e": ms, "fractions": st["gather"], "neighbours": st["transpose"], "reduce_span": st["epilogue"], "d2h": st["d2h"]}
                if clusters:
                    out.update(passes_span=st["phase"], hook=st["project"], flatten=st["fft"])
                else:
                    out.update(qlm=st["phase"] - st["project"], local=st["project"])
                return out
            calls = {"cluster_call": (lambda: eng.solid_clusters(box, r_cut, args.solid_l, thr, conn, 0, args.n_sizes), True),
                     "local_call": (lambda: eng.local_order(box, r_cut, (args.solid_l,), 1, 1, table, None, 1, 0.2, args.solid_l, thr), False)}
            runs = {key: [] for key in calls}
            for i in range(args.warmup + args.runs):                      # the calls alternate: every round runs each once
                for key, (call, clusters) in calls.items():
                    one = timed(key, call, clusters)
                    if i >= args.warmup:
                        runs[key].append(one)
            out = {key: summary(r) for key, r in runs.items()}
            got = kept["cluster_call"]
            assert np.array_equal(got["species_rows"], kept["local_call"][0][:, 3:3 + 69])
            cl, lo = out["cluster_call"]["median_ms"], out["local_call"]["median_ms"]
            bonds = cl["passes_span"] - cl["hook"] - cl["flatten"] - lo["qlm"]
            stats = cl["reduce_span"] - lo["reduce_span"]
            four = bonds + cl["hook"] + cl["flatten"] + stats
            res[f"{n_atoms}_atoms_{name}"] = dict(
                r_cut=r_cut, solid_threshold=thr, min_connections=conn, mean_solid=float(got["n_solid"].mean()),
                mean_clusters=float(got["n_clusters"].mean()), mean_largest=float(got["largest"].mean()), **out,
                passes_median_ms=dict(qlm=lo["qlm"], bonds=bonds, hook=cl["hook"], flatten=cl["flatten"], stats=stats),
                four_cluster_passes_ms=four, four_cluster_passes_over_neighbour_pass=four / cl["neighbours"],
                hook_and_flatten_over_neighbour_pass=(cl["hook"] + cl["flatten"]) / cl["neighbours"],
                cluster_call_over_local_call=cl["e2e"] / lo["e2e"])
    eng.close()
    return res


text = json.dumps(measure_all(), indent=1)
print(text)
if args.out:
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(text + "\n")
