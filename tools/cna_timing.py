#!/usr/bin/env python3
"""The common-neighbour call at size (GPU box): 32768 atoms x `--frames` frames of one species, every frame an origin, on the
two lattices of a dense metal with a thermal noise of `--noise` A (64 distinct frames, repeated; uploaded once and resident
before anything is timed):
  fcc   32 x 16 x 16 cells of 4 atoms, a = 4.05 A, r_cut between the first and the second shell: 12 neighbours an atom
  bcc   32 x 32 x 16 cells of 2 atoms, a = 2.87 A, r_cut = (1 + sqrt 2) / 2 a between the second and the third: 14 neighbours
with and without the per-atom outputs.  After `--warmup` calls, medians of `--runs` calls of the stage times of one call
(psa_last_timings) and of the call end to end (host clock):
  fractions   the fraction pass [5]                  neighbours  the neighbour pass [6]
  cna         the signature and the census pass [1]  census      of these the census pass [2]
  reduce      [4]                                    d2h         the accumulator and the per-atom rows [7]
Beside them what the new passes are measured against:
  * the neighbour pass of the same call (the signature pass tests n (n - 1) / 2 pairs a centre, the neighbour pass N);
  * the byte floor of the signature pass, 4 + 256 bytes per centre (the count, the tags) + 12 per bond (a neighbour's
    fractions) + 4 (the type), with the per-bond output 256 more, over `--copy-gbs`, the copy rate DESIGN records.
`rocprofv3 --kernel-trace --stats -- python tools/cna_timing.py --runs 1 --warmup 0` in a run of its own gives the kernels' own
times (profiles/cna_kernel_stats.csv).
    python tools/cna_timing.py [--runs 5] [--warmup 2] [--out profiles/cna_timing.json]"""
import argparse
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import numpy as np                                                       # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=64)
ap.add_argument("--noise", type=float, default=0.1)
ap.add_argument("--copy-gbs", type=float, default=6290.0)
ap.add_argument("--runs", type=int, default=5)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--out", default=None)
args = ap.parse_args()

LATTICES = {"fcc": ((32, 16, 16), 4.05, [[0, 0, 0], [0, .5, .5], [.5, 0, .5], [.5, .5, 0]], 0.5 * (2.0 ** -0.5 + 1.0)),
            "bcc": ((32, 32, 16), 2.87, [[0, 0, 0], [.5, .5, .5]], 0.5 * (1.0 + 2.0 ** 0.5))}


def lattice(name):
    """(sites (32768, 3) float64, box (3, 3) float64, r_cut) of a lattice"""
    reps, a, basis, cut = LATTICES[name]
    cell = np.stack(np.meshgrid(*[np.arange(k) for k in reps], indexing="ij"), -1).reshape(-1, 1, 3)
    return (cell + np.asarray(basis)[None]).reshape(-1, 3) * a, np.diag(np.asarray(reps, np.float64) * a), cut * a


def measure_all():
    from psa_amd import _hip
    eng = _hip.Engine(0)
    T = args.frames
    budget = dict((name, default) for _, name, default in _hip.option_table())["PSA_OPT_DYNAMIC_WORK_BYTES"]
    res = dict(device=eng.device_info()["name"], runs=args.runs, warmup=args.warmup, frames=T, origin_step=1, noise=args.noise,
               copy_gbs=args.copy_gbs)
    for name in LATTICES:
        r0, box, r_cut = lattice(name)
        rng = np.random.default_rng(len(name))
        some = (r0[None] + args.noise * rng.standard_normal((64,) + r0.shape)).astype(np.float32)
        eng.ensure_resident(_hip.SLOT_POSITIONS, np.ascontiguousarray(np.tile(some, (-(-T // 64), 1, 1))[:T]))
        H = np.asarray(box, np.float32).astype(np.float64)
        res[name] = dict(atoms=int(r0.shape[0]), r_cut=float(r_cut))
        for per_atom in (False, True):
            per_origin = (1040 + 8 + (256 if per_atom else 0)) * r0.shape[0]
            kept = {}

            def one():
                eng.timings()
                t0 = time.perf_counter()
                kept["out"] = eng.common_neighbours(H, r_cut, None, 1, per_atom=per_atom)
                ms = 1e3 * (time.perf_counter() - t0)
                st = eng.timings()
                return dict(e2e=ms, fractions=st["gather"], neighbours=st["transpose"], cna=st["phase"], census=st["project"],
                            reduce=st["epilogue"], d2h=st["d2h"])
            for _ in range(args.warmup):
                one()
            runs = [one() for _ in range(args.runs)]
            med = {k: float(np.median([r[k] for r in runs])) for k in runs[0]}
            got = kept["out"]
            bonds = int(got["signature_counts"].sum() + got["signature_outside"].sum())
            centres = T * r0.shape[0]
            floor_ms = 1e3 * ((4 + 256 + 4 + (256 if per_atom else 0)) * centres + 12 * bonds) / (args.copy_gbs * 1e9)
            res[name]["per_atom" if per_atom else "counts_only"] = dict(
                median_ms=med, min_ms={k: float(min(r[k] for r in runs)) for k in runs[0]}, max_ms={k: float(max(r[k] for r in runs)) for k in runs[0]},
                cna_over_neighbour_pass=med["cna"] / med["neighbours"], signature_byte_floor_ms=floor_ms,
                signature_over_byte_floor=(med["cna"] - med["census"]) / floor_ms, mean_neighbours=bonds / centres,
                origins_per_block_at_the_default_budget=int(min(T, budget // per_origin)),
                type_share={t: float(got["type_counts"][:, 0, i].sum()) / centres for i, t in enumerate(_hip.CNA_TYPES)},
                share_421=float(got["signature_counts"][0, 4, 2, 1]) / max(bonds, 1), share_666=float(got["signature_counts"][0, 6, 6, 6]) / max(bonds, 1),
                bonds_outside_the_table=int(got["signature_outside"].sum()), truncated=int(got["truncated"].sum()))
    eng.close()
    return res


text = json.dumps(measure_all(), indent=1)
print(text)
if args.out:
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(text + "\n")
