#!/usr/bin/env python3
"""The adaptive common-neighbour call at size (GPU box), beside the plain one in the same session: 32768 atoms x `--frames`
frames of one species, every frame an origin, on the two lattices of tools/cna_timing.py with a thermal noise of `--noise` A
(64 distinct frames, repeated; uploaded once and resident before anything is timed):
  fcc   32 x 16 x 16 cells of 4 atoms, a = 4.05 A; adaptive: candidates out to the third shell, r_cut = 1.3 a (42 an atom);
        plain: r_cut between the first and the second shell (12)
  bcc   32 x 32 x 16 cells of 2 atoms, a = 2.87 A; adaptive: out to the third shell, r_cut = 1.5 a (26); plain: (1 + sqrt 2) / 2 a (14)
with and without the per-atom outputs.  After `--warmup` calls, medians of `--runs` calls of the stage times of one call
(psa_last_timings) and of the call end to end (host clock):
  fractions   the fraction pass [5]                  neighbours  the neighbour pass [6]
  cna         the signature and the census pass [1]  census      of these the census pass [2]
  reduce      [4]                                    d2h         the accumulator and the per-atom rows [7]
The number recorded: the signature plus census time as a share of the same call's neighbour pass, for the adaptive call and
for the plain call.  Beside it the byte floor of the adaptive signature pass, 4 + 1024 bytes per centre (the count, the
candidates' legs) + 12 per member (its fractions) + 8 (type, cut-off), with the per-bond output 112 more, over `--copy-gbs`.
    python tools/acna_timing.py [--runs 5] [--warmup 2] [--out profiles/acna_timing.json]"""
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

# name: (cells, a, basis, the plain call's r_cut / a, the adaptive call's r_cut / a)
LATTICES = {"fcc": ((32, 16, 16), 4.05, [[0, 0, 0], [0, .5, .5], [.5, 0, .5], [.5, .5, 0]], 0.5 * (2.0 ** -0.5 + 1.0), 1.3),
            "bcc": ((32, 32, 16), 2.87, [[0, 0, 0], [.5, .5, .5]], 0.5 * (1.0 + 2.0 ** 0.5), 1.5)}


def lattice(name):
    """(sites (32768, 3) float64, box (3, 3) float64, the plain r_cut, the adaptive r_cut) of a lattice"""
    reps, a, basis, plain, wide = LATTICES[name]
    cell = np.stack(np.meshgrid(*[np.arange(k) for k in reps], indexing="ij"), -1).reshape(-1, 1, 3)
    return (cell + np.asarray(basis)[None]).reshape(-1, 3) * a, np.diag(np.asarray(reps, np.float64) * a), plain * a, wide * a


def measure_all():
    from psa_amd import _hip
    eng = _hip.Engine(0)
    T = args.frames
    res = dict(device=eng.device_info()["name"], runs=args.runs, warmup=args.warmup, frames=T, origin_step=1, noise=args.noise,
               copy_gbs=args.copy_gbs)
    for name in LATTICES:
        r0, box, plain_cut, wide_cut = lattice(name)
        rng = np.random.default_rng(len(name))
        some = (r0[None] + args.noise * rng.standard_normal((64,) + r0.shape)).astype(np.float32)
        eng.ensure_resident(_hip.SLOT_POSITIONS, np.ascontiguousarray(np.tile(some, (-(-T // 64), 1, 1))[:T]))
        H = np.asarray(box, np.float32).astype(np.float64)
        res[name] = dict(atoms=int(r0.shape[0]), r_cut_adaptive=float(wide_cut), r_cut_plain=float(plain_cut))
        centres = T * r0.shape[0]
        for kind, call, r_cut in (("adaptive", eng.adaptive_common_neighbours, wide_cut), ("plain", eng.common_neighbours, plain_cut)):
            for per_atom in (False, True):
                kept = {}

                def one():
                    eng.timings()
                    t0 = time.perf_counter()
                    kept["out"] = call(H, r_cut, None, 1, per_atom=per_atom)
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
                entry = dict(median_ms=med, min_ms={k: float(min(r[k] for r in runs)) for k in runs[0]},
                             max_ms={k: float(max(r[k] for r in runs)) for k in runs[0]}, cna_over_neighbour_pass=med["cna"] / med["neighbours"],
                             bonds_per_centre=bonds / centres,
                             type_share={t: float(got["type_counts"][:, 0, i].sum()) / centres for i, t in enumerate(_hip.CNA_TYPES)},
                             bonds_outside_the_table=int(got["signature_outside"].sum()), truncated=int(got["truncated"].sum()))
                if kind == "adaptive":
                    floor_ms = 1e3 * ((4 + 1024 + 8 + (112 if per_atom else 0)) * centres + 12 * bonds) / (args.copy_gbs * 1e9)
                    entry.update(signature_byte_floor_ms=floor_ms, signature_over_byte_floor=(med["cna"] - med["census"]) / floor_ms,
                                 short=int(got["short"].sum()))
                    if per_atom:
                        entry["mean_candidates"] = float(got["n"].mean())
                res[name][f"{kind}_{'per_atom' if per_atom else 'counts_only'}"] = entry
    eng.close()
    return res


text = json.dumps(measure_all(), indent=1)
print(text)
if args.out:
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(text + "\n")
