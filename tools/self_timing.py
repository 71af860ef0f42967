#!/usr/bin/env python3
"""The self (incoherent) spectra at size (GPU box): one call of psa_self_spectra at N_g = 8 `--cells`^3 atoms generated in HBM
(psa_data_fill_synthetic into the positions slot), the `--vectors` shortest half-space vectors of the generated box in
`--bins` shells, `--frames` frames and Segments(`--L`, `--hop`, "hann").  After `--warmup` calls, medians of `--runs` calls,
in one process, of the stage times (psa_last_timings: series kernel, FFT, power pass and finish, D2H) and of the call end to
end (host clock), each stage set against its byte floor of the staged form at the HBM rate DESIGN section 3 uses (8 TB/s):
per unit (atom, vector, segment, frame of the segment) an 8-byte series store, a 16-byte FFT read and write, an 8-byte power
read.  Kernel times: run it under `rocprofv3 --kernel-trace --stats` in a run of its own (no counters in that run).
`--budget` sets PSA_OPT_DYNAMIC_WORK_BYTES: a budget that leaves one segment per block makes the series kernel evaluate a
frame once per segment that holds it, a larger one once per block -- the two ways to treat overlapping segments, side by side.
    python tools/self_timing.py [--cells 8] [--frames 65536] [--vectors 64] [--L 4096] [--hop 2048] [--runs 5] [--warmup 1]
                                [--per-vector] [--budget BYTES] [--out profiles/self_timing.json]"""
import argparse
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import numpy as np                                                       # noqa: E402
from psa_amd import Segments, _hip, commensurate_vectors, lattice, shell_bins, synth     # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--cells", type=int, default=8)
ap.add_argument("--frames", type=int, default=65536)
ap.add_argument("--L", type=int, default=4096)
ap.add_argument("--hop", type=int, default=2048)
ap.add_argument("--vectors", type=int, default=64)
ap.add_argument("--bins", type=int, default=8)
ap.add_argument("--runs", type=int, default=5)
ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--per-vector", action="store_true", help="the per-vector form instead of the shell form")
ap.add_argument("--budget", type=int, default=None, help="PSA_OPT_DYNAMIC_WORK_BYTES")
ap.add_argument("--out", default=None)
args = ap.parse_args()
HBM = 8e12

spec = synth.SyntheticSpec((args.cells,) * 3, args.frames)
r0, types, box = synth.lattice(spec.cells)
T, N = spec.n_frames, spec.n_atoms
inv = lattice.box_inverse(box)
q_max = 2 * np.pi / float(np.max(np.linalg.norm(np.asarray(box, np.float64), axis=1)))
while commensurate_vectors(box, q_max)[0].shape[0] < args.vectors:
    q_max *= 1.05
ind, _, q = commensurate_vectors(box, q_max)
ind, q = ind[:args.vectors], q[:args.vectors]
K = ind.shape[0]
edges = np.linspace(0.0, float(q.max()) * (1 + 1e-9), args.bins + 1)
bins = shell_bins(q, edges)[0]

eng = _hip.Engine(0)
synth.fill_device(eng, _hip.SLOT_POSITIONS, spec, synth.mode_tables(spec, r0))
seg = Segments(args.L, args.hop, "hann")
eng.set_segments(seg)
if args.budget:
    eng.set_option(_hip.OPT_DYNAMIC_WORK_BYTES, args.budget)
info = eng.device_info()


def call():
    return eng.self_spectra(inv, ind, None, 0, None) if args.per_vector else eng.self_spectra(inv, ind, bins, args.bins, None)


def one():
    eng.timings()
    t0 = time.perf_counter()
    res = call()
    ms = 1e3 * (time.perf_counter() - t0)
    st = eng.timings()
    return dict(e2e=ms, series=st["transpose"], fft=st["fft"], power=st["epilogue"], d2h=st["d2h"], h2d=st["h2d"]), res


for _ in range(args.warmup):
    one()
runs = []
for _ in range(args.runs):
    st, res = one()
    runs.append(st)
n_seg = seg.count(T)
units = float(N) * K * n_seg * seg.length
med = {key: float(np.median([r[key] for r in runs])) for key in runs[0]}
floor_ms = dict(series=1e3 * 8 * units / HBM, fft=1e3 * 16 * units / HBM, power=1e3 * 8 * units / HBM)
filled = res.any(axis=0)                                                 # (an empty shell is a column of zeros)
total = float(res.astype(np.float64).sum(0)[filled].mean())
out = dict(T=T, N=N, K=K, form="per_vector" if args.per_vector else "shell", n_bins=args.bins, L=seg.length, hop=seg.hop, n_seg=n_seg,
           runs=args.runs, warmup=args.warmup, work_budget_bytes=args.budget or (4 << 30), device=info["name"], units=units, hbm_rate_bytes_per_s=HBM,
           median_ms=med, min_ms={key: float(min(r[key] for r in runs)) for key in runs[0]},
           max_ms={key: float(max(r[key] for r in runs)) for key in runs[0]}, floor_ms=floor_ms,
           times_the_floor={key: med[key] / floor_ms[key] for key in floor_ms},
           achieved_bytes_per_s=dict(series=8 * units / (med["series"] * 1e-3), fft=16 * units / (med["fft"] * 1e-3),
                                     power=8 * units / (med["power"] * 1e-3)),
           mean_column_sum_over_N=total / N, columns_filled=int(filled.sum()))
eng.close()
text = json.dumps(out, indent=1)
print(text)
if args.out:
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(text + "\n")
