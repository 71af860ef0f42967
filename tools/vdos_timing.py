#!/usr/bin/env python3
"""The vibrational density of states at size (GPU box): configuration 3's trajectory generated in HBM, the two type
groups (partial DOS), full length and with Segments(L, H, "hann").  After warm-up, medians of `--runs` calls of
  - the stage times (psa_last_timings) of psa_vdos: gather, FFT, power, D2H;
  - SEDCalculator.calculate_vdos() end to end (host clock; the call ends in a device synchronise).
Kernel times of vdos_gather / vdos_power: run it under `rocprofv3 --kernel-trace --stats`; the algorithmic bytes to
divide by them are printed here.
    python tools/vdos_timing.py [--cfg C3] [--L 4096] [--hop 2048] [--runs 10]"""
import argparse
import json
import sys
import time
import weakref
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import numpy as np                                                       # noqa: E402
from psa_amd import SEDCalculator, Segments, Trajectory, _hip, synth     # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--cfg", default="C3")
ap.add_argument("--L", type=int, default=4096)
ap.add_argument("--hop", type=int, default=2048)
ap.add_argument("--runs", type=int, default=10)
ap.add_argument("--warmup", type=int, default=3)
args = ap.parse_args()

spec, req = synth.baseline_spec(args.cfg)
r0, types, box = synth.lattice(spec.cells)
T, N = spec.n_frames, spec.n_atoms
eng = _hip.Engine(0)
synth.fill_device(eng, 0, spec, synth.mode_tables(spec, r0))
stand = np.broadcast_to(np.float32(0), (T, N, 3))
pos = np.broadcast_to(r0, (T, N, 3))
traj = Trajectory(pos, stand, types, np.broadcast_to(np.float32(0), (T,)), box, np.diag(box).copy(), np.zeros(3, np.float32),
                  spec.dt_ps)
calc = SEDCalculator(traj, *spec.cells).attach(engine=eng)
eng.adopt(0, stand)
calc._mean_cache = (weakref.ref(pos), r0, _hip.Engine._fingerprint(pos))
kinds = [int(t) for t in np.unique(types)]
groups = [np.flatnonzero(types == t) for t in kinds]
seg = Segments(args.L, args.hop, "hann")


def stages(segments):
    """psa_last_timings of one psa_vdos call"""
    eng.set_segments(segments)
    try:
        eng.timings()
        eng.vdos(0, None, groups)
        return eng.timings()
    finally:
        eng.set_segments(None)


def e2e(segments):
    t0 = time.perf_counter()
    calc.calculate_vdos(basis_atom_types=kinds, segments=segments)
    return 1e3 * (time.perf_counter() - t0)


def median_of(fn, *a):
    for _ in range(args.warmup):
        fn(*a)
    return [fn(*a) for _ in range(args.runs)]


out = dict(cfg=args.cfg, T=T, N=N, groups=len(groups), L=seg.length, hop=seg.hop, n_seg=seg.count(T), runs=args.runs,
           one_pass_floor_ms=12.0 * N * T / 8e12 * 1e3)
for name, s in (("segmented", seg), ("full", None)):
    runs = median_of(stages, s)
    out[f"stages_{name}_ms"] = {k: float(np.median([r[k] for r in runs])) for k in ("transpose", "fft", "epilogue", "d2h")}
    runs = median_of(e2e, s)
    out[f"e2e_{name}_ms"] = dict(median=float(np.median(runs)), min=float(np.min(runs)), max=float(np.max(runs)))
    # algorithmic bytes per call: the gather reads 12 N T_used bytes (each frame of each segment) and writes as many
    # (two atoms per complex value); the power pass reads 8 bytes per complex bin
    n_seg, L = (seg.count(T), seg.length) if s is not None else (1, T)
    out[f"gather_bytes_{name}"] = 2 * 12 * N * n_seg * L
    out[f"power_bytes_{name}"] = 8 * 3 * ((N + 1) // 2) * n_seg * L
print(json.dumps(out))
eng.close()
