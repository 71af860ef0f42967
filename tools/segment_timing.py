#!/usr/bin/env python3
"""Segment-averaged (Welch) spectra against the full-length result (GPU box): configuration 3's trajectory generated in
HBM, its 256-vector k-path, coherent.  After warm-up, medians of `--runs` calls of
  - the stage times (psa_last_timings) of the library's intensity step (psa_sed_calculate with PSA_F_INTENSITY), with
    Segments(L, H, "hann") and without;
  - SEDCalculator.calculate() end to end, with segments and without (the latter plus `.intensity`).
Kernel times of segment_window / segment_power: run it under `rocprofv3 --kernel-trace --stats`.
    python tools/segment_timing.py [--cfg C3] [--L 4096] [--hop 2048] [--runs 10]"""
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
mags, vecs = calc.get_k_path(req["direction"], req["bz_coverage"], req["n_k"])
seg = Segments(args.L, args.hop, "hann")
K = len(vecs)


def stages(segments):
    """psa_last_timings of one intensity step (all atoms as one group, like the coherent calculator call)"""
    eng.set_segments(segments)
    try:
        eng.timings()
        eng.calculate(0, r0, vecs, None, _hip.F_INTENSITY)
        return eng.timings()
    finally:
        eng.set_segments(None)


def e2e(segments):
    t0 = time.perf_counter()
    s = calc.calculate(mags, vecs, segments=segments)
    if segments is None:
        s.intensity
    return 1e3 * (time.perf_counter() - t0)


def median_of(fn, *a):
    for _ in range(args.warmup):
        fn(*a)
    return [fn(*a) for _ in range(args.runs)]


out = dict(cfg=args.cfg, T=T, N=N, K=K, L=seg.length, hop=seg.hop, n_seg=seg.count(T), runs=args.runs)
for name, s in (("segmented", seg), ("full", None)):
    runs = median_of(stages, s)
    out[f"stages_{name}_ms"] = {k: float(np.median([r[k] for r in runs])) for k in runs[0]}
for name, s in (("segmented", seg), ("full", None)):
    runs = median_of(e2e, s)
    out[f"e2e_{name}_ms"] = dict(median=float(np.median(runs)), min=float(np.min(runs)), max=float(np.max(runs)))
# algorithmic bytes of the two segment kernels (tools for GB/s against the kernel times of a rocprofv3 run)
n_seg = seg.count(T)
out["segment_window_bytes"] = 2 * 3 * K * n_seg * seg.length * 8
out["segment_power_bytes"] = 3 * K * n_seg * seg.length * 8 + 4 * K * seg.length
print(json.dumps(out))
eng.close()
