#!/usr/bin/env python3
"""The displacement moments at size (GPU box): N_g = 8 `--cells`^3 atoms x `--frames` frames generated in HBM, `--lags` lags,
origin steps 1 and 16, in one process.  After `--warmup` calls, medians of `--runs` calls of the stage times
(psa_last_timings: unwrap, moments kernel, reduce and finish, D2H) and of the call end to end (host clock):
  * the moments kernel beside its count of (lag, origin, atom) units -- each three float32 subtractions, four products,
    two fmas, four conversions and four float64 adds -- and the device's published vector float64 add rate;
  * the unwrap pass (psa_debug_unwrap is not used: the stage time of the moments call) beside its HBM floor, one read of
    the positions touched and one write of u64 at the 6.29 TB/s a float4 copy reaches;
  * a van Hove call of 8 lags and psa_self_correlations on the same atoms (64 vectors, boxcar Segments(4096, 2048)), for
    scale, not as a bar.
    python tools/msd_timing.py [--runs 5] [--warmup 2] [--out profiles/msd_timing.json]"""
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
ap.add_argument("--lags", type=int, default=2048)
ap.add_argument("--runs", type=int, default=5)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--out", default=None)
args = ap.parse_args()
# the two ceilings, as the rest of the project quotes them (BASELINE.md "Ceilings", bench.py PEAK_*, tools/correlation_timing.py):
# the vector float64 rate is half the published 157.3 TFLOP/s of vector float32 and counts an fma as two operations, so
# 39.3e12 float64 adds per second; 6.29 TB/s is the measured float4 copy rate (79 % of the 8.0 TB/s HBM specification)
F64_ADD_RATE = 157.3e12 / 2 / 2
HBM_COPY = 6.29e12

eng = _hip.Engine(0)
spec = synth.SyntheticSpec((args.cells,) * 3, args.frames)
r0, types, box = synth.lattice(spec.cells)
synth.fill_device(eng, _hip.SLOT_POSITIONS, spec, synth.mode_tables(spec, r0))
H = np.asarray(box, np.float32).astype(np.float64)
T, N = spec.n_frames, spec.n_atoms
budget = 4 << 30
out = dict(device=eng.device_info()["name"], runs=args.runs, warmup=args.warmup, T=T, N=N, n_lags=args.lags,
           work_bytes=budget, atoms_per_block=int(min(N, budget // (24 * T))), fp64_add_per_s=F64_ADD_RATE, hbm_copy_bytes_per_s=HBM_COPY)


def measure(call, stages):
    def one():
        eng.timings()
        t0 = time.perf_counter()
        call()
        ms = 1e3 * (time.perf_counter() - t0)
        st = eng.timings()
        return dict(e2e=ms, **{name: st[key] for name, key in stages.items()})
    for _ in range(args.warmup):
        one()
    runs = [one() for _ in range(args.runs)]
    return dict(median_ms={k: float(np.median([r[k] for r in runs])) for k in runs[0]},
                min_ms={k: float(min(r[k] for r in runs)) for k in runs[0]},
                max_ms={k: float(max(r[k] for r in runs)) for k in runs[0]})


stages = dict(unwrap="gather", kernel="transpose", reduce_and_finish="epilogue", d2h="d2h")
for step in (1, 16):
    res = measure(lambda: eng.displacement_moments(H, args.lags, None, origin_step=step), stages)
    lags = np.arange(args.lags)
    units = float(N) * float(np.sum((T - 1 - lags) // step + 1))
    res["units"] = units
    res["kernel_ms_at_the_fp64_add_rate"] = 1e3 * 4.0 * units / F64_ADD_RATE
    res["kernel_units_per_s"] = units / (1e-3 * res["median_ms"]["kernel"])
    floor = (12.0 + 24.0) * N * T / HBM_COPY
    res["unwrap"] = dict(bytes_read_once=12.0 * N * T, bytes_written=24.0 * N * T, floor_ms=1e3 * floor,
                         ms=res["median_ms"]["unwrap"], over_floor=res["median_ms"]["unwrap"] / (1e3 * floor))
    out[f"moments_step_{step}"] = res
out["moments_no_unwrap"] = measure(lambda: eng.displacement_moments(H, args.lags, None, origin_step=16, unwrap=False), stages)

vh_lags = [1, 4, 16, 64, 256, 1024, 4096, 16384]
out["van_hove_8_lags"] = dict(lags=vh_lags, n_r=200, **measure(lambda: eng.van_hove_self(H, vh_lags, 0.01, 200, None), stages))

inv = lattice.box_inverse(box)
q_max = 2 * np.pi / float(np.max(np.linalg.norm(np.asarray(box, np.float64), axis=1)))
while commensurate_vectors(box, q_max)[0].shape[0] < 64:
    q_max *= 1.05
ind, _, q = commensurate_vectors(box, q_max)
ind, q = ind[:64], q[:64]
bins = shell_bins(q, np.linspace(0.0, float(q.max()) * (1 + 1e-9), 9))[0]
seg = Segments(4096, 2048, "boxcar")
eng.set_segments(seg)
cor = dict(series="transpose", padding="gather", fft="fft", power="epilogue", back_transform="phase", d2h="d2h")
out["self_correlations_for_scale"] = dict(K=64, n_bins=8, L=seg.length, hop=seg.hop, n_lags=seg.length // 2,
                                          **measure(lambda: eng.self_correlations(inv, ind, seg.length // 2, bins, 8, None), cor))
eng.close()
text = json.dumps(out, indent=1)
print(text)
if args.out:
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(text + "\n")
