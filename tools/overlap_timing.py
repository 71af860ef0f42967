#!/usr/bin/env python3
"""The self-overlap at size (GPU box): N_g = 8 `--cells`^3 atoms x `--frames` frames generated in HBM, origin steps 1 and 16,
8 and 64 lags, in one process.  After `--warmup` calls, medians of `--runs` calls of the stage times (psa_last_timings:
unwrap, count kernel, reduce and moments, D2H) and of the call end to end (host clock).
  * The yardstick is the van Hove histogram kernel (msd_hist_kernel) in the same process on the same 8 lags, as
    tools/msd_timing.py runs it (n_r = 200) and with the one bin the identity uses (n_r = 1, dr = the cut-off): both
    kernels' samples per second side by side.  A sample is one (lag, origin, atom) unit.
  * The count kernel reads u64 at the origin once per run of eight lags, 24 (1 + 1/8) bytes per sample; its rate is
    also given against the 6.29 TB/s a float4 copy reaches.
    python tools/overlap_timing.py [--runs 5] [--warmup 2] [--out profiles/overlap_timing.json]"""
import argparse
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import numpy as np                                                       # noqa: E402
from psa_amd import _hip, synth                                          # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--cells", type=int, default=8)
ap.add_argument("--frames", type=int, default=65536)
ap.add_argument("--cutoff", type=float, default=0.05)
ap.add_argument("--runs", type=int, default=5)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--out", default=None)
args = ap.parse_args()
HBM_COPY = 6.29e12                       # the measured float4 copy rate (BASELINE.md "Ceilings")

eng = _hip.Engine(0)
spec = synth.SyntheticSpec((args.cells,) * 3, args.frames)
r0, types, box = synth.lattice(spec.cells)
synth.fill_device(eng, _hip.SLOT_POSITIONS, spec, synth.mode_tables(spec, r0))
H = np.asarray(box, np.float32).astype(np.float64)
T, N = spec.n_frames, spec.n_atoms
budget = 4 << 30
out = dict(device=eng.device_info()["name"], runs=args.runs, warmup=args.warmup, T=T, N=N, cutoff=args.cutoff, work_bytes=budget,
           hbm_copy_bytes_per_s=HBM_COPY)


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


def samples(lags, step):
    return float(N) * float(sum((T - 1 - t) // step + 1 for t in lags))


stages = dict(unwrap="gather", kernel="transpose", reduce="epilogue", d2h="d2h")
lags8 = [t for t in (1, 4, 16, 64, 256, 1024, 4096, 16384) if t < T]
lags64 = [t for t in (1 + 512 * i for i in range(64)) if t < T]
for step in (1, 16):
    for name, lags in (("8_lags", lags8), ("64_lags", lags64)):
        res = measure(lambda: eng.self_overlap(H, lags, args.cutoff, None, step), stages)
        n = samples(lags, step)
        res.update(lags=lags, samples=n, kernel_samples_per_s=n / (1e-3 * res["median_ms"]["kernel"]),
                   table_bytes=4 * len(lags) * ((T - 1 - min(lags)) // step + 1))
        res["kernel_bytes_per_s_at_27_bytes_a_sample"] = 27.0 * res["kernel_samples_per_s"]
        res["kernel_fraction_of_the_copy_rate"] = res["kernel_bytes_per_s_at_27_bytes_a_sample"] / HBM_COPY
        out[f"overlap_step_{step}_{name}"] = res
    res = measure(lambda: eng.self_overlap(H, lags8, args.cutoff, None, step, per_origin=True), stages)
    out[f"overlap_step_{step}_8_lags_with_the_table"] = res
    for name, dr, n_r in (("van_hove_8_lags_n_r_200", 0.01, 200), ("van_hove_8_lags_n_r_1", args.cutoff, 1)):
        res = measure(lambda: eng.van_hove_self(H, lags8, dr, n_r, None, step), stages)
        n = samples(lags8, step)
        res.update(lags=lags8, n_r=n_r, samples=n, kernel_samples_per_s=n / (1e-3 * res["median_ms"]["kernel"]))
        out[f"{name}_step_{step}"] = res
    out[f"count_over_histogram_rate_step_{step}"] = (out[f"overlap_step_{step}_8_lags"]["kernel_samples_per_s"]
                                                     / out[f"van_hove_8_lags_n_r_200_step_{step}"]["kernel_samples_per_s"])
sums = eng.self_overlap(H, lags8, args.cutoff, None, 1)[0]
out["identity_with_van_hove"] = bool(np.array_equal(sums[:, :, 0], eng.van_hove_self(H, lags8, args.cutoff, 1, None, 1)[:, :, 0]))
out["q_of_the_8_lags"] = [float(s) / (N * ((T - 1 - t) + 1)) for s, t in zip(sums[:, 0, 0], lags8)]
eng.close()
text = json.dumps(out, indent=1)
print(text)
if args.out:
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(text + "\n")
