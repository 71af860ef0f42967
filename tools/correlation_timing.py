#!/usr/bin/env python3
"""The time correlations at size (GPU box), against their spectral twins on the same workloads, in one process:
  coherent   N = 32768 atoms x `--frames` frames generated in HBM, the half sphere that holds at least `--vectors` vectors in
             `--bins` shells, boxcar Segments(1024, 512): psa_lattice_correlations (shell form, lags = L // 2) against
             psa_lattice_spectra (shell form) -- the workload of tools/lattice_timing.py;
  self       N_g = 8 `--self-cells`^3 atoms x `--self-frames` frames, the `--self-vectors` shortest half-space vectors in 8
             shells, boxcar Segments(4096, 2048): psa_self_correlations against psa_self_spectra -- the workload of
             tools/self_timing.py.
After `--warmup` calls, medians of `--runs` calls of the stage times (psa_last_timings: projection or series kernel,
padding pass, FFT, power pass, back-transform, D2H) and of the call end to end (host clock); the back-transform's time
beside its P n_lags cols FMA count and the device's published vector float64 peak (78.6 TFLOP/s, half its float32 vector rate: 39.3e12 FMA/s).
    python tools/correlation_timing.py [--runs 5] [--warmup 2] [--only coherent|self] [--out profiles/correlation_timing.json]"""
import argparse
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import numpy as np                                                       # noqa: E402
from psa_amd import Segments, _hip, commensurate_vectors, lattice, shell_bins, synth     # noqa: E402
from psa_amd.correlations import padded_length                            # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=4096)
ap.add_argument("--vectors", type=int, default=5000)
ap.add_argument("--bins", type=int, default=16)
ap.add_argument("--self-cells", type=int, default=8)
ap.add_argument("--self-frames", type=int, default=65536)
ap.add_argument("--self-vectors", type=int, default=64)
ap.add_argument("--runs", type=int, default=5)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--only", choices=["coherent", "self"], default=None)
ap.add_argument("--out", default=None)
args = ap.parse_args()
FMA_RATE = 78.6e12 / 2

eng = _hip.Engine(0)
out = dict(device=eng.device_info()["name"], runs=args.runs, warmup=args.warmup, fp64_fma_per_s=FMA_RATE)


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


def back_transform(entry, P, n_lags, cols):
    fma = float(P) * n_lags * cols
    ms = entry["median_ms"]["back_transform"]
    entry["back_transform"] = dict(P=P, n_lags=n_lags, cols=cols, fma=fma, ms_at_the_fp64_rate=1e3 * fma / FMA_RATE, ms=ms,
                                   share_of_call=ms / entry["median_ms"]["e2e"])


if args.only != "self":
    spec = synth.SyntheticSpec((16, 16, 16), args.frames)
    r0, types, box = synth.lattice(spec.cells)
    inv = lattice.box_inverse(box)
    g = 2 * np.pi / float(np.max(np.linalg.norm(np.asarray(box, np.float64), axis=1)))
    q_max = g * (1.5 * args.vectors / np.pi) ** (1.0 / 3.0)
    while commensurate_vectors(box, q_max)[0].shape[0] < args.vectors:
        q_max *= 1.01
    ind, kv, q = commensurate_vectors(box, q_max)
    bins = shell_bins(q, np.linspace(0.0, q_max * (1 + 1e-9), args.bins + 1))[0]
    tables = synth.mode_tables(spec, r0)
    for slot in (_hip.SLOT_VELOCITIES, _hip.SLOT_POSITIONS):
        synth.fill_device(eng, slot, spec, tables)
    seg = Segments(1024, 512, "boxcar")
    eng.set_segments(seg)
    n_lags = seg.length // 2
    P = padded_length(seg.length, n_lags)
    cor = dict(projection="project", padding="gather", fft="fft", power="epilogue", back_transform="phase", d2h="d2h")
    spe = dict(projection="project", fft="fft", window_and_power="epilogue", d2h="d2h")
    res = dict(T=spec.n_frames, N=spec.n_atoms, K=int(ind.shape[0]), n_bins=args.bins, L=seg.length, hop=seg.hop,
               n_seg=seg.count(spec.n_frames), n_lags=n_lags, P=P,
               spectra_shell=measure(lambda: eng.lattice_spectra(inv, ind, bins, args.bins, None, True), spe),
               correlations_shell=measure(lambda: eng.lattice_correlations(inv, ind, n_lags, bins, args.bins, None, True), cor),
               correlations_per_vector=measure(lambda: eng.lattice_correlations(inv, ind, n_lags, None, 0, None, True), cor))
    back_transform(res["correlations_shell"], P, n_lags, 3 * args.bins)
    back_transform(res["correlations_per_vector"], P, n_lags, 3 * int(ind.shape[0]))
    res["correlations_over_spectra_e2e"] = res["correlations_shell"]["median_ms"]["e2e"] / res["spectra_shell"]["median_ms"]["e2e"]
    out["coherent"] = res
    eng.release(_hip.SLOT_VELOCITIES)
    eng.release(_hip.SLOT_POSITIONS)

if args.only != "coherent":
    spec = synth.SyntheticSpec((args.self_cells,) * 3, args.self_frames)
    r0, types, box = synth.lattice(spec.cells)
    inv = lattice.box_inverse(box)
    q_max = 2 * np.pi / float(np.max(np.linalg.norm(np.asarray(box, np.float64), axis=1)))
    while commensurate_vectors(box, q_max)[0].shape[0] < args.self_vectors:
        q_max *= 1.05
    ind, _, q = commensurate_vectors(box, q_max)
    ind, q = ind[:args.self_vectors], q[:args.self_vectors]
    bins = shell_bins(q, np.linspace(0.0, float(q.max()) * (1 + 1e-9), 9))[0]
    synth.fill_device(eng, _hip.SLOT_POSITIONS, spec, synth.mode_tables(spec, r0))
    seg = Segments(4096, 2048, "boxcar")
    eng.set_segments(seg)
    n_lags = seg.length // 2
    P = padded_length(seg.length, n_lags)
    cor = dict(series="transpose", padding="gather", fft="fft", power="epilogue", back_transform="phase", d2h="d2h")
    spe = dict(series="transpose", fft="fft", power="epilogue", d2h="d2h")
    res = dict(T=spec.n_frames, N=spec.n_atoms, K=int(ind.shape[0]), n_bins=8, L=seg.length, hop=seg.hop,
               n_seg=seg.count(spec.n_frames), n_lags=n_lags, P=P,
               spectra_shell=measure(lambda: eng.self_spectra(inv, ind, bins, 8, None), spe),
               correlations_shell=measure(lambda: eng.self_correlations(inv, ind, n_lags, bins, 8, None), cor))
    back_transform(res["correlations_shell"], P, n_lags, 8)
    a, b = res["correlations_shell"]["median_ms"], res["spectra_shell"]["median_ms"]
    res["correlations_over_spectra_e2e"] = a["e2e"] / b["e2e"]
    res["correlations_over_spectra_fft_and_power"] = (a["fft"] + a["power"] + a["padding"]) / (b["fft"] + b["power"])
    out["self"] = res

eng.close()
text = json.dumps(out, indent=1)
print(text)
if args.out:
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(text + "\n")
