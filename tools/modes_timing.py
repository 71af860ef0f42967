#!/usr/bin/env python3
"""The mode-projected SED at size (GPU box): configuration 3's trajectory generated in HBM, k-path [1,1,0] with 256
vectors, the 8 silicon sites as groups, M = 24 random unitary mode vectors per k-point, sqrt(m) weights.  After
warm-up, medians of `--runs` calls of
  (a) the stage times (psa_last_timings) of psa_sed_modes: projection, FFT, the contraction kernel, D2H -- the kernel
      against both of its floors, bytes / 8 TB/s and flop / 157 TF;
  (b) SEDCalculator.calculate_mode_sed() end to end (host clock), against the only way to the same array without it:
      one `calculate(basis_atom_indices=site b)` per site plus np.abs(np.einsum(...))**2 on the host.  The B complex
      results are fetched in full; the einsum is timed on `--contract-frames` of the T frames and scaled to T (it is
      linear in T), which the output states;
  (c) the incoherent `calculate` of the same 8 groups, which does the same projections and the same transforms;
  (d) with --peaks: SEDCalculator.calculate_mode_peaks() end to end without and with `return_sed`, the stage times of
      psa_sed_modes_fit (the two fit kernels are in the "epilogue" stage beside the contraction) and the statuses.
  (e) with --segments L,H (Hann window): the same for the Welch-averaged mode spectra beside the figures above, measured
      in the same process -- the stage times of psa_sed_modes_welch (window and contraction in the "epilogue" stage),
      calculate_mode_sed(segments=...) end to end and, with --peaks, calculate_mode_peaks(segments=...), the stage times of
      psa_sed_modes_welch_fit and the statuses; the contraction's floors are those of mode_power_kernel<MT, true>.
Kernel time of mode_power_kernel<MT, false> (no segments), mode_power_kernel<MT, true>, peak_find_kernel, peak_fit_kernel: run it under `rocprofv3
--kernel-trace --stats` (with --skip-baseline).
    python tools/modes_timing.py [--cfg C3] [--n-k 256] [--modes 24] [--runs 10] [--skip-baseline] [--peaks] [--segments L,H]"""
import argparse
import json
import sys
import time
import weakref
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import numpy as np                                                                   # noqa: E402
from psa_amd import SEDCalculator, Segments, Trajectory, _hip, mass_weights, site_groups, synth     # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--cfg", default="C3")
ap.add_argument("--n-k", type=int, default=256)
ap.add_argument("--modes", type=int, default=24)
ap.add_argument("--runs", type=int, default=10)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--contract-frames", type=int, default=2048)
ap.add_argument("--skip-baseline", action="store_true")
ap.add_argument("--peaks", action="store_true")
ap.add_argument("--segments", default=None, metavar="L,H", help="also measure the Welch average: segments of L frames, H apart, Hann")
args = ap.parse_args()
seg = Segments(*(int(v) for v in args.segments.split(",")), "hann") if args.segments else None

spec, req = synth.baseline_spec(args.cfg)
r0, types, box = synth.lattice(spec.cells)
T, N, K, M, B = spec.n_frames, spec.n_atoms, args.n_k, args.modes, 8
eng = _hip.Engine(0)
synth.fill_device(eng, 0, spec, synth.mode_tables(spec, r0))
stand = np.broadcast_to(np.float32(0), (T, N, 3))
pos = np.broadcast_to(r0, (T, N, 3))
traj = Trajectory(pos, stand, types, np.broadcast_to(np.float32(0), (T,)), box, np.diag(box).copy(), np.zeros(3, np.float32),
                  spec.dt_ps)
calc = SEDCalculator(traj, *spec.cells).attach(engine=eng)
eng.adopt(0, stand)
calc._mean_cache = (weakref.ref(pos), r0, _hip.Engine._fingerprint(pos))
mags, vecs = calc.get_k_path([1, 1, 0], 1.0, K)
groups = site_groups(np.arange(N) % B)
lists = [g.tolist() for g in groups]
w = mass_weights(types, {1: 28.0855, 2: 28.0855})
rng = np.random.default_rng(0)
z = rng.standard_normal((K, 3 * B, 3 * B)) + 1j * rng.standard_normal((K, 3 * B, 3 * B))
eig = np.ascontiguousarray(np.stack([np.linalg.qr(zk)[0] for zk in z])[:, :M].reshape(K, M, B, 3).astype(np.complex64))


def stages():
    """psa_last_timings of one psa_sed_modes call"""
    eng.set_atom_weights(w)
    try:
        eng.timings()
        t0 = time.perf_counter()
        eng.sed_modes(0, r0, vecs, groups, eig)
        call_ms = 1e3 * (time.perf_counter() - t0)
        return dict(eng.timings(), call=call_ms)                 # call: host clock around Engine.sed_modes
    finally:
        eng.set_atom_weights(None)


def stages_welch(fit=False):
    """psa_last_timings of one psa_sed_modes_welch call (fit: psa_sed_modes_welch_fit, the spectra left on the device)"""
    eng.set_atom_weights(w)
    eng.set_segments(seg)
    try:
        eng.timings()
        t0 = time.perf_counter()
        if fit:
            eng.sed_modes_welch_fit(0, r0, vecs, groups, eig, 1.0 / (seg.length * spec.dt_ps))
        else:
            eng.sed_modes_welch(0, r0, vecs, groups, eig)
        call_ms = 1e3 * (time.perf_counter() - t0)
        return dict(eng.timings(), call=call_ms)
    finally:
        eng.set_atom_weights(None)
        eng.set_segments(None)


def e2e_modes(segments=None):
    t0 = time.perf_counter()
    calc.calculate_mode_sed(mags, vecs, eig, groups, atom_weights=w, segments=segments)
    return 1e3 * (time.perf_counter() - t0)


def e2e_peaks(return_sed=False, segments=None):
    t0 = time.perf_counter()
    calc.calculate_mode_peaks(mags, vecs, eig, groups, atom_weights=w, return_sed=return_sed, segments=segments)
    return 1e3 * (time.perf_counter() - t0)


def stages_peaks():
    """psa_last_timings of one psa_sed_modes_fit call that leaves the spectra on the device"""
    eng.set_atom_weights(w)
    try:
        eng.timings()
        t0 = time.perf_counter()
        eng.sed_modes_fit(0, r0, vecs, groups, eig, 1.0 / (T * spec.dt_ps))
        call_ms = 1e3 * (time.perf_counter() - t0)
        return dict(eng.timings(), call=call_ms)
    finally:
        eng.set_atom_weights(None)


def e2e_incoherent():
    t0 = time.perf_counter()
    calc.calculate(mags, vecs, basis_atom_indices=lists, summation_mode="incoherent", atom_weights=w)
    return 1e3 * (time.perf_counter() - t0)


def stages_incoherent():
    eng.timings()
    calc.calculate(mags, vecs, basis_atom_indices=lists, summation_mode="incoherent", atom_weights=w)
    return eng.timings()


def per_site_calls():
    """the B complex results on the host, as the public methods deliver them"""
    t0 = time.perf_counter()
    out = [calc.calculate(mags, vecs, basis_atom_indices=lists[b], atom_weights=w).sed for b in range(B)]
    return 1e3 * (time.perf_counter() - t0), out


def runs_of(fn):
    for _ in range(args.warmup):
        fn()
    return [fn() for _ in range(args.runs)]


def stats(v):
    return dict(median=float(np.median(v)), min=float(np.min(v)), max=float(np.max(v)))


kernel_bytes = 24 * B * T * K + 4 * T * K * M
kernel_flop = 8 * 3 * B * M * T * K
out = dict(cfg=args.cfg, T=T, N=N, K=K, B=B, M=M, runs=args.runs, warmup=args.warmup, kernel_bytes=kernel_bytes,
           kernel_flop=kernel_flop, floor_bytes_ms=kernel_bytes / 8e12 * 1e3, floor_flop_ms=kernel_flop / 157e12 * 1e3,
           result_bytes=4 * T * K * M, stacked_bytes=24 * B * T * K)
n0 = eng.lowrank_launches()
st = runs_of(stages)
out["lowrank_launches_per_call"] = (eng.lowrank_launches() - n0) / (args.warmup + args.runs)
out["stages_ms"] = {k: float(np.median([r[k] for r in st])) for k in ("h2d", "phase", "project", "fft", "epilogue", "d2h", "call")}
out["e2e_modes_ms"] = stats(runs_of(e2e_modes))
st = runs_of(stages_incoherent)
out["stages_incoherent_ms"] = {k: float(np.median([r[k] for r in st])) for k in ("h2d", "phase", "project", "fft", "epilogue",
                                                                                  "transpose", "d2h")}
out["e2e_incoherent_ms"] = stats(runs_of(e2e_incoherent))
if args.peaks:
    st = runs_of(stages_peaks)
    out["peaks_stages_ms"] = {k: float(np.median([r[k] for r in st])) for k in ("h2d", "phase", "project", "fft", "epilogue", "d2h",
                                                                               "call")}
    out["peaks_fit_kernels_ms"] = out["peaks_stages_ms"]["epilogue"] - out["stages_ms"]["epilogue"]
    out["e2e_peaks_ms"] = stats(runs_of(e2e_peaks))
    out["e2e_peaks_with_sed_ms"] = stats(runs_of(lambda: e2e_peaks(True)))
    out["e2e_modes_again_ms"] = stats(runs_of(e2e_modes))                 # the spectra alone once more, after the fit calls
    fit = calc.calculate_mode_peaks(mags, vecs, eig, groups, atom_weights=w)
    out["peaks_statuses"] = np.bincount(fit.status.ravel(), minlength=4).tolist()
    out["peaks_iterations"] = stats(fit.iterations.ravel())
    out["peaks_window_bins"] = stats(fit.window[..., 1] - fit.window[..., 0])
    out["peak_find_bytes"] = 4 * ((T + 1) // 2 - 1) * K * M
    out["peak_find_floor_ms"] = out["peak_find_bytes"] / 8e12 * 1e3
STAGES = ("h2d", "phase", "project", "fft", "epilogue", "d2h", "call")
if seg is not None:
    L, n_seg = seg.length, seg.count(T)
    wb, wf = 24 * B * K * n_seg * L + 4 * L * K * M, 8 * 3 * B * M * L * K * n_seg
    out["welch"] = dict(L=L, hop=seg.hop, n_seg=n_seg, window="hann", kernel_bytes=wb, kernel_flop=wf, floor_bytes_ms=wb / 8e12 * 1e3,
                        floor_flop_ms=wf / 157e12 * 1e3, result_bytes=4 * L * K * M, segment_data_over_q=n_seg * L / T)
    n0 = eng.lowrank_launches()
    st = runs_of(stages_welch)
    out["welch"]["lowrank_launches_per_call"] = (eng.lowrank_launches() - n0) / (args.warmup + args.runs)
    out["welch"]["stages_ms"] = {k: float(np.median([r[k] for r in st])) for k in STAGES}
    out["welch"]["e2e_modes_ms"] = stats(runs_of(lambda: e2e_modes(seg)))
    if args.peaks:
        st = runs_of(lambda: stages_welch(True))
        out["welch"]["peaks_stages_ms"] = {k: float(np.median([r[k] for r in st])) for k in STAGES}
        out["welch"]["e2e_peaks_ms"] = stats(runs_of(lambda: e2e_peaks(False, seg)))
        out["welch"]["e2e_peaks_with_sed_ms"] = stats(runs_of(lambda: e2e_peaks(True, seg)))
        fit = calc.calculate_mode_peaks(mags, vecs, eig, groups, atom_weights=w, segments=seg)
        out["welch"]["peaks_statuses"] = np.bincount(fit.status.ravel(), minlength=4).tolist()
        out["welch"]["peaks_iterations"] = stats(fit.iterations.ravel())
        out["welch"]["peaks_window_bins"] = stats(fit.window[..., 1] - fit.window[..., 0])
    out["e2e_modes_after_welch_ms"] = stats(runs_of(e2e_modes))           # the unsegmented call once more, same process
if not args.skip_baseline:
    per_site_calls()                                                      # warm-up
    ms, spectra = zip(*[per_site_calls() for _ in range(3)])
    out["baseline_calls_ms"] = stats(ms)
    Tc = min(T, args.contract_frames)
    lo = min(max(0, T // 8 - Tc // 2), T - Tc)                            # a slice around the planted bin on this path (T // 8)
    S = np.stack([s[lo:lo + Tc] for s in spectra[-1]])                    # (B, Tc, K, 3)
    t0 = time.perf_counter()
    phi = np.abs(np.einsum("kmbc,btkc->tkm", np.conj(eig), S, optimize=True)) ** 2
    ms_c = 1e3 * (time.perf_counter() - t0)
    got = calc.calculate_mode_sed(mags, vecs, eig, groups, atom_weights=w).sed
    out["baseline_contract_frames"] = [lo, lo + Tc]
    out["baseline_contract_ms_measured"] = ms_c
    out["baseline_contract_ms_scaled_to_T"] = ms_c * T / Tc
    out["baseline_total_ms"] = out["baseline_calls_ms"]["median"] + ms_c * T / Tc
    # max-norm relative difference of the two routes on those frames, over the largest value of the whole result
    out["baseline_agreement_rel_max"] = float(np.max(np.abs(got[lo:lo + Tc] - phi)) / np.max(got))
    out["slice_holds_the_maximum"] = bool(np.max(got[lo:lo + Tc]) == np.max(got))
print(json.dumps(out))
eng.close()
