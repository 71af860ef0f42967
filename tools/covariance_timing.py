#!/usr/bin/env python3
"""The spectral covariance at size (GPU box): configuration 3's trajectory generated in HBM, k-path [1,1,0] with 256
vectors, the 8 silicon sites as groups, sqrt(m) weights, two weight rows (the moments -2 and 0 of a velocity run).
After `--warmup` calls, medians of `--runs` calls of
  (a) the stage times (psa_last_timings) of psa_sed_covariance: projection, FFT, the two covariance kernels ("epilogue"),
      D2H -- the kernels against their byte floor, 24 B T K bytes read once at 8 TB/s, and their matrix-core floor
      (the fp32 MFMAs issued, padded tiles included, at 32 cycles each on 1024 SIMDs at 2.4 GHz);
  (b) in the same process, the stage times of psa_sed_modes with M = 24 random unitary vectors on the same inputs: the
      covariance reads the same stacked spectra and writes a megabyte where the contraction writes 4 T K M bytes, so
      its "epilogue" stage is held against that one;
  (c) SEDCalculator.calculate_mode_vectors() end to end (host clock, the eigensolver on the host included);
  (d) the route without the feature, as tools/modes_timing.py builds its baseline: one complex
      `calculate(basis_atom_indices=site b)` per site fetched in full, plus the NumPy einsum of the covariance on
      `--contract-frames` of the T frequencies scaled to T (it is linear in T), which the output states.
Without --child the tool starts `--processes` fresh processes of itself one after the other and writes their results as
a JSON list to `--out`.  Kernel times of covariance_kernel<NB> and covariance_finish_kernel: run a child under
`rocprofv3 --kernel-trace --stats` (with --skip-baseline).
    python tools/covariance_timing.py [--cfg C3] [--n-k 256] [--runs 10] [--processes 3] [--out profiles/covariance_C3_timing.json]"""
import argparse
import json
import subprocess
import sys
import time
import weakref
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

ap = argparse.ArgumentParser()
ap.add_argument("--cfg", default="C3")
ap.add_argument("--n-k", type=int, default=256)
ap.add_argument("--modes", type=int, default=24)
ap.add_argument("--runs", type=int, default=10)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--contract-frames", type=int, default=2048)
ap.add_argument("--skip-baseline", action="store_true")
ap.add_argument("--processes", type=int, default=3)
ap.add_argument("--out", default=None)
ap.add_argument("--child", action="store_true", help="measure in this process and print one JSON line")
args = ap.parse_args()

if not args.child:
    out_path = Path(args.out) if args.out else ROOT / "profiles" / f"covariance_{args.cfg}_timing.json"
    results = []
    for _ in range(args.processes):
        cmd = [sys.executable, __file__, "--child", "--cfg", args.cfg, "--n-k", str(args.n_k), "--modes", str(args.modes), "--runs",
               str(args.runs), "--warmup", str(args.warmup), "--contract-frames", str(args.contract_frames)]
        res = subprocess.run(cmd + (["--skip-baseline"] if args.skip_baseline else []), capture_output=True, text=True, check=True)
        results.append(json.loads(res.stdout.strip().splitlines()[-1]))
        print(json.dumps(results[-1]), flush=True)
    out_path.write_text(json.dumps(results) + "\n")
    sys.exit(0)

import numpy as np                                                                   # noqa: E402
from psa_amd import SEDCalculator, Trajectory, _hip, mass_weights, site_groups, spectral_weights, synth     # noqa: E402

spec, req = synth.baseline_spec(args.cfg)
r0, types, box = synth.lattice(spec.cells)
T, N, K, M, B = spec.n_frames, spec.n_atoms, args.n_k, args.modes, 8
n, n_w = 3 * B, 2
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
g = np.stack([spectral_weights(T, spec.dt_ps, -2), spectral_weights(T, spec.dt_ps, 0)])
rng = np.random.default_rng(0)
z = rng.standard_normal((K, n, n)) + 1j * rng.standard_normal((K, n, n))
eig = np.ascontiguousarray(np.stack([np.linalg.qr(zk)[0] for zk in z])[:, :M].reshape(K, M, B, 3).astype(np.complex64))
STAGES = ("h2d", "phase", "project", "fft", "epilogue", "d2h", "call")


def staged(run):
    """psa_last_timings of one engine call under the weights, and the host clock around it"""
    eng.set_atom_weights(w)
    try:
        eng.timings()
        t0 = time.perf_counter()
        run()
        call_ms = 1e3 * (time.perf_counter() - t0)
        return dict(eng.timings(), call=call_ms)
    finally:
        eng.set_atom_weights(None)


def e2e_vectors():
    t0 = time.perf_counter()
    calc.calculate_mode_vectors(mags, vecs, groups, atom_weights=w)
    return 1e3 * (time.perf_counter() - t0)


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


def medians(st):
    return {k: float(np.median([r[k] for r in st])) for k in STAGES}


nb = (n + 15) // 16
mfmas = 2 * (nb * (nb + 1) // 2) * 2 * n_w * (T // 4) * K            # two per tile pair, part, weight row and 4 frequencies
kernel_bytes = 24 * B * T * K
out = dict(cfg=args.cfg, T=T, N=N, K=K, B=B, n_w=n_w, M_modes=M, runs=args.runs, warmup=args.warmup, kernel_bytes=kernel_bytes,
           floor_bytes_ms=kernel_bytes / 8e12 * 1e3, mfma_instructions=mfmas, floor_mfma_ms=mfmas * 32 / 1024 / 2.4e9 * 1e3,
           result_bytes=16 * n_w * K * n * n, slab_bytes=4 * K * -(-T // _hip.COV_CHUNK) * 2 * (nb * (nb + 1) // 2) * 512)
out["stages_ms"] = medians(runs_of(lambda: staged(lambda: eng.sed_covariance(0, r0, vecs, groups, g))))
out["modes_stages_ms"] = medians(runs_of(lambda: staged(lambda: eng.sed_modes(0, r0, vecs, groups, eig))))
out["stages_again_ms"] = medians(runs_of(lambda: staged(lambda: eng.sed_covariance(0, r0, vecs, groups, g))))
out["epilogue_over_modes_epilogue"] = out["stages_ms"]["epilogue"] / out["modes_stages_ms"]["epilogue"]
out["e2e_mode_vectors_ms"] = stats(runs_of(e2e_vectors))
mv = calc.calculate_mode_vectors(mags, vecs, groups, atom_weights=w)
out["modes_ok"] = int(mv.ok.sum())
if not args.skip_baseline:
    per_site_calls()                                                      # warm-up
    ms, spectra = zip(*[per_site_calls() for _ in range(3)])
    out["baseline_calls_ms"] = stats(ms)
    Tc = min(T, args.contract_frames)
    lo = min(max(0, T // 8 - Tc // 2), T - Tc)                            # a slice around the planted bin on this path (T // 8)
    S = np.stack([s[lo:lo + Tc] for s in spectra[-1]]).transpose(2, 0, 3, 1).reshape(K, n, Tc)    # (B, Tc, K, 3) -> rows
    t0 = time.perf_counter()
    G = np.einsum("mt,kit,kjt->mkij", g[:, lo:lo + Tc].astype(np.float64), S, np.conj(S), optimize=True)
    ms_c = 1e3 * (time.perf_counter() - t0)
    gs = np.zeros_like(g)
    gs[:, lo:lo + Tc] = g[:, lo:lo + Tc]
    got = calc.calculate_spectral_covariance(mags, vecs, groups, atom_weights=w, freq_weights=gs)
    out["baseline_contract_frames"] = [lo, lo + Tc]
    out["baseline_contract_ms_measured"] = ms_c
    out["baseline_contract_ms_scaled_to_T"] = ms_c * T / Tc
    out["baseline_total_ms"] = out["baseline_calls_ms"]["median"] + ms_c * T / Tc
    # max-norm relative difference of the two routes on those frequencies, per weight row
    out["baseline_agreement_rel_max"] = [float(np.max(np.abs(got[m] - G[m])) / np.max(np.abs(got[m]))) for m in range(n_w)]
print(json.dumps(out))
eng.close()
