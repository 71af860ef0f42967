#!/usr/bin/env python3
"""The partial (species-resolved) spectra at size (GPU box), against code this path does not touch: N = 32768 atoms x
`--frames` frames generated in HBM (psa_data_fill_synthetic into both slots), Segments(1024, 512, "hann"), the half-sphere of
the generated box up to the |k| at which it holds at least `--vectors` vectors, in `--bins` shells, and S = 1, 2, 3 species
of equal size (atom a belongs to species a mod S).  Per S, after `--warmup` calls, medians of `--runs` calls, in one
process, of the stage times (psa_last_timings: projection, FFT, window and pair or shell pass, D2H) and of the call end to
end (host clock) of
  - psa_partial_spectra, shell form             one call, (3, P, L, n_bins) crosses to the host
  - psa_partial_spectra, per-vector form        one call, (3, P, L, K) crosses to the host
  - psa_lattice_spectra, shell form, S calls    the species one by one: the yardstick (the S diagonal pairs and nothing else)
The projection stage of the partial call runs the same kernel on the same lists, once per species, so it is expected to
equal the sum of the S calls' projection stages: `projection.inside_spread` says whether its median lies within the
min-max spread of that sum over the run.  The pair shell pass is set against S (S + 1) / 2 times the mean shell stage of the
one-species calls of the same run (stage 4 holds the window pass too, in both).  The bytes each form copies to the host are
reported with it.
    python tools/partial_timing.py [--frames 4096] [--vectors 5000] [--runs 10] [--warmup 3] [--density]
                                   [--out profiles/partial_timing.json]"""
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
ap.add_argument("--frames", type=int, default=4096)
ap.add_argument("--L", type=int, default=1024)
ap.add_argument("--hop", type=int, default=512)
ap.add_argument("--vectors", type=int, default=5000)
ap.add_argument("--bins", type=int, default=16)
ap.add_argument("--species", type=int, nargs="+", default=[1, 2, 3])
ap.add_argument("--runs", type=int, default=10)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--density", action="store_true", help="density only (no currents)")
ap.add_argument("--out", default=None)
args = ap.parse_args()
currents = not args.density
STAGES = ("e2e", "kernel", "fft", "window_pair_shell", "d2h")

spec = synth.SyntheticSpec((16, 16, 16), args.frames)
r0, types, box = synth.lattice(spec.cells)
T, N = spec.n_frames, spec.n_atoms
inv = lattice.box_inverse(box)
g = 2 * np.pi / float(np.max(np.linalg.norm(np.asarray(box, np.float64), axis=1)))
q_max = g * (1.5 * args.vectors / np.pi) ** (1.0 / 3.0)
while commensurate_vectors(box, q_max)[0].shape[0] < args.vectors:
    q_max *= 1.01
ind, kv, q = commensurate_vectors(box, q_max)
K = ind.shape[0]
edges = np.linspace(0.0, q_max * (1 + 1e-9), args.bins + 1)
bins, sel, avail, used = shell_bins(q, edges)
assert np.all(sel)

eng = _hip.Engine(0)
tables = synth.mode_tables(spec, r0)
for slot in (_hip.SLOT_VELOCITIES, _hip.SLOT_POSITIONS):
    synth.fill_device(eng, slot, spec, tables)
seg = Segments(args.L, args.hop, "hann")
eng.set_segments(seg)
rows = 3 if currents else 1


def one(calls):
    """the stage times of `calls`, one after the other, added up; the last result"""
    tot = dict.fromkeys(STAGES, 0.0)
    res = None
    for call in calls:
        eng.timings()
        t0 = time.perf_counter()
        res = call()
        ms = 1e3 * (time.perf_counter() - t0)
        st = eng.timings()
        for key, v in zip(STAGES, (ms, st["project"], st["fft"], st["epilogue"], st["d2h"])):
            tot[key] += v
    return tot, res


def measure(calls):
    for _ in range(args.warmup):
        one(calls)
    runs = []
    for _ in range(args.runs):
        st, res = one(calls)
        runs.append(st)
    med = {key: float(np.median([r[key] for r in runs])) for key in STAGES}
    return dict(median_ms=med, kernel_min_ms=float(min(r["kernel"] for r in runs)),
                kernel_max_ms=float(max(r["kernel"] for r in runs))), res


out = dict(T=T, N=N, K=K, q_max=q_max, n_bins=args.bins, L=seg.length, hop=seg.hop, n_seg=seg.count(T), currents=currents,
           runs=args.runs, warmup=args.warmup, device=eng.device_info()["name"], species={})
for S in args.species:
    P = S * (S + 1) // 2
    groups = [np.arange(a, N, S, dtype=np.int32) for a in range(S)]
    shell, res_shell = measure([lambda: eng.partial_spectra(inv, ind, groups, bins, args.bins, currents)])
    vector, _ = measure([lambda: eng.partial_spectra(inv, ind, groups, None, 0, currents)])
    singles, res_last = measure([(lambda g=g: eng.lattice_spectra(inv, ind, bins, args.bins, g, currents)) for g in groups])
    # the last species' diagonal pair is what the one-species call of that species gives
    diag = float(np.max(np.abs(res_shell[:, P - 1] - res_last)) / np.max(np.abs(res_last)))
    spread = singles["kernel_max_ms"] - singles["kernel_min_ms"]
    excess = shell["median_ms"]["kernel"] - singles["median_ms"]["kernel"]
    pass_yardstick = P * singles["median_ms"]["window_pair_shell"] / S
    out["species"][str(S)] = dict(
        pairs=P, atoms_per_species=[int(g.size) for g in groups], partial_shell=shell, partial_per_vector=vector,
        lattice_shell_species_one_by_one=singles,
        projection=dict(partial_ms=shell["median_ms"]["kernel"], sum_of_species_ms=singles["median_ms"]["kernel"],
                        excess_ms=excess, spread_of_sum_ms=spread, inside_spread=bool(abs(excess) <= spread)),
        shell_pass=dict(partial_ms=shell["median_ms"]["window_pair_shell"], pairs_times_one_species_ms=pass_yardstick,
                        ratio=shell["median_ms"]["window_pair_shell"] / pass_yardstick),
        d2h_bytes=dict(partial_shell=rows * P * seg.length * args.bins * 4, partial_per_vector=rows * P * seg.length * K * 4,
                       saved_by_the_shell_form=rows * P * seg.length * (K - args.bins) * 4),
        last_diagonal_pair_against_its_one_species_call_rel_max=diag)
eng.close()
text = json.dumps(out, indent=1)
print(text)
if args.out:
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(text + "\n")
