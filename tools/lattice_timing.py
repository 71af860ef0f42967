#!/usr/bin/env python3
"""The spectra on the box's reciprocal lattice at size (GPU box), against psa_dynamic_spectra on the same vectors: N = 32768
atoms x `--frames` frames generated in HBM (psa_data_fill_synthetic into both slots), Segments(1024, 512, "hann"), the
half-sphere of the generated box up to the |k| at which it holds at least `--vectors` vectors (2000 .. 8000), in
`--bins` shells.  After `--warmup` calls, medians of `--runs` calls, in one process, of the stage times
(psa_last_timings: kernel, FFT, window and power or shell pass, D2H) and of the call end to end (host clock) of
  - psa_lattice_spectra, shell form            (L, n_bins) crosses to the host
  - psa_lattice_spectra, per-vector form       (L, K) crosses to the host
  - psa_dynamic_spectra on float32(n.G)        the same vectors, rounded, through dynamic.hip
with the spread (min, max) of the kernel stage, the ratio of the two projection stages, the unit rates ((vector, atom,
frame) units per second), the bytes each form copies to the host, and the instruction mix of the accumulating block of
lattice_project_kernel from `make asm`'s build/lattice.s.  The condition this tool exists to check: the projection stage of
psa_lattice_spectra takes less than that of psa_dynamic_spectra by more than the spread of the repeated medians.
Kernel times: run it under `rocprofv3 --kernel-trace --stats` in a run of its own (no counters in that run).
    python tools/lattice_timing.py [--frames 4096] [--vectors 2000] [--runs 10] [--warmup 3] [--density]
                                   [--out profiles/lattice_timing.json]"""
import argparse
import json
import re
import sys
import time
from collections import Counter
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import numpy as np                                                       # noqa: E402
from psa_amd import Segments, _hip, commensurate_vectors, lattice, shell_bins, synth     # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=4096)
ap.add_argument("--L", type=int, default=1024)
ap.add_argument("--hop", type=int, default=512)
ap.add_argument("--vectors", type=int, default=2000)
ap.add_argument("--bins", type=int, default=16)
ap.add_argument("--runs", type=int, default=10)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--density", action="store_true", help="density only (no currents)")
ap.add_argument("--skip-dynamic", action="store_true", help="time the lattice paths alone (a kernel-stats run)")
ap.add_argument("--spot-check", type=int, default=0, help="vectors whose spectra are also formed in float64 on the host")
ap.add_argument("--out", default=None)
args = ap.parse_args()
currents = not args.density


def accumulate_block_mix(nc):
    """instruction mix of the block of lattice_project_kernel<nc> that gathers the factors and accumulates (the largest
    such block, should the compiler have unrolled it), per atom of two units, or None without the listing"""
    listing = ROOT / "psa_amd" / "csrc" / "build" / "lattice.s"
    if not listing.exists():
        return None
    asm = listing.read_text()
    name = re.findall(rf"^(_ZN\S*lattice_project_kernelILi{nc}E\S*):", asm, flags=re.M)[0]
    body = asm[asm.index(name + ":"):]
    body = body[:body.index("s_endpgm")]
    hot = [b for b in re.split(r"\n\.LBB\d+_\d+:", body) if b.count("ds_read_b64") >= 6 and "v_fmac_f32" in b]
    ops = [ln.split()[0] for ln in min(hot, key=len).splitlines() if ln.startswith("\t") and ln.split() and not ln.split()[0].startswith((".", ";"))]
    atoms = max(1, sum(op.startswith("ds_read_b64") for op in ops) // 6)
    mix = Counter("valu" if op.startswith("v_") else "lds" if op.startswith("ds_") else "scalar" for op in ops)
    return dict(atoms_in_block=atoms, units_per_atom=_hip.LAT_KS // _hip.LAT_THREADS,
                valu_per_unit=mix["valu"] / atoms / 2, lds_reads_per_unit=mix["lds"] / atoms / 2,
                scalar_per_unit=mix["scalar"] / atoms / 2, ops=dict(Counter(ops)))


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
assert 2000 <= K <= 8000 or args.vectors < 2000, K
edges = np.linspace(0.0, q_max * (1 + 1e-9), args.bins + 1)
bins, sel, avail, used = shell_bins(q, edges)
assert np.all(sel)
k32 = kv.astype(np.float32)

eng = _hip.Engine(0)
tables = synth.mode_tables(spec, r0)
for slot in (_hip.SLOT_VELOCITIES, _hip.SLOT_POSITIONS):
    synth.fill_device(eng, slot, spec, tables)
seg = Segments(args.L, args.hop, "hann")
eng.set_segments(seg)
info = eng.device_info()

PATHS = {
    "lattice_shell": lambda: eng.lattice_spectra(inv, ind, bins, args.bins, None, currents),
    "lattice_per_vector": lambda: eng.lattice_spectra(inv, ind, None, 0, None, currents),
    "dynamic": lambda: eng.dynamic_spectra(k32, None, currents),
}
if args.skip_dynamic:
    del PATHS["dynamic"]


def one(call):
    eng.timings()
    t0 = time.perf_counter()
    res = call()
    ms = 1e3 * (time.perf_counter() - t0)
    st = eng.timings()
    return dict(e2e=ms, kernel=st["project"], fft=st["fft"], window_power_shell=st["epilogue"], d2h=st["d2h"]), res


units = float(K) * N * T
rows = 3 if currents else 1
out = dict(T=T, N=N, K=K, q_max=q_max, n_bins=args.bins, L=seg.length, hop=seg.hop, n_seg=seg.count(T), currents=currents,
           runs=args.runs, warmup=args.warmup, device=info["name"], units=units, paths={},
           d2h_bytes=dict(lattice_shell=rows * seg.length * args.bins * 4, lattice_per_vector=rows * seg.length * K * 4,
                          dynamic=rows * seg.length * K * 4))
results = {}
for name, call in PATHS.items():
    for _ in range(args.warmup):
        one(call)
    runs = []
    for _ in range(args.runs):
        st, results[name] = one(call)
        runs.append(st)
    med = {key: float(np.median([r[key] for r in runs])) for key in runs[0]}
    out["paths"][name] = dict(median_ms=med, kernel_min_ms=float(min(r["kernel"] for r in runs)),
                              kernel_max_ms=float(max(r["kernel"] for r in runs)),
                              kernel_units_per_s=units / (med["kernel"] * 1e-3))
if "dynamic" in out["paths"]:
    lat, dyn = out["paths"]["lattice_shell"], out["paths"]["dynamic"]
    spread = max(lat["kernel_max_ms"] - lat["kernel_min_ms"], dyn["kernel_max_ms"] - dyn["kernel_min_ms"])
    out["projection_stage"] = dict(lattice_ms=lat["median_ms"]["kernel"], dynamic_ms=dyn["median_ms"]["kernel"],
                                   ratio_lattice_over_dynamic=lat["median_ms"]["kernel"] / dyn["median_ms"]["kernel"],
                                   spread_ms=spread,
                                   condition_met=bool(dyn["median_ms"]["kernel"] - lat["median_ms"]["kernel"] > spread))
    # the two per-vector results differ by the rounding of k to float32 alone
    a, b = results["lattice_per_vector"], results["dynamic"]
    out["per_vector_against_dynamic_rel_max"] = [float(np.max(np.abs(a[i] - b[i])) / np.max(np.abs(b[i]))) for i in range(rows)]
if args.spot_check and "dynamic" in out["paths"]:
    # a few columns in float64 on the host (tests/lattice64.py, the trajectory downloaded in chunks of frames): how far
    # each path's per-vector fields are from the definition, each against the largest value of the column's field
    import lattice64                                                      # noqa: E402
    cols = np.unique(np.linspace(0, K - 1, args.spot_check).astype(int))
    q64 = np.zeros((cols.size, 4 if currents else 1, T), np.complex128)
    for t0 in range(0, T, 128):
        nt = min(128, T - t0)
        pos = eng.download(_hip.SLOT_POSITIONS, t0, nt)
        vel = eng.download(_hip.SLOT_VELOCITIES, t0, nt) if currents else None
        q64[:, :, t0:t0 + nt] = lattice64.project64(pos, vel, ind[cols], inv, None, None, currents)
    ref = lattice64.spectra64(q64, ind[cols], inv, seg.window_array(), seg.length, seg.hop)
    spot = dict(columns=[int(c) for c in cols], indices=ind[cols].tolist())
    for i, field in enumerate(("density", "longitudinal", "transverse")[:rows]):
        top = np.max(np.abs(ref[i]), axis=0)
        for path in ("lattice_per_vector", "dynamic"):
            spot[f"{field}_{path}_rel_max"] = [float(x) for x in np.max(np.abs(results[path][i][:, cols] - ref[i]), axis=0) / top]
        spot[f"{field}_largest_value"] = [float(x) for x in top]
    out["float64_spot_check"] = spot
for nc, name in ((1, "density"), (4, "currents")):
    out[f"accumulate_block_{name}"] = accumulate_block_mix(nc) or "no build/lattice.s (make asm)"
eng.close()
text = json.dumps(out, indent=1)
print(text)
if args.out:
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(text + "\n")
