#!/usr/bin/env python3
"""The dynamic structure factor and the current correlations at size (GPU box): N = 32768 atoms x T = 4096 frames generated
in HBM (psa_data_fill_synthetic into both slots), the 256-vector [110] path, its first 16 vectors and its first one,
density only and with currents, Segments(1024, 512, "hann").  After warm-up, medians of `--runs` calls, in one process, of
  - the stage times (psa_last_timings) of psa_dynamic_spectra: kernel, FFT, window and power, D2H;
  - Engine.dynamic_spectra end to end (host clock; the call ends in a device synchronise).
Beside them:
  - two issue-time figures of the kernel: (k-vector, atom, frame) units / 64 lanes x the issue cycles of the inner loop
    per atom / (SIMDs x clock).  The instructions are counted here, from `make asm`'s build/dynamic.s (the block that
    holds v_sin_f32 up to its back edge; tools/asm_blocks.py prints the same block's mix for a reader, but is a script
    without an interface, so it is not called).  `one_wave_stream_ms` prices them at what ONE wavefront's stream
    sustains (4 cycles a plain VALU instruction, 8 a v_sin_f32 / v_cos_f32: MI355X_MICROARCH's constants table) -- not a
    floor once several wavefronts share a SIMD; `simd_issue_floor_ms` at what the 32-lane SIMD itself can issue (2
    cycles per wave64 instruction, 4 per transcendental): the floor.  The clock is read from rocm-smi after the timed
    calls where that works, else --clock-mhz;
  - the float64 restatement (tests/dynamic64.py) of a bounded sample on the host, units per second: what the same
    spectra cost without the feature;
  - the extrapolation of the K = 256 call to configuration-3 size (T = 65536: 16 x the frames), marked as one.
Kernel times: run it under `rocprofv3 --kernel-trace --stats` in a run of its own.
    python tools/dynamic_timing.py [--frames 4096] [--L 1024] [--hop 512] [--runs 10] [--out profiles/dynamic_timing.json]"""
import argparse
import json
import re
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import numpy as np                                                       # noqa: E402
from psa_amd import SEDCalculator, Segments, Trajectory, _hip, synth     # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=4096)
ap.add_argument("--L", type=int, default=1024)
ap.add_argument("--hop", type=int, default=512)
ap.add_argument("--runs", type=int, default=10)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--clock-mhz", type=float, default=2400.0)
ap.add_argument("--sample-frames", type=int, default=4)
ap.add_argument("--out", default=None)
args = ap.parse_args()


def inner_loop_cycles(nc):
    """(plain VALU per atom, transcendentals per atom) of dynamic_project_kernel<nc>'s inner loop in build/dynamic.s, or
    None without the listing"""
    listing = ROOT / "psa_amd" / "csrc" / "build" / "dynamic.s"
    if not listing.exists():
        return None
    asm = listing.read_text()
    name = re.findall(rf"^(_ZN\S*dynamic_project_kernelILi{nc}E\S*):", asm, flags=re.M)[0]
    body = asm[asm.index(name + ":"):]
    body = body[:body.index("s_endpgm")]
    hot = next(b for b in re.split(r"\n\.LBB\d+_\d+:", body) if "v_sin_f32" in b)
    loop = hot.split("s_cbranch")[0]                                   # up to the back edge
    ops = [ln.split()[0] for ln in loop.splitlines() if ln.startswith("\t") and ln.split() and ln.split()[0].startswith("v_")]
    trans = sum(op.startswith(("v_sin_f32", "v_cos_f32")) for op in ops)
    atoms = trans // 2
    plain = len(ops) - trans
    return plain / atoms, trans / atoms


def read_clock_mhz():
    try:
        txt = subprocess.run(["rocm-smi", "--showclocks"], capture_output=True, text=True, timeout=20).stdout
        m = re.search(r"sclk clock level:\s*\d+:?\s*\((\d+)Mhz\)", txt)
        return float(m.group(1)) if m else None
    except (OSError, subprocess.SubprocessError):
        return None


spec = synth.SyntheticSpec((16, 16, 16), args.frames)
r0, types, box = synth.lattice(spec.cells)
T, N = spec.n_frames, spec.n_atoms
eng = _hip.Engine(0)
tables = synth.mode_tables(spec, r0)
for slot in (_hip.SLOT_VELOCITIES, _hip.SLOT_POSITIONS):
    synth.fill_device(eng, slot, spec, tables)
stand = np.broadcast_to(np.float32(0), (T, N, 3))
traj = Trajectory(stand, stand, types, np.broadcast_to(np.float32(0), (T,)), box, np.diag(box).copy(), np.zeros(3, np.float32),
                  spec.dt_ps)
calc = SEDCalculator(traj, *spec.cells)
_, path = calc.get_k_path([1, 1, 0], 1.0, 256)
path = np.asarray(path, np.float32)
seg = Segments(args.L, args.hop, "hann")
eng.set_segments(seg)
info = eng.device_info()
simds = 4 * info["compute_units"]


def one(k, currents):
    eng.timings()
    t0 = time.perf_counter()
    eng.dynamic_spectra(k, None, currents)
    ms = 1e3 * (time.perf_counter() - t0)
    st = eng.timings()
    return dict(e2e=ms, kernel=st["project"], fft=st["fft"], window_power=st["epilogue"], d2h=st["d2h"])


out = dict(T=T, N=N, L=seg.length, hop=seg.hop, n_seg=seg.count(T), runs=args.runs, device=info["name"], simds=simds, calls={})
for K in (256, 16, 1):
    for currents in (False, True):
        k = path[:K]
        for _ in range(args.warmup):
            one(k, currents)
        runs = [one(k, currents) for _ in range(args.runs)]
        med = {key: float(np.median([r[key] for r in runs])) for key in runs[0]}
        units = float(K) * N * T
        entry = dict(K=K, currents=currents, units=units, median_ms=med, e2e_min_ms=float(min(r["e2e"] for r in runs)),
                     e2e_max_ms=float(max(r["e2e"] for r in runs)), kernel_units_per_s=units / (med["kernel"] * 1e-3))
        out["calls"][f"K{K}_{'currents' if currents else 'density'}"] = entry
clock = read_clock_mhz()
out["clock_mhz"] = clock or args.clock_mhz
out["clock_source"] = "rocm-smi after the timed calls" if clock else "--clock-mhz (not read)"
for nc, name in ((1, "density"), (4, "currents")):
    cyc = inner_loop_cycles(nc)
    if cyc is None:
        out[f"inner_loop_{name}"] = "no build/dynamic.s (make asm)"
        continue
    plain, trans = cyc
    one_wave, simd = 4.0 * plain + 8.0 * trans, 2.0 * plain + 4.0 * trans
    out[f"inner_loop_{name}"] = dict(plain_valu_per_atom=plain, transcendentals_per_atom=trans,
                                     one_wave_stream_cycles_per_atom=one_wave, simd_issue_cycles_per_atom=simd)
    for K in (256, 16, 1):
        e = out["calls"][f"K{K}_{name}"]
        per_cycle = e["units"] / 64.0 / (simds * out["clock_mhz"] * 1e6) * 1e3
        e["one_wave_stream_ms"], e["simd_issue_floor_ms"] = per_cycle * one_wave, per_cycle * simd
        e["kernel_over_one_wave_stream"] = e["median_ms"]["kernel"] / e["one_wave_stream_ms"]
        e["kernel_over_simd_issue_floor"] = e["median_ms"]["kernel"] / e["simd_issue_floor_ms"]
e = out["calls"]["K256_currents"]
out["extrapolation_to_configuration_3"] = dict(note="extrapolated, not measured: 16 x the frames of the K = 256 call with currents",
                                               frames=65536, units=e["units"] * 65536 / T, kernel_ms=e["median_ms"]["kernel"] * 65536 / T,
                                               e2e_ms=e["median_ms"]["e2e"] * 65536 / T)

# the float64 restatement of a bounded sample on the host: a few frames, 16 k-vectors
import dynamic64                                                         # noqa: E402
f = args.sample_frames
pos, vel = eng.download(_hip.SLOT_POSITIONS, 0, f), eng.download(_hip.SLOT_VELOCITIES, 0, f)
t0 = time.perf_counter()
ref = dynamic64.project64(pos, vel, path[:16])
host_s = time.perf_counter() - t0
got = eng.debug_dynamic_project(path[:16])[:, :, :f]
out["host_float64_sample"] = dict(frames=f, K=16, units=16.0 * N * f, seconds=host_s, units_per_s=16.0 * N * f / host_s,
                                  gpu_rel_max_against_it=float(np.max(np.abs(got - ref)) / np.max(np.abs(ref))))
eng.close()
text = json.dumps(out, indent=1)
print(text)
if args.out:
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(text + "\n")
