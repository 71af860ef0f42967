#!/usr/bin/env python3
"""The bond-angle call at size (GPU box): 8 `cells`^3 atoms as one species at `--cells` 8 (4096 atoms) and 16 (32768 atoms)
x `--frames` frames, placed uniformly at random in the box of the synthetic lattice (the synthetic generator fills a slot
with unit-variance noise, which as positions is one dense cloud where every centre is truncated), uploaded once and
resident in HBM before anything is timed; `--n-theta` bins, r_cut the radius that holds `--neighbours` atoms at the mean
density.
After `--warmup` calls, medians of `--runs` calls of the stage times (psa_last_timings: fraction pass, neighbour pass,
angle pass, reduce, D2H) and of the call end to end (host clock).  In the same session the pair kernel of `calculate_rdf`
(psa_pair_histogram at lag 0, 200 bins at the served radius) on the same atoms, and per size
  * the pairs each kernel evaluates -- the neighbour pass every ORDERED pair (every centre keeps its own list), the pair
    kernel at lag 0 every unordered pair once -- and the ns per evaluated pair of both, their ratio, and the ratio of
    the two kernels' times;
  * the vector instructions per pair of both inner loops, counted in the assembly hipcc gives with the Makefile's flags
    (the block with the most square roots over its four pairs), where hipcc is there;
  * the angle pass's share of the call.
    python tools/angle_timing.py [--runs 5] [--warmup 2] [--out profiles/angle_timing.json]"""
import argparse
import json
import re
import shutil
import subprocess
import sys
import tempfile
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import numpy as np                                                       # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--cells", type=int, nargs="+", default=[8, 16])
ap.add_argument("--frames", type=int, default=16)
ap.add_argument("--n-theta", type=int, default=180)
ap.add_argument("--neighbours", type=float, default=12.0)
ap.add_argument("--runs", type=int, default=5)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--out", default=None)
args = ap.parse_args()


def inner_loop_valu(source, kernel):
    """vector instructions per pair of a kernel's inner loop -- its block with the most square roots, four pairs -- from the
    assembly; None where there is no hipcc"""
    csrc = ROOT / "psa_amd" / "csrc"
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not Path(hipcc).exists():
        return None
    mk = (csrc / "Makefile").read_text()
    line = next(ln for ln in mk.splitlines() if ln.startswith("CXXFLAGS"))
    raw = (line.split(":=")[1].rstrip("\\") + " " + mk.split(line)[1].splitlines()[1]).split()
    flags = [f.replace("$(ARCH)", "gfx950").replace("$(ROOT)", str(ROOT)) for f in raw if not f.startswith("-W")]
    with tempfile.TemporaryDirectory() as tmp:
        out = Path(tmp) / "kernel.s"
        subprocess.run([hipcc, *flags, "-S", "--cuda-device-only", str(csrc / source), "-o", str(out)], check=True, timeout=600)
        asm = out.read_text()
    name = re.search(rf"^(\w*{kernel}\w*):", asm, re.M).group(1)
    body = asm[asm.index(name + ":"):]
    blocks = re.split(r"\n\.LBB\d+_\d+:", body[:body.index("s_endpgm")])
    inner = max(blocks, key=lambda b: b.count("v_sqrt_f32") + b.count("v_rsq_f32"))
    return len(re.findall(r"\n\s+v_", inner)) / max(1, inner.count("v_sqrt_f32") + inner.count("v_rsq_f32"))


def medians(one):
    for _ in range(args.warmup):
        one()
    runs = [one() for _ in range(args.runs)]
    return ({k: float(np.median([r[k] for r in runs])) for k in runs[0]}, {k: float(min(r[k] for r in runs)) for k in runs[0]},
            {k: float(max(r[k] for r in runs)) for k in runs[0]})


def measure_all():
    from psa_amd import _hip, max_pair_radius, synth
    eng = _hip.Engine(0)
    res = dict(device=eng.device_info()["name"], runs=args.runs, warmup=args.warmup, frames=args.frames, n_theta=args.n_theta,
               valu_per_pair=dict(neighbour_pass=inner_loop_valu("angle.hip", "angle_neighbours_kernel"),
                                  pair_kernel=inner_loop_valu("pair.hip", "pair_hist_kernel")))
    for cells in args.cells:
        spec = synth.SyntheticSpec((cells,) * 3, args.frames)
        box = synth.lattice(spec.cells)[2]
        H = np.asarray(box, np.float32).astype(np.float64)
        n_atoms = spec.n_atoms
        pos = (np.random.default_rng(cells).uniform(0.0, 1.0, (args.frames, n_atoms, 3)) @ H).astype(np.float32)
        eng.ensure_resident(_hip.SLOT_POSITIONS, pos)
        r_cut = float((args.neighbours / n_atoms * abs(np.linalg.det(H)) * 3.0 / (4.0 * np.pi)) ** (1.0 / 3.0))

        def angle():
            eng.timings()
            t0 = time.perf_counter()
            out = eng.angle_histogram(H, r_cut, args.n_theta)
            ms = 1e3 * (time.perf_counter() - t0)
            st = eng.timings()
            angle.out = out
            return dict(e2e=ms, fractions=st["gather"], neighbours=st["transpose"], angles=st["phase"], reduce=st["epilogue"], d2h=st["d2h"])

        def pair():
            eng.timings()
            t0 = time.perf_counter()
            eng.pair_histogram(H, [0], max_pair_radius(box) / 200, 200)
            ms = 1e3 * (time.perf_counter() - t0)
            st = eng.timings()
            return dict(e2e=ms, fractions=st["gather"], kernel=st["transpose"], reduce=st["epilogue"], d2h=st["d2h"])
        a_med, a_min, a_max = medians(angle)
        p_med, p_min, p_max = medians(pair)
        angles, coord, trunc = angle.out
        ordered, unordered = float(n_atoms) * (n_atoms - 1) * args.frames, float(n_atoms) * (n_atoms - 1) / 2 * args.frames
        ns_n, ns_p = 1e6 * a_med["neighbours"] / ordered, 1e6 * p_med["kernel"] / unordered
        res[f"{n_atoms}_atoms"] = dict(
            r_cut=r_cut, mean_neighbours=float((coord[0, 0] * np.arange(65)).sum()) / (n_atoms * args.frames), truncated=int(trunc[0]),
            triplets=int(angles.sum()), angle_call=dict(median_ms=a_med, min_ms=a_min, max_ms=a_max),
            rdf_call=dict(median_ms=p_med, min_ms=p_min, max_ms=p_max),
            neighbour_pass_pairs=ordered, pair_kernel_pairs=unordered, neighbour_pass_ns_per_pair=ns_n, pair_kernel_ns_per_pair=ns_p,
            ns_per_pair_ratio=ns_n / ns_p, kernel_time_ratio=a_med["neighbours"] / p_med["kernel"],
            angle_pass_share_of_call=a_med["angles"] / a_med["e2e"])
    eng.close()
    return res


text = json.dumps(measure_all(), indent=1)
print(text)
if args.out:
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(text + "\n")
