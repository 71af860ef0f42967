#!/usr/bin/env python3
"""The pair histograms at size (GPU box): g(r) (lag 0) and one G_d call (one lag > 0) of 8 `cells`^3 atoms in two species,
generated in HBM, at `--cells` 8 (4096 atoms) and 16 (32768 atoms), 200 bins at the served radius.  After `--warmup`
calls, medians of `--runs` calls of the stage times (psa_last_timings: fraction pass, pair kernel, reduce, D2H) and of
the call end to end (host clock), and per call
  * the pairs the kernel evaluates -- at lag 0 every unordered pair once (tiles of the upper triangle, the diagonal tile
    masked), at a lag > 0 every ordered pair -- and the kernel's ns per evaluated pair;
  * the same beside the VALU floor: the vector instructions per pair -- counted here in the assembly hipcc gives for
    psa_amd/csrc/pair.hip with the Makefile's flags, the block of pair_hist_kernel with the most square roots over its
    four pairs, as tests/test_pair_resources.py finds it; `--valu-per-pair` sets it where there is no hipcc -- each issued
    over 2 cycles for a wavefront's 64 lanes on each of a compute unit's 4 SIMDs (128 lanes per compute unit and clock),
    at the nominal `--clock-ghz`: the clock the chip holds under this load is not read here (the library has no entry
    for it), so the fraction is of the nominal rate and says so in the file.
`--other-library PATH` repeats everything in a fresh process on another build of the library (PSA_HIP_LIBRARY) and stores
it beside the first.  profiles/pair_timing.json holds, as `rejected`, a build of a variant of the kernel with one LDS
histogram per wavefront; that variant is not in the tree, so that half of the file cannot be repeated from it.
    python tools/pair_timing.py [--runs 5] [--warmup 2] [--other-library PATH] [--out profiles/pair_timing.json]"""
import argparse
import json
import os
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
ap.add_argument("--lag", type=int, default=8)
ap.add_argument("--n-r", type=int, default=200)
ap.add_argument("--runs", type=int, default=5)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--valu-per-pair", type=float, default=None)
ap.add_argument("--clock-ghz", type=float, default=2.4)
ap.add_argument("--other-library", default=None)
ap.add_argument("--label", default="one LDS histogram per workgroup")
ap.add_argument("--other-label", default="one LDS histogram per wavefront")
ap.add_argument("--out", default=None)
args = ap.parse_args()


def inner_loop_valu():
    """vector instructions per pair of the pair kernel's inner loop, from the assembly"""
    csrc = ROOT / "psa_amd" / "csrc"
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    mk = (csrc / "Makefile").read_text()
    line = next(ln for ln in mk.splitlines() if ln.startswith("CXXFLAGS"))
    raw = (line.split(":=")[1].rstrip("\\") + " " + mk.split(line)[1].splitlines()[1]).split()
    flags = [f.replace("$(ARCH)", "gfx950").replace("$(ROOT)", str(ROOT)) for f in raw if not f.startswith("-W")]
    with tempfile.TemporaryDirectory() as tmp:
        out = Path(tmp) / "pair.s"
        subprocess.run([hipcc, *flags, "-S", "--cuda-device-only", str(csrc / "pair.hip"), "-o", str(out)], check=True, timeout=600)
        asm = out.read_text()
    name = re.search(r"^(\w*pair_hist_kernel\w*):", asm, re.M).group(1)
    body = asm[asm.index(name + ":"):]
    blocks = re.split(r"\n\.LBB\d+_\d+:", body[:body.index("s_endpgm")])
    inner = max(blocks, key=lambda b: b.count("v_sqrt_f32") + b.count("v_rsq_f32"))
    pairs = inner.count("ds_add_u32")
    return len(re.findall(r"\n\s+v_", inner)) / pairs


if args.valu_per_pair is None:
    args.valu_per_pair, valu_source = inner_loop_valu(), "counted in the assembly of pair.hip by this run"
else:
    valu_source = "given on the command line"


def measure_all():
    from psa_amd import _hip, max_pair_radius, synth
    eng = _hip.Engine(0)
    info = eng.device_info()
    res = dict(device=info["name"], label=args.label, runs=args.runs, warmup=args.warmup, n_r=args.n_r, frames=args.frames,
               valu_per_pair=args.valu_per_pair, valu_per_pair_source=valu_source, clock_ghz=args.clock_ghz,
               clock_source="nominal, not read from the device")
    tile = _hip.PAIR_TILE
    for cells in args.cells:
        spec = synth.SyntheticSpec((cells,) * 3, args.frames)
        r0, types, box = synth.lattice(spec.cells)
        synth.fill_device(eng, _hip.SLOT_POSITIONS, spec, synth.mode_tables(spec, r0))
        H = np.asarray(box, np.float32).astype(np.float64)
        kinds = np.unique(types)
        groups = [np.flatnonzero(types == t).astype(np.int32) for t in kinds] if kinds.size == 2 else \
            [np.arange(0, types.size // 2, dtype=np.int32), np.arange(types.size // 2, types.size, dtype=np.int32)]
        sizes = [int(g.size) for g in groups]
        dr = max_pair_radius(box) / args.n_r
        tiles = [-(-n // tile) for n in sizes]
        # lane slots the kernel walks: whole tiles of 256 x 256, the masked diagonal tile included
        slots0 = tile * tile * (sum(t * (t + 1) // 2 for t in tiles) + tiles[0] * tiles[1])
        slots1 = tile * tile * sum(tiles) ** 2
        n_atoms = sum(sizes)
        for name, lags, pairs, slots in (("g_of_r", [0], n_atoms * (n_atoms - 1) // 2, slots0),
                                         ("g_d_one_lag", [args.lag], n_atoms * (n_atoms - 1), slots1)):
            n_o = args.frames - lags[0]

            def one():
                eng.timings()
                t0 = time.perf_counter()
                eng.pair_histogram(H, lags, dr, args.n_r, groups)
                ms = 1e3 * (time.perf_counter() - t0)
                st = eng.timings()
                return dict(e2e=ms, fractions=st["gather"], kernel=st["transpose"], reduce=st["epilogue"], d2h=st["d2h"])
            for _ in range(args.warmup):
                one()
            runs = [one() for _ in range(args.runs)]
            med = {k: float(np.median([r[k] for r in runs])) for k in runs[0]}
            evaluated = float(pairs) * n_o
            floor_ns = args.valu_per_pair / (info["compute_units"] * 128 * args.clock_ghz)
            res[f"{n_atoms}_atoms_{name}"] = dict(
                species=sizes, lags=lags, origins=n_o, evaluated_pairs=evaluated, lane_slots=float(slots) * n_o, median_ms=med,
                min_ms={k: float(min(r[k] for r in runs)) for k in runs[0]}, max_ms={k: float(max(r[k] for r in runs)) for k in runs[0]},
                kernel_ns_per_pair=1e6 * med["kernel"] / evaluated, valu_floor_ns_per_pair=floor_ns,
                valu_floor_over_kernel=floor_ns / (1e6 * med["kernel"] / evaluated))
    eng.close()
    return res


out = measure_all()
if args.other_library:
    env = dict(os.environ, PSA_HIP_LIBRARY=str(Path(args.other_library).resolve()))
    cmd = [sys.executable, __file__, "--cells", *map(str, args.cells), "--frames", str(args.frames), "--lag", str(args.lag), "--n-r",
           str(args.n_r), "--runs", str(args.runs), "--warmup", str(args.warmup), "--valu-per-pair", str(args.valu_per_pair), "--clock-ghz",
           str(args.clock_ghz), "--label", args.other_label]                   # (the count of THIS tree's loop, for the same floor)
    child = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900, check=True)
    out = dict(chosen=out, rejected=json.loads(child.stdout[child.stdout.index("{"):]))
text = json.dumps(out, indent=1)
print(text)
if args.out:
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(text + "\n")
