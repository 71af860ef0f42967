#!/usr/bin/env python3
"""The bond-persistence call at size (GPU box): 8 `--cells`^3 atoms (16: 32768) x `--frames` frames of one species,
`--origin-step` 10, `--lags` 64 logarithmic lags up to `--max-lag` 2048, sample_step 1, r_break = 1.1 r_cut, continuous on and
off, on two trajectories that bracket what the step pass can meet:
  hbm_noise  generated in HBM (psa_data_fill_synthetic into the positions slot): every frame an independent Gaussian cloud of
             unit width, r_cut the radius that holds `--neighbours` atoms at the cloud's centre -- every bond is broken one
             frame later, so between two listed lags a continuous call has next to nothing left to test;
  crystal    the diamond lattice of the same atoms with a thermal noise of 0.1 A (64 distinct frames, repeated; uploaded
             once and resident before anything is timed), r_cut 2.8 A between the first and the second shell: 4 neighbours an
             atom and almost no bond ever breaks, so every visited frame tests every bond -- the step pass's worst case.
After `--warmup` calls, medians of `--runs` calls of the stage times (psa_last_timings) and of the call end to end (host
clock):
  fractions    the fraction pass of the origins                              neighbours   the neighbour pass
  persistence  the tag pass and, per visited frame, the fraction pass of the lagged frames, the step pass and -- at a listed
               lag -- the reduce: one span (a stage timer per visited frame would cost two events each, thousands a call)
Beside them what the span is measured against:
  * the neighbour pass of the same call;
  * the byte floor of the step pass, 256 + 24 + 16 bytes per centre and visited frame (the tags; the fractions of the centre
    and of a neighbour; the two masks) over `--copy-gbs`, the copy rate DESIGN records (6290 GB/s);
  * the launches of the span (three per visited frame and block at most) -- counted, not timed.
`rocprofv3 --kernel-trace --stats -- python tools/persistence_timing.py --runs 1 --warmup 0` in a run of its own gives the
kernels' own times (profiles/persistence_kernel_stats.csv).
    python tools/persistence_timing.py [--runs 5] [--warmup 2] [--out profiles/persistence_timing.json]"""
import argparse
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import numpy as np                                                       # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--cells", type=int, default=16)
ap.add_argument("--frames", type=int, default=2304)
ap.add_argument("--origin-step", type=int, default=10)
ap.add_argument("--lags", type=int, default=64)
ap.add_argument("--max-lag", type=int, default=2048)
ap.add_argument("--r-cut", type=float, default=2.8)
ap.add_argument("--neighbours", type=float, default=12.0)
ap.add_argument("--hysteresis", type=float, default=1.1)
ap.add_argument("--copy-gbs", type=float, default=6290.0)
ap.add_argument("--runs", type=int, default=5)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--out", default=None)
args = ap.parse_args()

PER_ORIGIN, STEP_BYTES = 1040 + 288, 256 + 24 + 16


def log_lags(n, last):
    """n strictly ascending integer lags in [1, last], as evenly spaced in the logarithm as distinct integers allow"""
    want = n
    while True:
        lags = np.unique(np.rint(np.geomspace(1, last, want)).astype(np.int64))
        if lags.size >= n:
            keep = np.unique(np.rint(np.linspace(0, lags.size - 1, n)).astype(np.int64))
            return lags[keep]
        want += 1


def measure_all():
    from psa_amd import _hip, synth
    eng = _hip.Engine(0)
    spec = synth.SyntheticSpec((args.cells,) * 3, args.frames)
    r0, types, box = synth.lattice(spec.cells)
    H = np.asarray(box, np.float32).astype(np.float64)
    n_atoms, T, s = spec.n_atoms, args.frames, args.origin_step
    lags = log_lags(args.lags, args.max_lag)
    assert lags.size == args.lags and lags[-1] == args.max_lag <= T - 1
    n_o = (T - 1) // s + 1
    budget = dict((name, default) for _, name, default in _hip.option_table())["PSA_OPT_DYNAMIC_WORK_BYTES"]
    res = dict(device=eng.device_info()["name"], runs=args.runs, warmup=args.warmup, atoms=n_atoms, frames=T, origin_step=s, origins=n_o,
               lags=lags.tolist(), hysteresis=args.hysteresis, sample_step=1, copy_gbs=args.copy_gbs,
               step_bytes_per_centre_and_frame=STEP_BYTES, origins_per_block_at_the_default_budget=int(min(n_o, budget // (PER_ORIGIN * n_atoms))))
    for where in ("hbm_noise", "crystal"):
        if where == "hbm_noise":
            synth.fill_device(eng, _hip.SLOT_POSITIONS, spec, synth.mode_tables(spec, r0))
            # the density at the centre of a Gaussian cloud of unit width is N / (2 pi)^(3/2)
            r_cut = float((args.neighbours * (2.0 * np.pi) ** 1.5 / n_atoms * 3.0 / (4.0 * np.pi)) ** (1.0 / 3.0))
        else:
            rng = np.random.default_rng(args.cells)
            some = (r0[None].astype(np.float64) + 0.1 * rng.standard_normal((64,) + r0.shape)).astype(np.float32)
            pos = np.ascontiguousarray(np.tile(some, (-(-T // 64), 1, 1))[:T])
            eng.ensure_resident(_hip.SLOT_POSITIONS, pos)
            r_cut = args.r_cut
        res[where] = timed_calls(eng, H, r_cut, lags, n_atoms, T, s)
    eng.close()
    return res


def timed_calls(eng, H, r_cut, lags, n_atoms, T, s):
    res = dict(r_cut=r_cut, r_break=r_cut * args.hysteresis)
    origins = np.arange(0, T, s)
    for name, continuous in (("continuous", True), ("intermittent_only", False)):
        visited = np.arange(1, args.max_lag + 1) if continuous else lags
        # (origin, visited frame) pairs with o + f <= T - 1: the centre rows the step pass walks are n_atoms times that
        origin_frames = int(sum(int((origins + f <= T - 1).sum()) for f in visited))
        kept = {}

        def one():
            eng.timings()
            t0 = time.perf_counter()
            kept["out"] = eng.bond_persistence(H, r_cut, lags, None, s, r_break=r_cut * args.hysteresis, continuous=continuous)
            ms = 1e3 * (time.perf_counter() - t0)
            st = eng.timings()
            return dict(e2e=ms, fractions=st["gather"], neighbours=st["transpose"], persistence=st["phase"], d2h=st["d2h"])
        for _ in range(args.warmup):
            one()
        runs = [one() for _ in range(args.runs)]
        med = {k: float(np.median([r[k] for r in runs])) for k in runs[0]}
        got = kept["out"]
        floor_ms = 1e3 * STEP_BYTES * n_atoms * origin_frames / (args.copy_gbs * 1e9)
        res[name] = dict(visited_frames=int(visited.size), origin_frames=origin_frames, median_ms=med,
                         min_ms={k: float(min(r[k] for r in runs)) for k in runs[0]}, max_ms={k: float(max(r[k] for r in runs)) for k in runs[0]},
                         persistence_over_neighbour_pass=med["persistence"] / med["neighbours"],
                         step_byte_floor_ms=floor_ms, persistence_over_byte_floor=med["persistence"] / floor_ms,
                         bonds_first_lag=int(got["bonds"][0].sum()), mean_neighbours=float(got["bonds"][0].sum()) / max(int(got["lost"][0].sum()), 1),
                         alive_share_first_lag=float(got["alive"][0].sum()) / max(float(got["bonds"][0].sum()), 1.0),
                         alive_share_last_lag=float(got["alive"][-1].sum()) / max(float(got["bonds"][-1].sum()), 1.0),
                         unbroken_share_last_lag=float(got["unbroken"][-1].sum()) / max(float(got["bonds"][-1].sum()), 1.0),
                         truncated_first_lag=int(got["truncated"][0].sum()))
    return res


text = json.dumps(measure_all(), indent=1)
print(text)
if args.out:
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(text + "\n")
