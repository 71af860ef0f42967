"""K1 time per launch of the low-rank route for k-paths against the dense planes kernels at configuration 3, on the
generated trajectory: the whole 256-vector path, and one 128-vector shard of it (K_total = 256, what one rank of a
two-rank k-sharded run projects) with the per-launch minimum at 128 (route) and 256 (dense).  Arms interleaved.
    python tools/lowrank_ab.py [reps] [arm]    (one JSON line per arm and round; an arm alone: one round, for traces)"""
import json
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from psa_amd import SEDCalculator, Trajectory, _hip, synth  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 6
spec, req = synth.baseline_spec("C3")
r0, types, box = synth.lattice(spec.cells)
eng = _hip.Engine(0)
synth.fill_device(eng, _hip.SLOT_VELOCITIES, spec, synth.mode_tables(spec, r0))
stub = np.zeros((1, spec.n_atoms, 3), np.float32)
calc = SEDCalculator(Trajectory(stub, stub, types, np.zeros(1, np.float32), box, np.diag(box).copy(),
                                np.zeros(3, np.float32), spec.dt_ps), *spec.cells)
_, vecs = calc.get_k_path(req["direction"], req["bz_coverage"], req["n_k"])
vecs = np.asarray(vecs, np.float32)
K = len(vecs)
arms = [("whole_dense", 0, 128, K), ("whole_lowrank", 1, 128, K), ("shard128_dense", 1, 256, K // 2),
        ("shard128_lowrank", 1, 128, K // 2)]
only = sys.argv[2] if len(sys.argv) > 2 else None
for rnd in range(1 if only else 3):
    for name, on, min_local, nk in arms:
        if only and name != only:
            continue
        eng.set_option(_hip.OPT_K1_LOWRANK, on)
        eng.set_option(_hip.OPT_K1_LOWRANK_MIN_LOCAL, min_local)
        run = lambda: eng.project(_hip.SLOT_VELOCITIES, r0, vecs[:nk], None, 0, K_total=K, k_offset=0)
        run()
        eng.synchronize()
        eng.k1_stats()
        l0 = eng.lowrank_launches()
        for _ in range(reps):
            run()
        eng.synchronize()
        n, ms = eng.k1_stats()
        print(json.dumps({"round": rnd, "arm": name, "k_local": nk, "k1_ms_per_launch": round(ms / n, 3),
                          "lowrank_launches": eng.lowrank_launches() - l0, "launches": n}), flush=True)
