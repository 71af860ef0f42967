"""K1 time per launch of the low-rank k-path route at configuration 3 with each arm of its combine: PSA_K1_COMBINE=0
the scalar kernel (k1_planes_diff.hip), 1 the packed complex-weights kernel and 2, the default, the packed
real-weights kernel (both lowrank_combine.hip).  PSA_K1_COMBINE is read when an engine is created, so every arm runs in a
process of its own; rounds interleave the arms.  K1 = node pass + D pass + combine, timed together (psa_k1_stats).
    python tools/lowrank_arms_ab.py [rounds] [reps]        one JSON line per arm and round"""
import json
import os
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
ARMS = {"scalar_combine": "0", "packed_combine": "1", "real_weights_combine": "2"}

CHILD = r"""
import json, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from psa_amd import SEDCalculator, Trajectory, _hip, synth
reps = int(sys.argv[2])
spec, req = synth.baseline_spec("C3")
r0, types, box = synth.lattice(spec.cells)
eng = _hip.Engine(0)
synth.fill_device(eng, _hip.SLOT_VELOCITIES, spec, synth.mode_tables(spec, r0))
stub = np.zeros((1, spec.n_atoms, 3), np.float32)
calc = SEDCalculator(Trajectory(stub, stub, types, np.zeros(1, np.float32), box, np.diag(box).copy(),
                                np.zeros(3, np.float32), spec.dt_ps), *spec.cells)
_, vecs = calc.get_k_path(req["direction"], req["bz_coverage"], req["n_k"])
vecs = np.asarray(vecs, np.float32)
run = lambda: eng.project(_hip.SLOT_VELOCITIES, r0, vecs, None, 0)
run()
eng.synchronize()
eng.k1_stats()
l0 = eng.lowrank_launches()
for _ in range(reps):
    run()
eng.synchronize()
n, ms = eng.k1_stats()
print(json.dumps({"k1_ms_per_launch": round(ms / n, 3), "lowrank_launches": eng.lowrank_launches() - l0, "launches": n}))
eng.close()
"""

rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 3
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 10
for rnd in range(rounds):
    for name, arm in ARMS.items():
        env = dict(os.environ, PSA_K1_COMBINE=arm)
        res = subprocess.run([sys.executable, "-c", CHILD, str(ROOT), str(reps)], env=env, capture_output=True, text=True,
                             timeout=600)
        if res.returncode != 0:
            sys.exit(f"arm {name}: exit {res.returncode}\n{res.stderr[-2000:]}")
        line = json.loads(res.stdout.strip().splitlines()[-1])
        print(json.dumps({"round": rnd, "arm": name, **line}), flush=True)
