"""A/B timing of the simulator's timeline against the per-round loop it replaces, at C4 (10,000
nodes, 1 % down from the start, run to convergence). The two legs alternate, each run in a fresh
process, after one warm-up run of each that is not reported.

    python tools/ab_timeline.py [--parent-lib FILE] [--runs 3] [--out FILE]
    rocprofv3 --kernel-trace --stats ... -- python tools/ab_timeline.py --leg timeline

  timeline   this tree: timeline_enable(R); step_async(R); timeline(), R = the rounds the loop leg's
             warm-up run needed to converge, so both legs run the same rounds (the recorded
             rounds_to_convergence must agree with the loop's: the last record is the first converged)
  loop       the C4 leg of bench.py: step(1); converged() until it converges, straight on the C ABI
             of --parent-lib (the parent commit's librpamd.so, which has no timeline entry points;
             default: this tree's library)

Both report wall time per round over their whole run (the simulator already created, the device
idle at the start, the last result on the host at the end). The spread of the loop leg's own runs
is the yardstick for the ratio. Prints one JSON object and writes it to --out when given.
"""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
N, KILL, SEED, SUSP, LIMIT = 10000, 100, 11, 25, 300


def cluster():
    import bench
    S = bench._synth()
    return [S.c2_addr(i) for i in range(N)], S.c3_members(N)[2], S.kill_set(N, KILL, SEED)


def leg_timeline(rounds):
    import bench
    import torch
    rpa = bench.load_pkg()
    names, inc0, dead = cluster()
    sim = rpa.GossipSim(names, inc0, dead, seed=SEED, suspicion_rounds=SUSP)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    sim.timeline_enable(rounds)
    sim.step_async(rounds)
    tl = sim.timeline()
    dt = time.perf_counter() - t0
    sim.close()
    conv = rpa.rounds_to_convergence(tl)
    return {"leg": "timeline", "rounds_run": rounds, "rounds_to_convergence": None if conv is None else conv + 1,
            "ms_per_round": dt * 1e3 / rounds, "unmet_first": int(tl["unmet"][0]), "applied": int(tl["stats"][-1][3])}


def leg_loop(lib_path):
    import torch  # the HIP runtime the library binds to, as the package loads it
    assert torch.cuda.is_available()
    L = ctypes.CDLL(lib_path)
    P = ctypes.c_void_p
    L.rp_sim_create.argtypes = [ctypes.c_uint32, P, P, P, P, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_int64,
                                ctypes.c_int, P]
    L.rp_sim_step.argtypes = [P, ctypes.c_uint32]
    L.rp_sim_converged.argtypes = [P, P]
    L.rp_sim_destroy.argtypes = [P]
    names, inc0, dead = cluster()
    blob = "".join(names).encode()
    off = np.zeros(N + 1, dtype=np.uint32)
    off[1:] = np.cumsum([len(s) for s in names])
    inc0 = np.ascontiguousarray(inc0, dtype=np.int64)
    dead = np.ascontiguousarray(dead, dtype=np.uint8)
    h = P()
    rc = L.rp_sim_create(N, blob, off.ctypes.data, inc0.ctypes.data, dead.ctypes.data, SEED, SUSP,
                         1434401518824 + 10 ** 9, 0, ctypes.byref(h))
    assert rc == 0, rc
    torch.cuda.synchronize()
    c = ctypes.c_int()
    rounds, t0 = 0, time.perf_counter()
    while rounds < LIMIT and not c.value:
        assert L.rp_sim_step(h, 1) == 0
        assert L.rp_sim_converged(h, ctypes.byref(c)) == 0
        rounds += 1
    dt = time.perf_counter() - t0
    L.rp_sim_destroy(h)
    return {"leg": "loop", "rounds_run": rounds, "rounds_to_convergence": rounds if c.value else None,
            "ms_per_round": dt * 1e3 / rounds}


def child(args):
    out = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, check=True, capture_output=True,
                         text=True, timeout=240).stdout
    return json.loads(out.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=os.path.join(REPO, "ringpop-node_amd", "librpamd.so"))
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=39)
    ap.add_argument("--leg", choices=("timeline", "loop"), help="one run of one leg in this process")
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.leg:
        print(json.dumps(leg_timeline(a.rounds) if a.leg == "timeline" else leg_loop(a.parent_lib)))
        return
    loop_args = ["--leg", "loop", "--parent-lib", a.parent_lib]
    warm = child(loop_args)
    assert warm["rounds_to_convergence"], "the loop leg did not converge"
    tl_args = ["--leg", "timeline", "--rounds", str(warm["rounds_to_convergence"])]
    child(tl_args)
    runs = []
    for _ in range(max(a.runs, 3)):
        runs.append(child(loop_args))
        runs.append(child(tl_args))
    loop = [r["ms_per_round"] for r in runs if r["leg"] == "loop"]
    tl = [r["ms_per_round"] for r in runs if r["leg"] == "timeline"]
    res = {"config": "C4: %d nodes, %d down from the start, suspicion %d rounds" % (N, KILL, SUSP),
           "parent_lib": os.path.relpath(a.parent_lib, REPO), "runs": runs,
           "rounds_agree": len({r["rounds_to_convergence"] for r in runs}) == 1,
           "loop_ms_per_round": {"median": float(np.median(loop)), "min": min(loop), "max": max(loop)},
           "timeline_ms_per_round": {"median": float(np.median(tl)), "min": min(tl), "max": max(tl)},
           "ratio_timeline_over_loop": float(np.median(tl) / np.median(loop)),
           "loop_spread_max_over_min": max(loop) / min(loop)}
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
