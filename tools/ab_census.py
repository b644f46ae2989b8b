"""A/B timing of the simulator's census call against the composition a caller needs without it, in
ONE process, the two legs alternating, after a warm-up.

    python tools/ab_census.py [--n 10000] [--kill 100] [--mid-round 12] [--reps 5] [--out FILE]
    rocprofv3 --kernel-trace --stats ... -- python tools/ab_census.py --fused-only --reps 20

The configuration is C4 (10,000 nodes, 1 % down from the start). The census is sampled twice: at
`mid-round`, while the suspicions of the dead nodes are still spreading, and at the first round at
which the simulator reports convergence.

  fused        GossipSim.census(): two passes over the deviation bitmaps on the device, the counts
               come back
  first_pass   GossipSim.census(want=status, in_ring, max_inc): the same without at_max / behind
  composition  today's public calls: view(v) and ring_members(v) of every node, stacked, and the
               numpy model over the stack (tests/census_model.py)

The tool checks that fused and composition are identical at both samples before it reports. Legs
are wall-clock (every leg ends synchronised with the device). Prints one JSON object with the
medians and writes it to --out when given.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import bench  # noqa: E402
import census_model as cm  # noqa: E402


def composition(sim, n, observe):
    st = np.empty((n, n), dtype=np.uint8)
    inc = np.empty((n, n), dtype=np.int64)
    ring = np.empty((n, n), dtype=bool)
    for v in range(n):
        st[v], inc[v] = sim.view(v)
        ring[v] = sim.ring_members(v)
    return cm.census(st, inc, ring, observe)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10000)
    ap.add_argument("--kill", type=int, default=100)
    ap.add_argument("--mid-round", type=int, default=12)
    ap.add_argument("--limit", type=int, default=400)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--fused-only", action="store_true",
                    help="no composition leg and no comparison (the kernel-trace run: device time of each kernel)")
    ap.add_argument("--out")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("ab_census.py needs a HIP device (there is no CPU fallback)")
    rpa = bench.load_pkg()
    S = bench._synth()
    names = [bench.c2_addr(i) for i in range(a.n)]
    inc0 = S.c3_members(a.n)[2]
    dead = S.kill_set(a.n, a.kill, 11)
    sim = rpa.GossipSim(names, inc0, dead, seed=11, suspicion_rounds=25)
    up = dead == 0
    res = {"n": a.n, "killed": a.kill, "reps": a.reps, "bitmap_words": a.n * ((a.n + 31) // 32), "samples": {}}
    ok = True

    def sample(label):
        nonlocal ok
        got = {}

        def fused():
            got["fused"] = sim.census()

        def first():
            got["first_pass"] = sim.census(want=("status", "in_ring", "max_inc"))

        def comp():
            got["composition"] = composition(sim, a.n, up)

        variants = {"fused": fused, "first_pass": first, "composition": comp}
        if a.fused_only:
            del variants["composition"]
            got["composition"] = None
        times = {k: [] for k in variants}
        for r in range(a.reps + 1):  # round 0 warms every buffer up and is not timed
            order = list(variants) if r % 2 == 0 else list(variants)[::-1]
            for name in order:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                variants[name]()
                t1 = time.perf_counter()
                if r > 0:
                    times[name].append((t1 - t0) * 1e3)
            same = a.fused_only or cm.same(got["fused"], got["composition"]) is None
            same = same and all(np.array_equal(got["first_pass"][k], got["fused"][k]) for k in got["first_pass"])
            ok = ok and same
        c = got["fused"]
        run = {"round": sim.round, "observers": c["observers"], "results_identical": bool(ok),
               "rows_not_alive": int(c["observers"]) * a.n - int(c["status"][:, 0].sum(dtype=np.int64)),
               "members_not_alive_somewhere": int((c["status"][:, 0] != c["observers"]).sum()),
               "nodes_behind": int((c["behind"] > 0).sum())}
        for name, t in times.items():
            run[name] = {"median_ms": float(np.median(t)), "min_ms": float(np.min(t)), "max_ms": float(np.max(t))}
        if not a.fused_only:
            run["fused_over_composition"] = run["fused"]["median_ms"] / run["composition"]["median_ms"]
        res["samples"][label] = run

    sim.step(a.mid_round)
    sample("spreading")
    while not sim.converged() and sim.round < a.limit:
        sim.step(1)
    res["converged"] = bool(sim.converged())
    sample("converged")
    sim.close()
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    if not ok:
        sys.exit("the fused census and the composition disagree")


if __name__ == "__main__":
    main()
