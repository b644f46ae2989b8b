"""A/B timing of the key-free routing agreement (rp_ring_route_share_dev) against the sampled
estimate a caller had before it (rp_ring_route_views_dev over a key set), in ONE process, legs
alternating, HIP-event timed.

    python tools/ab_route_share.py [--servers 10000] [--log2 20] [--kills 100] [--sim-rounds 6]
                                   [--suspicion 3] [--rounds 7] [--only LEG] [--out FILE]

The configuration is that of tools/ab_route.py: a ring of `servers` servers x 100 distinct points
and a GossipSim of as many nodes; `kills` nodes are killed at round 1 and the simulator runs
`sim-rounds` rounds with a short suspicion period. Every node's ring membership is one view; the
truth is the nodes that are up.

  keys       rp_ring_route_views_dev, counts only, over 2^log2 device UUID keys (the parent's way)
  share      rp_ring_route_share_dev with wrong / lost
  share_pos  the same with pos_wrong

Prints one JSON object: medians with min-max, share / keys (goal: <= 2), and what the exact value
buys: per active view wrong_keys / 2^log2 against wrong_share / 2^32, the largest gap in units of
the binomial standard error, and how many views the sample reports as 0 although they disagree
somewhere. --only runs one leg alone (for a kernel trace).
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from ab_route import collision_free  # noqa: E402

LEGS = ("keys", "share", "share_pos")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--servers", type=int, default=10000)
    ap.add_argument("--log2", type=int, default=20)
    ap.add_argument("--kills", type=int, default=100)
    ap.add_argument("--sim-rounds", type=int, default=6)
    ap.add_argument("--suspicion", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--only", choices=LEGS, default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("ab_route_share.py needs a HIP device (there is no CPU fallback)")
    rpa = bench.load_pkg()
    S = bench._synth()
    N, B = a.servers, 1 << a.log2
    names, replaced = collision_free(rpa, S, N)
    inc0 = S.c3_members(N)[2]
    killed = np.flatnonzero(S.kill_set(N, a.kills, 11))
    sim = rpa.GossipSim(names, inc0, np.zeros(N, dtype=np.uint8), suspicion_rounds=a.suspicion,
                        events=[(1, "kill", int(v)) for v in killed])
    sim.step(a.sim_rounds)
    truth = np.ones(N, dtype=bool)
    truth[killed] = False
    ring = rpa.HashRing()
    ring.addRemoveServers(names)
    M = ring.size
    assert M == N * 100  # every replica token is distinct
    ids = np.array([ring.server_id(s) for s in names])
    assert (ids == np.arange(N)).all() and ring.id_bound() == N  # member index == ring id
    rows_h = np.stack([sim.ring_members(v) for v in range(N)])
    sim.close()
    st = torch.cuda.current_stream()
    keys = torch.empty(B * 36, dtype=torch.uint8, device="cuda")
    rpa.gen_uuid_keys_dev(42, 0, B, keys.data_ptr(), st.cuda_stream)
    rows = torch.from_numpy(rows_h.astype(np.uint8)).cuda()
    d_truth = torch.from_numpy(truth.astype(np.uint8)).cuda()
    out = {leg: (torch.zeros(N, dtype=torch.int64, device="cuda"), torch.zeros(N, dtype=torch.int64, device="cuda"))
           for leg in LEGS}
    pos = torch.zeros(M, dtype=torch.int32, device="cuda")

    def run(leg):
        w, lo = out[leg]
        if leg == "keys":
            ring.route_views_dev(B, rows.data_ptr(), N, N, keys_ptr=keys.data_ptr(), truth_ptr=d_truth.data_ptr(),
                                 active_ptr=d_truth.data_ptr(), wrong_ptr=w.data_ptr(), lost_ptr=lo.data_ptr(),
                                 stream=st.cuda_stream)
        else:
            ring.route_share_dev(rows.data_ptr(), N, N, truth_ptr=d_truth.data_ptr(), active_ptr=d_truth.data_ptr(),
                                 wrong_ptr=w.data_ptr(), lost_ptr=lo.data_ptr(),
                                 pos_wrong_ptr=pos.data_ptr() if leg == "share_pos" else None, pos_cap=M,
                                 stream=st.cuda_stream)

    def timed(leg):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        run(leg)
        e1.record(st)
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    legs = (a.only,) if a.only else LEGS
    times = {leg: [] for leg in legs}
    for r in range(a.rounds + 1):  # round 0 warms every shape up and is not timed
        for i in range(len(legs)):
            leg = legs[(i + r) % len(legs)]  # the order rotates from round to round
            ms = timed(leg)
            if r:
                times[leg].append(ms)

    def stat(t):
        return {"median_ms": float(np.median(t)), "min_ms": float(np.min(t)), "max_ms": float(np.max(t))}
    res = {"servers": N, "tokens": int(M), "keys": B, "views": N, "active_views": int(truth.sum()),
           "kills": int(len(killed)), "sim_rounds": a.sim_rounds, "suspicion_rounds": a.suspicion, "rounds": a.rounds,
           "names_replaced_for_distinct_tokens": int(replaced)}
    for leg in legs:
        res[leg] = stat(times[leg])
    if not a.only:
        res["share_over_keys"] = res["share"]["median_ms"] / res["keys"]["median_ms"]
        res["share_pos_over_keys"] = res["share_pos"]["median_ms"] / res["keys"]["median_ms"]
        res["goal_share_over_keys_at_most_2"] = bool(res["share_over_keys"] <= 2.0)
        wk, lk = (x.cpu().numpy().astype(np.float64) for x in out["keys"])
        ws, ls = (x.cpu().numpy().astype(np.float64) for x in out["share"])
        wp, lp = (x.cpu().numpy().astype(np.float64) for x in out["share_pos"])
        res["share_legs_identical"] = bool((ws == wp).all() and (ls == lp).all())
        act = truth
        p = ws[act] / 2.0 ** 32
        est = wk[act] / B
        se = np.sqrt(p * (1 - p) / B)
        ok = se > 0
        z = np.abs(est[ok] - p[ok]) / se[ok]
        ln = np.diff(ring.dump()[0].astype(np.int64), prepend=int(ring.dump()[0][-1]) - (1 << 32))
        res["exact_against_sample"] = {
            "wrong_share_total_of_2^32": float(p.sum()), "wrong_keys_total_of_keys": float(est.sum()),
            "lost_share_total_of_2^32": float(ls[act].sum() / 2.0 ** 32), "lost_keys_total_of_keys": float(lk[act].sum() / B),
            "views_that_disagree_somewhere": int((p > 0).sum()),
            "of_those_the_sample_reports_zero": int(((p > 0) & (est == 0)).sum()),
            "smallest_nonzero_share": float(p[p > 0].min()) if (p > 0).any() else 0.0,
            "largest_gap_in_standard_errors": float(z.max()) if len(z) else 0.0,
            "mean_gap_in_standard_errors": float(z.mean()) if len(z) else 0.0,
            "largest_absolute_gap": float(np.abs(est - p).max()),
            "disputed_share_of_2^32": float(ln[pos.cpu().numpy() > 0].sum() / 2.0 ** 32)}
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    if not a.only and not res["share_legs_identical"]:
        sys.exit("the two share legs disagree")


if __name__ == "__main__":
    main()
