"""A/B timing of the fused routing-agreement call against the composition a caller needs without
it, in ONE process, legs alternating, HIP-event timed.

    python tools/ab_route.py [--servers 10000] [--log2 20] [--kills 100] [--sim-rounds 6]
                             [--suspicion 3] [--compose 64] [--rounds 7] [--out FILE]

The configuration is the C4 shape: a ring of `servers` servers x 100 points and a GossipSim of as
many nodes; `kills` nodes are killed at round 1 and the simulator runs `sim-rounds` rounds (with a
short suspicion period, so that some views have already dropped the killed members and others have
not). Every node's ring membership (rp_sim_ring_members) is one view; the truth is the nodes that
are up; 2^log2 device UUID keys.

  fused        rp_ring_route_views_dev over all views (pack + route), counts only
  composition  on `compose` of those views, per view: addRemoveServers on a twin ring to that
               view's server set (timed apart, wall clock), then rp_ring_lookup_dev and a torch
               compare against the truth owners (timed together, HIP events)

The tool checks in every round that the `compose` views' wrong / lost counts are identical in both
legs. Prints one JSON object: medians with min-max, the per-view times and their ratio (goal:
fused per view <= composition lookup-and-compare per view), and the traffic model's prediction.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402

NIL = 0xFFFFFFFF


def collision_free(rpa, S, n, points=100):
    """n synthetic server names whose n * points replica tokens are all distinct: names that lose
    a token to an earlier one are replaced by the next names of the series. Only then is a view's
    owner `lookup` on the ring built for that view alone, so that the composition leg
    answers what the fused leg answers."""
    pool, nxt = [S.c2_addr(i) for i in range(n)], n
    while True:
        r = rpa.HashRing({"replicaPoints": points})
        r.addRemoveServers(pool)
        _, own = r.dump()
        held = np.bincount(own, minlength=r.id_bound())
        short = {s for s in pool if held[r.server_id(s)] < points}
        r.close()
        if not short:
            return pool, nxt - n
        pool = [s for s in pool if s not in short] + [S.c2_addr(nxt + j) for j in range(len(short))]
        nxt += len(short)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--servers", type=int, default=10000)
    ap.add_argument("--log2", type=int, default=20)
    ap.add_argument("--kills", type=int, default=100)
    ap.add_argument("--sim-rounds", type=int, default=6)
    ap.add_argument("--suspicion", type=int, default=3)
    ap.add_argument("--compose", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("ab_route.py needs a HIP device (there is no CPU fallback)")
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
    ring, twin = rpa.HashRing(), rpa.HashRing()
    ring.addRemoveServers(names)
    twin.addRemoveServers(names)
    assert ring.size == N * 100  # every replica token is distinct
    ids = np.array([ring.server_id(s) for s in names])
    assert (ids == np.arange(N)).all() and ring.id_bound() == N  # member index == ring id in both rings
    rows_h = np.stack([sim.ring_members(v) for v in range(N)])
    sim.close()
    st = torch.cuda.current_stream()
    keys = torch.empty(B * 36, dtype=torch.uint8, device="cuda")
    rpa.gen_uuid_keys_dev(42, 0, B, keys.data_ptr(), st.cuda_stream)
    rows = torch.from_numpy(rows_h.astype(np.uint8)).cuda()
    d_truth = torch.from_numpy(truth.astype(np.uint8)).cuda()
    truth_mask = torch.cat([d_truth.bool(), torch.zeros(1, dtype=torch.bool, device="cuda")])  # (entry N: null)
    wrong = torch.zeros(N, dtype=torch.int64, device="cuda")
    lost = torch.zeros(N, dtype=torch.int64, device="cuda")
    active = np.flatnonzero(truth)
    differ = active[(rows_h[active] != truth[None, :]).any(axis=1)]
    pick = (differ if len(differ) >= a.compose else active)
    pick = pick[np.linspace(0, len(pick) - 1, a.compose).astype(int)]

    # the truth owners, from the twin ring holding exactly the truth's servers
    twin.addRemoveServers(None, [names[v] for v in killed])
    t_own = torch.empty(B, dtype=torch.int32, device="cuda")
    twin.lookup_dev(keys.data_ptr(), B, t_own.data_ptr(), stream=st.cuda_stream)
    t_own = t_own.long() & NIL
    own = torch.empty(B, dtype=torch.int32, device="cuda")
    current = truth.copy()

    def fused():
        ring.route_views_dev(B, rows.data_ptr(), N, N, keys_ptr=keys.data_ptr(), truth_ptr=d_truth.data_ptr(),
                             active_ptr=d_truth.data_ptr(), wrong_ptr=wrong.data_ptr(), lost_ptr=lost.data_ptr(),
                             stream=st.cuda_stream)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        out = fn()
        e1.record(st)
        torch.cuda.synchronize()
        return e0.elapsed_time(e1), out

    def compose_view(v):
        nonlocal current
        want = rows_h[v]
        t0 = time.perf_counter()
        twin.addRemoveServers([names[i] for i in np.flatnonzero(want & ~current)],
                              [names[i] for i in np.flatnonzero(~want & current)])
        torch.cuda.synchronize()
        rebuild = (time.perf_counter() - t0) * 1e3
        current = want.copy()

        def look():
            twin.lookup_dev(keys.data_ptr(), B, own.data_ptr(), stream=st.cuda_stream)
            o = own.long() & NIL
            return (o != t_own).sum(), (~truth_mask[torch.clamp(o, max=N)] & (o != NIL)).sum()
        ms, (w, lo) = timed(look)
        return rebuild, ms, int(w.item()), int(lo.item())

    t_fused, t_look, t_rebuild = [], [], []
    identical, worst = True, 0
    for r in range(a.rounds + 1):  # round 0 warms every shape up and is not timed
        def leg_fused():
            ms, _ = timed(fused)
            if r:
                t_fused.append(ms)

        def leg_comp():
            res = [compose_view(int(v)) for v in pick]
            if r:
                t_rebuild.append(sum(x[0] for x in res))
                t_look.append(sum(x[1] for x in res))
            return res
        if r % 2 == 0:
            leg_fused()
            res = leg_comp()
        else:
            res = leg_comp()
            leg_fused()
        w, lo = wrong.cpu().numpy(), lost.cpu().numpy()
        identical = identical and all(w[v] == x[2] and lo[v] == x[3] for v, x in zip(pick, res))
        worst = max([worst] + [max(abs(int(w[v]) - x[2]), abs(int(lo[v]) - x[3])) for v, x in zip(pick, res)])

    def stat(t):
        return {"median_ms": float(np.median(t)), "min_ms": float(np.min(t)), "max_ms": float(np.max(t))}
    w = wrong.cpu().numpy()
    nact, pw = int(truth.sum()), (N + 63) // 64
    res = {"servers": N, "keys": B, "views": N, "active_views": nact, "kills": int(len(killed)),
           "sim_rounds": a.sim_rounds, "suspicion_rounds": a.suspicion, "composed_views": int(len(pick)),
           "views_that_differ_from_the_truth": int(len(differ)), "wrong_total": int(w.sum()),
           "lost_total": int(lost.sum().item()), "rounds": a.rounds, "counts_identical": bool(identical),
           "largest_count_difference": int(worst), "names_replaced_for_distinct_tokens": int(replaced),
           "fused": stat(t_fused), "composition_lookup_compare": stat(t_look), "composition_rebuild": stat(t_rebuild)}
    res["fused_us_per_view"] = res["fused"]["median_ms"] * 1e3 / nact
    res["composition_lookup_compare_us_per_view"] = res["composition_lookup_compare"]["median_ms"] * 1e3 / len(pick)
    res["composition_rebuild_us_per_view"] = res["composition_rebuild"]["median_ms"] * 1e3 / len(pick)
    res["fused_over_composition_per_view"] = res["fused_us_per_view"] / res["composition_lookup_compare_us_per_view"]
    # the issue's traffic model (nothing in it is measured): one plane row a key and step at 8.6 TB/s
    step_bytes = B * pw * 8
    res["model"] = {"plane_bytes": N * pw * 8, "bytes_per_step": step_bytes, "ms_per_step_at_8.6TBs": step_bytes / 8.6e9,
                    "pack_read_bytes": N * N}
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    if not identical:
        sys.exit("the fused counts and the composition disagree")


if __name__ == "__main__":
    main()
