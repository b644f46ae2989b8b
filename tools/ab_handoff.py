"""A/B timing of the fused hand-off call against the composition a caller needs without it, in ONE
process, legs alternating, HIP-event timed.

    python tools/ab_handoff.py [--servers 10000] [--log2 26] [--n 3] [--churn 10] [--rounds 7] [--out FILE]

The configuration is the C2 ring (10k servers x 100 points), 2^26 device UUID keys, lookupN(3);
a snapshot is taken, then `churn` servers are removed and `churn` added.

  a  handoff          rp_ring_handoff_dev with cap = 1.25 x count (count from a count-only call)
  b  composition      rp_ring_moved_keys_dev with both rows, then torch: gained mask, in-ring gather
                      for src, nonzero, stable sort by dst, run heads
  c  moved_keys       rp_ring_moved_keys_dev alone (both rows)
  d  handoff_count    rp_ring_handoff_dev with cap = 0 (the key pass alone)
  a8 handoff_cap8     leg a with cap = 8 x count (the _dev grouping runs over cap slots)

Legs a and b both produce the grouped plan; the tool checks in every round that they are identical
(and that a8 equals a) before it reports. Prints one JSON object: median / min / max ms of each leg
and the two ratios a / b and d / c.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402

NIL = 0xFFFFFFFF


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--servers", type=int, default=10000)
    ap.add_argument("--log2", type=int, default=26)
    ap.add_argument("--n", type=int, default=3)
    ap.add_argument("--churn", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("ab_handoff.py needs a HIP device (there is no CPU fallback)")
    rpa = bench.load_pkg()
    names = [bench.c2_addr(i) for i in range(a.servers + a.churn)]
    ring = rpa.HashRing()
    ring.addRemoveServers(names[:a.servers])
    snap = ring.snapshot()
    step = max(a.servers // max(a.churn, 1), 1)
    ring.addRemoveServers(names[a.servers:], names[:a.servers:step][:a.churn])
    B, W = 1 << a.log2, max(a.n, 1)
    bound = ring.id_bound()
    st = torch.cuda.current_stream()
    keys = torch.empty(B * 36, dtype=torch.uint8, device="cuda")
    rpa.gen_uuid_keys_dev(42, 0, B, keys.data_ptr(), st.cuda_stream)
    inring = torch.zeros(bound + 1, dtype=torch.bool, device="cuda")  # (entry `bound`: the null id)
    inring[torch.from_numpy(ring.server_ids().astype(np.int64)).cuda()] = True
    cnt = torch.zeros(2, dtype=torch.int32, device="cuda")

    # the count-only call sizes every buffer
    ring.handoff_dev(snap, keys.data_ptr(), B, a.n, 0, None, None, None, None, None, cnt[1:].data_ptr(),
                     cnt.data_ptr(), stream=st.cuda_stream)
    count = int(cnt[0].item())
    ring.moved_dev(snap, keys.data_ptr(), B, a.n, 0, None, None, None, cnt.data_ptr(), stream=st.cuda_stream)
    moved = int(cnt[0].item())
    cap, cap8 = count + count // 4 + 1, 8 * count + 1
    i32 = lambda k: torch.empty(max(k, 1), dtype=torch.int32, device="cuda")  # noqa: E731
    out = {c: {"dests": i32(min(c, bound)), "goff": i32(min(c, bound) + 1), "key": i32(c), "src": i32(c),
               "slot": torch.empty(c, dtype=torch.uint8, device="cuda"), "cnt": torch.zeros(2, dtype=torch.int32,
                                                                                            device="cuda")}
           for c in (cap, cap8)}
    idx, brow, arow = i32(moved), i32(moved * W), i32(moved * W)
    got = {}

    def handoff_at(c):
        o = out[c]
        ring.handoff_dev(snap, keys.data_ptr(), B, a.n, c, o["dests"].data_ptr(), o["goff"].data_ptr(),
                         o["key"].data_ptr(), o["src"].data_ptr(), o["slot"].data_ptr(), o["cnt"][1:].data_ptr(),
                         o["cnt"].data_ptr(), stream=st.cuda_stream)
        return o

    def leg_a():
        got["a"] = handoff_at(cap)

    def leg_a8():
        got["a8"] = handoff_at(cap8)

    def moved_rows():
        ring.moved_dev(snap, keys.data_ptr(), B, a.n, moved, idx.data_ptr(), brow.data_ptr(), arow.data_ptr(),
                       cnt.data_ptr(), stream=st.cuda_stream)

    def leg_b():
        moved_rows()
        m = int(cnt[0].item())  # (the caller has to know how many rows came back)
        br = brow[:m * W].view(m, W).long() & NIL
        ar = arow[:m * W].view(m, W).long() & NIL
        gained = (ar != NIL) & ~(ar[:, :, None] == br[:, None, :]).any(dim=2)
        live = inring[torch.clamp(br, max=bound)]
        first = live.int().argmax(dim=1, keepdim=True)
        src = torch.where(live.any(dim=1), br.gather(1, first).flatten(), torch.full_like(first.flatten(), NIL))
        k, q = torch.nonzero(gained, as_tuple=True)  # (key, slot) order
        dst = ar[k, q]
        sd, order = torch.sort(dst, stable=True)
        dests, sizes = torch.unique_consecutive(sd, return_counts=True)
        goff = torch.cat([torch.zeros(1, dtype=torch.long, device="cuda"), sizes.cumsum(0)])
        got["b"] = {"dests": dests, "goff": goff, "key": idx[:m].long()[k][order], "src": src[k][order],
                    "slot": q[order]}

    def leg_c():
        moved_rows()

    def leg_d():
        ring.handoff_dev(snap, keys.data_ptr(), B, a.n, 0, None, None, None, None, None, cnt[1:].data_ptr(),
                         cnt.data_ptr(), stream=st.cuda_stream)

    def same(x, b):
        """A device result (int32 buffers + counts) against the composition's tensors."""
        t, nd = int(x["cnt"][0].item()), int(x["cnt"][1].item())
        u = lambda v: v.long() & NIL  # noqa: E731
        return (t == count == int(b["key"].numel()) and nd == int(b["dests"].numel())
                and bool((u(x["dests"][:nd]) == b["dests"]).all()) and bool((u(x["goff"][:nd + 1]) == b["goff"]).all())
                and bool((u(x["key"][:t]) == b["key"]).all()) and bool((u(x["src"][:t]) == b["src"]).all())
                and bool((x["slot"][:t].long() == b["slot"]).all()))

    legs = {"handoff": leg_a, "composition": leg_b, "moved_keys": leg_c, "handoff_count": leg_d,
            "handoff_cap8": leg_a8}
    times = {k: [] for k in legs}
    identical = True
    for r in range(a.rounds + 1):  # round 0 warms every shape up and is not timed
        order = list(legs) if r % 2 == 0 else list(legs)[::-1]
        for name in order:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            legs[name]()
            e1.record(st)
            torch.cuda.synchronize()
            if r:
                times[name].append(e0.elapsed_time(e1))
        identical = identical and same(got["a"], got["b"]) and same(got["a8"], got["b"])
    res = {"servers": a.servers, "keys": B, "n": a.n, "churn": a.churn, "moved": moved, "transfers": count,
           "destinations": int(got["b"]["dests"].numel()), "cap": cap, "cap8": cap8, "rounds": a.rounds,
           "results_identical": identical}
    for name, t in times.items():
        res[name] = {"median_ms": float(np.median(t)), "min_ms": float(np.min(t)), "max_ms": float(np.max(t)),
                     "Gkeys_s": B / float(np.median(t)) / 1e6}
    res["handoff_over_composition"] = res["handoff"]["median_ms"] / res["composition"]["median_ms"]
    res["handoff_count_over_moved_keys"] = res["handoff_count"]["median_ms"] / res["moved_keys"]["median_ms"]
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    if not identical:
        sys.exit("the fused plan and the composition disagree")


if __name__ == "__main__":
    main()
