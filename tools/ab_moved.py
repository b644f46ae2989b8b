"""A/B timing of the fused moved-keys call against the composition a caller needs without it, in
ONE process, alternating, HIP-event timed.

    python tools/ab_moved.py [--servers 10000] [--log2 26] [--n 3] [--churn 10] [--rounds 7]

The configuration is the C2 ring (10k servers x 100 points), 2^26 device UUID keys, lookupN(3);
a snapshot is taken, then `churn` servers are removed and `churn` added.

  fused        rp_ring_moved_keys_dev: one pass over the keys, rows written for moved keys only
  composition  rp_ring_lookupn_dev on the ring now + rp_ring_snap_lookupn_dev on the snapshot
               (two passes over the keys, 2 x n x 4 B of rows per key written and read back),
               then a torch row compare and nonzero

Both produce the moved key indices; the tool checks that they are identical before it reports.
Prints one JSON object: median / min ms of each, their ratio, the moved share.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--servers", type=int, default=10000)
    ap.add_argument("--log2", type=int, default=26)
    ap.add_argument("--n", type=int, default=3)
    ap.add_argument("--churn", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=7)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("ab_moved.py needs a HIP device (there is no CPU fallback)")
    rpa = bench.load_pkg()
    names = [bench.c2_addr(i) for i in range(a.servers + a.churn)]
    ring = rpa.HashRing()
    ring.addRemoveServers(names[:a.servers])
    snap = ring.snapshot()
    step = max(a.servers // max(a.churn, 1), 1)
    ring.addRemoveServers(names[a.servers:], names[:a.servers:step][:a.churn])
    B, W = 1 << a.log2, max(a.n, 1)
    st = torch.cuda.current_stream()
    keys = torch.empty(B * 36, dtype=torch.uint8, device="cuda")
    rpa.gen_uuid_keys_dev(42, 0, B, keys.data_ptr(), st.cuda_stream)
    now = torch.empty((B, W), dtype=torch.int32, device="cuda")
    was = torch.empty((B, W), dtype=torch.int32, device="cuda")
    idx = torch.empty(B, dtype=torch.int32, device="cuda")
    brow = torch.empty((B, W), dtype=torch.int32, device="cuda")
    arow = torch.empty((B, W), dtype=torch.int32, device="cuda")
    cnt = torch.zeros(1, dtype=torch.int32, device="cuda")
    got = {}

    def fused():
        ring.moved_dev(snap, keys.data_ptr(), B, a.n, B, idx.data_ptr(), brow.data_ptr(), arow.data_ptr(),
                       cnt.data_ptr(), stream=st.cuda_stream)
        got["fused"] = (idx, cnt)

    def composition():
        ring.lookupn_dev(keys.data_ptr(), B, a.n, now.data_ptr(), None, 36, None, st.cuda_stream)
        snap.lookupn_dev(keys.data_ptr(), B, a.n, was.data_ptr(), None, 36, None, st.cuda_stream)
        got["composition"] = torch.nonzero((now != was).any(dim=1)).flatten()

    variants = {"fused": fused, "composition": composition}
    times = {k: [] for k in variants}
    for r in range(a.rounds + 1):  # round 0 warms every shape up and is not timed
        order = list(variants) if r % 2 == 0 else list(variants)[::-1]
        for name in order:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            variants[name]()
            e1.record(st)
            torch.cuda.synchronize()
            if r:
                times[name].append(e0.elapsed_time(e1))
    moved = int(got["fused"][1].item())
    want = got["composition"]
    same = moved == int(want.numel()) and bool((got["fused"][0][:moved].long() == want).all().item())
    if same and moved:
        same = bool((brow[:moved] == was[want]).all().item()) and bool((arow[:moved] == now[want]).all().item())
    res = {"servers": a.servers, "keys": B, "n": a.n, "churn": a.churn, "moved": moved, "moved_share": moved / B,
           "results_identical": same}
    for name, t in times.items():
        res[name] = {"median_ms": float(np.median(t)), "min_ms": float(np.min(t)),
                     "max_ms": float(np.max(t)), "Gkeys_s": B / float(np.median(t)) / 1e6}
    res["fused_over_composition"] = res["fused"]["median_ms"] / res["composition"]["median_ms"]
    print(json.dumps(res, indent=1))
    if not same:
        sys.exit("the fused list and the composition disagree")


if __name__ == "__main__":
    main()
