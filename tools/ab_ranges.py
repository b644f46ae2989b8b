"""A/B timing of the fused moved-ranges call against the composition a caller needs without it, in
ONE process, the two legs alternating, after a warm-up.

    python tools/ab_ranges.py [--servers 10000] [--churn 10] [--n 3 1] [--reps 21]

The configuration is the C2 ring (10k servers x 100 points); a snapshot is taken, then `churn`
servers are removed and `churn` added. A twin ring that stays at the state before the change
stands for "the ring before the change" in the composition (a snapshot had no dump).

  fused        rp_ring_moved_ranges with host outputs: one device pass over the two token sets,
               the ranges come back
  composition  today's public calls: dump() of the ring before the change and of the ring now,
               np.union1d of the two token arrays (2^32-1 appended), rp_ring_moved_hashes over the
               union, and a numpy pass that turns the moved union values into intervals and joins
               neighbours that touch and carry the same rows

Both produce lo, hi and the two row arrays; the tool checks that they are identical before it
reports. Host legs are wall-clock (both end synchronised with the device); the _dev form alone is
timed with HIP events. Prints one JSON object with the medians.
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402

TOP = 0xFFFFFFFF


def composition(rpa, before_ring, ring, snap, n):
    w = max(n, 1)
    tb, _ = before_ring.dump()
    ta, _ = ring.dump()
    u = np.union1d(np.union1d(tb, ta), np.array([TOP], dtype=np.uint32))
    idx = np.empty(len(u), dtype=np.uint32)
    br = np.empty((len(u), w), dtype=np.uint32)
    ar = np.empty((len(u), w), dtype=np.uint32)
    c = ctypes.c_uint32()
    rpa.check(rpa.lib().rp_ring_moved_hashes(ring._h, snap._h, u.ctypes.data, len(u), n, len(u), idx.ctypes.data,
                                             br.ctypes.data, ar.ctypes.data, ctypes.byref(c)))
    m = c.value
    idx, br, ar = idx[:m].astype(np.int64), br[:m], ar[:m]
    hi = u[idx]
    lo = np.where(idx > 0, u[np.maximum(idx - 1, 0)].astype(np.int64) + 1, 0).astype(np.uint32)
    cont = np.zeros(m, dtype=bool)  # interval j continues j - 1: they touch and carry the same rows
    if m > 1:
        cont[1:] = (idx[1:] == idx[:-1] + 1) & (br[1:] == br[:-1]).all(axis=1) & (ar[1:] == ar[:-1]).all(axis=1)
    head = ~cont
    tail = np.ones(m, dtype=bool)
    tail[:-1] = head[1:]
    return lo[head], hi[tail], br[head], ar[head]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--servers", type=int, default=10000)
    ap.add_argument("--churn", type=int, default=10)
    ap.add_argument("--n", type=int, nargs="+", default=[3, 1])
    ap.add_argument("--reps", type=int, default=21)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("ab_ranges.py needs a HIP device (there is no CPU fallback)")
    rpa = bench.load_pkg()
    names = [bench.c2_addr(i) for i in range(a.servers + a.churn)]
    ring, before_ring = rpa.HashRing(), rpa.HashRing()
    ring.addRemoveServers(names[:a.servers])
    before_ring.addRemoveServers(names[:a.servers])
    snap = ring.snapshot()
    step = max(a.servers // max(a.churn, 1), 1)
    ring.addRemoveServers(names[a.servers:], names[:a.servers:step][:a.churn])
    bound = snap.info()["tokens"] + ring.size + 1
    st = torch.cuda.current_stream()
    res = {"servers": a.servers, "churn": a.churn, "tokens_before": snap.info()["tokens"], "tokens_now": ring.size,
           "reps": a.reps, "runs": {}}
    ok = True
    for n in a.n:
        w = max(n, 1)
        d_lo = torch.empty(bound, dtype=torch.int32, device="cuda")
        d_hi = torch.empty(bound, dtype=torch.int32, device="cuda")
        d_br = torch.empty((bound, w), dtype=torch.int32, device="cuda")
        d_ar = torch.empty((bound, w), dtype=torch.int32, device="cuda")
        d_cnt = torch.zeros(1, dtype=torch.int32, device="cuda")
        d_mh = torch.zeros(1, dtype=torch.int64, device="cuda")
        got = {}

        def fused():
            got["fused"] = ring.moved_range_ids(snap, n)

        def comp():
            got["composition"] = composition(rpa, before_ring, ring, snap, n)

        variants = {"fused": fused, "composition": comp}
        times = {k: [] for k in variants}
        dev = []
        for r in range(a.reps + 2):  # rounds 0 and 1 warm every buffer up and are not timed
            order = list(variants) if r % 2 == 0 else list(variants)[::-1]
            for name in order:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                variants[name]()
                t1 = time.perf_counter()
                if r > 1:
                    times[name].append((t1 - t0) * 1e3)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            ring.moved_ranges_dev(snap, n, bound, d_lo.data_ptr(), d_hi.data_ptr(), d_br.data_ptr(), d_ar.data_ptr(),
                                  d_cnt.data_ptr(), d_mh.data_ptr(), stream=st.cuda_stream)
            e1.record(st)
            torch.cuda.synchronize()
            if r > 1:
                dev.append(e0.elapsed_time(e1))
        same = all(np.array_equal(x, y) for x, y in zip(got["fused"], got["composition"]))
        count = int(d_cnt.item())
        same = same and count == len(got["fused"][0]) == ring.moved_range_count
        same = same and np.array_equal(d_lo[:count].cpu().numpy().view(np.uint32), got["fused"][0])
        same = same and np.array_equal(d_hi[:count].cpu().numpy().view(np.uint32), got["fused"][1])
        ok = ok and same
        run = {"ranges": ring.moved_range_count, "moved_hashes": ring.moved_hash_count,
               "moved_share": ring.moved_hash_count / 2.0 ** 32, "results_identical": bool(same)}
        for name, t in times.items():
            run[name] = {"median_ms": float(np.median(t)), "min_ms": float(np.min(t)), "max_ms": float(np.max(t))}
        run["dev_only"] = {"median_ms": float(np.median(dev)), "min_ms": float(np.min(dev)),
                           "max_ms": float(np.max(dev))}
        run["fused_over_composition"] = run["fused"]["median_ms"] / run["composition"]["median_ms"]
        res["runs"]["n%d" % n] = run
    print(json.dumps(res, indent=1))
    if not ok:
        sys.exit("the fused ranges and the composition disagree")


if __name__ == "__main__":
    main()
