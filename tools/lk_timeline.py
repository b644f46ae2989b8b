"""Timeline of one sorted-tile lookupN(3) launch on the C2 ring (diagnostics).

    DEFS=-DRP_LK_PROF OUT=librpamd_lkprof.so tools/build_prof.sh
    RP_AMD_LIB=ringpop-node_amd/librpamd_lkprof.so python tools/lk_timeline.py \
        --forms '{"strided 4096": {"RP_LOOKUP_GRID": "4096"}, "ticket": {"RP_LOOKUP_TICKET": "1"}}' --out DIR

A -DRP_LK_PROF build stamps, per workgroup of k_lookupn_sorted<256,3> (strided or ticketed), its
start, its end and the end of each of its tiles (s_memrealtime, 100 MHz) with its HW_ID and XCC_ID,
and writes them to the file RP_LK_TL_DUMP names. For each form this runs warm-up launches over
2^26 keys, then one stamped launch, keeps its dump as DIR/<form>.tl.txt and prints:

  - running workgroups at the middle of each twentieth of the span;
  - the spread of the workgroups' durations, and the span from the first to the last workgroup end;
  - the order workgroups are dealt in: how many CUs the first blocks land on, and the slot
    (order of arrival on its CU) of every block against blockIdx / CUs;
  - per CU, at 1/4, 1/2 and 3/4 of the span, how far apart in phase its running workgroups are:
    phase = a workgroup's last tile-end stamp modulo the mean tile time; the figure is the
    shortest arc of the tile period that holds all of them, as a fraction of the period
    (0: in step; 0.75: four workgroups evenly apart; 0.48: four independent ones on average).
"""
import argparse
import json
import os
import sys
from collections import defaultdict

import numpy as np

KNOBS = ("RP_LOOKUP_GRID", "RP_LOOKUP_TICKET", "RP_LOOKUP_STAGGER", "RP_LOOKUP_TICKET_GRID", "RP_LOOKUP_SORT")


def read_dump(path):
    head, W, T = "", [], []
    with open(path) as f:
        for line in f:
            p = line.split()
            if p[0] == "#":
                head = line[2:].strip()
            elif p[0] == "W":
                W.append([int(x) for x in p[1:]])
            elif p[0] == "T":
                T.append([int(x) for x in p[1:]])
    return head, np.array(W, dtype=np.int64), np.array(T, dtype=np.int64)


def cu_of(hw, xcc):
    # HW_ID (gfx9): cu_id [11:8], sh_id [12], se_id [15:13]; XCC_ID [3:0]
    return ((xcc & 15) << 8) | (((hw >> 13) & 7) << 5) | (((hw >> 12) & 1) << 4) | ((hw >> 8) & 15)


def arc(phases):
    """Shortest arc of the unit circle holding all phases."""
    p = np.sort(np.asarray(phases) % 1.0)
    if len(p) < 2:
        return 0.0
    gaps = np.diff(np.concatenate([p, [p[0] + 1.0]]))
    return float(1.0 - gaps.max())


def analyse(path, out=sys.stdout):
    head, W, T = read_dump(path)
    pr = lambda *a: print(*a, file=out)  # noqa: E731
    b, hw, xcc, start, end = W.T
    ran = end > 0
    t0, t1 = start[ran].min(), end[ran].max()
    span = t1 - t0
    us = lambda ticks: ticks / 100.0  # noqa: E731
    pr("launch: %s" % head)
    pr("workgroups %d, tiles %d, span %.1f us (first start to last end)" % (len(b), len(T), us(span)))
    mids = t0 + (np.arange(20) + 0.5) * span / 20
    pr("running workgroups by twentieth: %s" % " ".join(str(int(((start <= m) & (end > m)).sum())) for m in mids))
    dur = us(end - start)
    pr("workgroup duration us: min %.1f p5 %.1f median %.1f p95 %.1f max %.1f"
       % (dur.min(), np.percentile(dur, 5), np.median(dur), np.percentile(dur, 95), dur.max()))
    pr("workgroup starts: first to last %.1f us; first 1,024 within %.1f us"
       % (us(start.max() - start.min()), us(np.sort(start)[min(1023, len(start) - 1)] - start.min())))
    pr("workgroup ends: first to last %.1f us; last end after the median end %.1f us"
       % (us(end.max() - end.min()), us(end.max() - np.median(end))))
    # tiles per workgroup, tile times
    tiles_of = defaultdict(list)
    for t, wg, te in T:
        if te:
            tiles_of[wg].append(te)
    tt = []
    for wg, ends in tiles_of.items():
        e = np.sort(np.array(ends))
        tt.extend(np.diff(np.concatenate([[start[wg]], e])))
    tt = np.array(tt, dtype=np.float64)
    mean_tile = tt.mean()
    cnt = np.array([len(v) for v in tiles_of.values()])
    pr("tile time us: mean %.2f p5 %.2f median %.2f p95 %.2f; tiles a workgroup: min %d max %d"
       % (us(mean_tile), us(np.percentile(tt, 5)), us(np.median(tt)), us(np.percentile(tt, 95)), cnt.min(), cnt.max()))
    # dispatch order
    cu = np.array([cu_of(h, x) for h, x in zip(hw, xcc)])
    ncu = len(set(cu.tolist()))
    pr("CUs seen %d; XCC of blocks 0..15: %s" % (ncu, " ".join(str(int(x & 15)) for x in xcc[:16])))
    for n in (ncu, 2 * ncu, 4 * ncu):
        if n <= len(b):
            pr("blocks 0..%d land on %d distinct CUs" % (n - 1, len(set(cu[:n].tolist()))))
    first = min(len(b), 4 * ncu)
    slot = np.zeros(first, dtype=np.int64)
    seen = defaultdict(int)
    for i in np.argsort(start[:first], kind="stable"):
        slot[i] = seen[cu[i]]
        seen[cu[i]] += 1
    agree = float((slot == (np.arange(first) // ncu)).mean())
    pr("first %d blocks: arrival slot on the CU == blockIdx / CUs for %.1f %% of them" % (first, 100 * agree))
    # phase spread per CU
    for frac in (0.25, 0.5, 0.75):
        at = t0 + frac * span
        per_cu = defaultdict(list)
        for wg in np.nonzero((start <= at) & (end > at))[0]:
            e = np.array(tiles_of.get(wg, []))
            e = e[e <= at]
            last = e.max() if len(e) else start[wg]
            per_cu[cu[wg]].append((last % mean_tile) / mean_tile)
        arcs = np.array([arc(v) for v in per_cu.values() if len(v) >= 2])
        if len(arcs):
            pr("phase spread at %.2f of the span: %d CUs with >= 2 running; arc mean %.3f p10 %.3f median %.3f p90 %.3f; "
               "CUs with arc < 0.1: %d" % (frac, len(arcs), arcs.mean(), np.percentile(arcs, 10), np.median(arcs),
                                         np.percentile(arcs, 90), int((arcs < 0.1).sum())))
        else:
            pr("phase spread at %.2f of the span: no CU with two running workgroups" % frac)
    pr("")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--forms", default="")
    ap.add_argument("--out", default="bench_out/timeline")
    ap.add_argument("--log2", type=int, default=26)
    ap.add_argument("--warm", type=int, default=12)
    ap.add_argument("--analyse", nargs="*", default=None, help="only analyse these dump files")
    a = ap.parse_args()
    if a.analyse is not None:
        for p in a.analyse:
            analyse(p)
        return
    import torch

    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import bench

    forms = json.loads(a.forms)
    os.makedirs(a.out, exist_ok=True)
    rpa = bench.load_pkg()
    ring = rpa.HashRing()
    ring.addRemoveServers([bench.c2_addr(i) for i in range(10000)])
    B = 1 << a.log2
    st = torch.cuda.current_stream()
    keys = torch.empty(B * 36, dtype=torch.uint8, device="cuda")
    rpa.gen_uuid_keys_dev(42, 0, B, keys.data_ptr(), st.cuda_stream)
    owners = torch.empty(B * 3, dtype=torch.int32, device="cuda")
    with open(os.path.join(a.out, "timelines.txt"), "w") as report:
        for name, env in forms.items():
            for kn in KNOBS:
                os.environ.pop(kn, None)
            os.environ.update(env)
            path = os.path.join(a.out, name.replace(" ", "_") + ".tl.txt")
            ms = 0.0
            for i in range(a.warm + 1):
                if i == a.warm:
                    os.environ["RP_LK_TL_DUMP"] = path
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(st)
                ring.lookupn_dev(keys.data_ptr(), B, 3, owners.data_ptr(), None, 36, None, st.cuda_stream)
                e1.record(st)
                torch.cuda.synchronize()
                if i == a.warm - 1:
                    ms = e0.elapsed_time(e1)
            os.environ.pop("RP_LK_TL_DUMP", None)
            for f in (sys.stdout, report):
                print("== %s %s: %.4f ms the launch before the stamped one (diagnostics build)" % (name, json.dumps(env), ms),
                      file=f, flush=True)
                analyse(path, f)
    for kn in KNOBS:
        os.environ.pop(kn, None)


if __name__ == "__main__":
    main()
