"""A/B timing of the owner-load call against the lookup alone and against the composition a
caller needs without it, in ONE process, alternating, HIP-event timed.

    python tools/ab_load.py [--log2 26] [--n 3] [--rounds 7] [--out profiles/owner_load/ab_load.json]

Shape A: the C2 ring (10k servers x 100 points), 2^26 device UUID keys, lookupN(3).
Shape B: the same keys on a 3-server ring (every lane of a wave adds to the same few bins).

  load         rp_ring_owner_load_dev: chunks of rows into the handle's scratch, counted in LDS
  lookup       rp_ring_lookupn_dev alone on the same keys (the floor: every key is looked up)
  composition  rp_ring_lookupn_dev into full rows (keys x n x 4 B) + torch.bincount of the flat bins
  load_nocopy  (shape B) load with RP_LOAD_COPIES=0: one copy of the bin window in LDS
  load_c<k>    (shape A) load with RP_LOAD_CHUNK = 2^k keys, k = 20..24

load and composition must give identical counts; the tool checks before it reports. Writes one
JSON object: median / min / max ms of each variant, load / lookup and load / composition, and the
extra device memory of load (the device's free memory around its first call) and of composition
(torch's peak allocation over one call).
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import bench  # noqa: E402


def run_shape(rpa, servers, keys, B, n, rounds, sweep, nocopy):
    st = torch.cuda.current_stream()
    W = max(n, 1)
    ring = rpa.HashRing()
    ring.addRemoveServers([bench.c2_addr(i) for i in range(servers)])
    cap = ring.id_bound()
    load = torch.zeros(cap * W, dtype=torch.int64, device="cuda")
    rows = torch.empty((B, W), dtype=torch.int32, device="cuda")
    q = torch.arange(W, dtype=torch.int64, device="cuda")
    got = {}

    def f_load():
        ring.owner_load_dev(keys.data_ptr(), B, n, load.data_ptr(), cap, stream=st.cuda_stream)

    def f_lookup():
        ring.lookupn_dev(keys.data_ptr(), B, n, rows.data_ptr(), None, 36, None, st.cuda_stream)

    def f_comp():
        ring.lookupn_dev(keys.data_ptr(), B, n, rows.data_ptr(), None, 36, None, st.cuda_stream)
        got["composition"] = torch.bincount((rows.long() * W + q).view(-1), minlength=cap * W)

    def with_env(name, value, f):
        def g():
            os.environ[name] = value
            try:
                f()
            finally:
                del os.environ[name]
        return g

    # the extra device memory of each side, before anything is warm
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    f_load()
    torch.cuda.synchronize()
    load_extra = free0 - torch.cuda.mem_get_info()[0]
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    f_comp()
    torch.cuda.synchronize()
    comp_extra = torch.cuda.max_memory_allocated() - base + rows.numel() * 4
    same = bool((got["composition"] == load).all().item()) and int(load.view(-1, W)[:, 0].sum().item()) == B

    variants = {"load": f_load, "lookup": f_lookup, "composition": f_comp}
    if nocopy:
        variants["load_nocopy"] = with_env("RP_LOAD_COPIES", "0", f_load)
    for k in sweep:
        variants["load_c%d" % k] = with_env("RP_LOAD_CHUNK", str(1 << k), f_load)
    times = {k: [] for k in variants}
    for r in range(rounds + 1):  # round 0 warms every shape up and is not timed
        order = list(variants) if r % 2 == 0 else list(variants)[::-1]
        for name in order:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            variants[name]()
            e1.record(st)
            torch.cuda.synchronize()
            if r:
                times[name].append(e0.elapsed_time(e1))
            if name.startswith("load"):
                same = same and bool((got["composition"] == load).all().item())
    res = {"servers": servers, "keys": B, "n": n, "bins": cap * W, "results_identical": same,
           "load_extra_device_bytes": int(load_extra), "composition_extra_device_bytes": int(comp_extra)}
    for name, t in times.items():
        res[name] = {"median_ms": float(np.median(t)), "min_ms": float(np.min(t)), "max_ms": float(np.max(t))}
    res["load_over_lookup"] = res["load"]["median_ms"] / res["lookup"]["median_ms"]
    res["load_over_composition"] = res["load"]["median_ms"] / res["composition"]["median_ms"]
    ring.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2", type=int, default=26)
    ap.add_argument("--n", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "owner_load", "ab_load.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("ab_load.py needs a HIP device (there is no CPU fallback)")
    rpa = bench.load_pkg()
    B = 1 << a.log2
    keys = torch.empty(B * 36, dtype=torch.uint8, device="cuda")
    rpa.gen_uuid_keys_dev(42, 0, B, keys.data_ptr(), torch.cuda.current_stream().cuda_stream)
    res = {"A": run_shape(rpa, 10000, keys, B, a.n, a.rounds, [k for k in range(20, 25) if k <= a.log2], False),
           "B": run_shape(rpa, 3, keys, B, a.n, a.rounds, [], True)}
    text = json.dumps(res, indent=1)
    print(text)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    if not (res["A"]["results_identical"] and res["B"]["results_identical"]):
        sys.exit("the owner load and the composition disagree")


if __name__ == "__main__":
    main()
