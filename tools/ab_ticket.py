"""A/B of the schedules of the 256-thread sorted tiles at C2 in ONE process (lookupN(3), 2^26 keys).

    python tools/ab_ticket.py [--out FILE] [--forms JSON]

The forms alternate launch by launch, 30 launches each; a form's figure is the mean of its last
10 launches (HIP events around the whole call: the sorted kernel and the fix pass), next to their
min and max. Every form's owners are compared with the first form's (digest of the whole output).
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402

KNOBS = ("RP_LOOKUP_GRID", "RP_LOOKUP_TICKET", "RP_LOOKUP_STAGGER", "RP_LOOKUP_TICKET_GRID", "RP_LOOKUP_SORT")
FORMS = {
    "strided 4096": {"RP_LOOKUP_TICKET": "0"},
    "ticket": {"RP_LOOKUP_TICKET": "1", "RP_LOOKUP_STAGGER": "0"},
    "ticket stagger 1/8": {"RP_LOOKUP_TICKET": "1", "RP_LOOKUP_STAGGER": "2"},
    "ticket stagger 1/4": {"RP_LOOKUP_TICKET": "1", "RP_LOOKUP_STAGGER": "4"},
    "ticket stagger 1/2": {"RP_LOOKUP_TICKET": "1", "RP_LOOKUP_STAGGER": "8"},
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--forms", default="")
    ap.add_argument("--launches", type=int, default=30)
    ap.add_argument("--log2", type=int, default=26)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    forms = json.loads(a.forms) if a.forms else FORMS
    rpa = bench.load_pkg()
    ring = rpa.HashRing()
    ring.addRemoveServers([bench.c2_addr(i) for i in range(10000)])
    B = 1 << a.log2
    st = torch.cuda.current_stream()
    keys = torch.empty(B * 36, dtype=torch.uint8, device="cuda")
    rpa.gen_uuid_keys_dev(42, 0, B, keys.data_ptr(), st.cuda_stream)
    out = torch.empty(B * 3, dtype=torch.int32, device="cuda")
    w = torch.arange(B * 3, device="cuda") % 1009 + 1
    times = {k: [] for k in forms}
    digests = {}
    for r in range(a.launches):
        for name, env in forms.items():
            for kn in KNOBS:
                os.environ.pop(kn, None)
            os.environ.update(env)
            if r == 0:
                out.fill_(-2)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            ring.lookupn_dev(keys.data_ptr(), B, 3, out.data_ptr(), None, 36, None, st.cuda_stream)
            e1.record(st)
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1))
            if r == 0:
                digests[name] = int(torch.sum(out.long() * w).item())
    for kn in KNOBS:
        os.environ.pop(kn, None)
    first = next(iter(forms))
    res = {}
    for name, t in times.items():
        last = np.asarray(t[-10:])
        res[name] = {"env": forms[name], "mean_last10_ms": round(float(last.mean()), 4), "min_ms": round(float(last.min()), 4),
                     "max_ms": round(float(last.max()), 4), "G_lookupN3_s": round(B / float(last.mean()) / 1e6, 2),
                     "same_owners_as_" + first: digests[name] == digests[first]}
    txt = json.dumps(res, indent=1)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
