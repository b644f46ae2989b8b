"""Which kernels the ring's key passes launch for every key form, launch by launch.

    rocprofv3 --kernel-trace --output-format csv -d DIR -o run -- python tools/ring_pass_kernels.py run
    python tools/ring_pass_kernels.py list DIR > kernels.txt

`run` builds a 64-server ring, snapshots it, adds one server and removes one, and then calls, over
the six key forms of tests/ring_key_forms.py (36-byte keys at a 16-byte, a 4-byte and an odd base,
offsets, stride 20 through the device entry points, caller hashes through the host ones):
moved keys, then the hand-off plan, for nrep in -2, 0, 1, 3, 4, 5, 8 and n in 1, 1023, 1024, 1025,
2055; the routing agreement under three views with and without the per-view owners for n in 1, 257,
2055; the owner load of 2,055 keys in chunks of 1,024 (RP_LOAD_CHUNK) for the aligned, the offsets and
the hashes form. It checks no result, only that every call returns, and closes every section with
a one-key k_gen_uuid launch that marks its end in the trace. `list` takes name, grid, workgroup
and LDS size of every launch of the library's (what PyTorch launches itself is left out) and prints
each distinct launch once, numbered by first use, then every section's launches in order as
those numbers. Equal files from two builds mean equal kernel choices, launch for launch.
"""
import csv
import ctypes
import glob
import os
import re
import sys
import textwrap

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NREPS = (-2, 0, 1, 3, 4, 5, 8)
SECTIONS = ("moved", "handoff", "route", "load")


def run():
    import numpy as np
    import torch

    sys.path[:0] = [REPO, os.path.join(REPO, "oracle"), os.path.join(REPO, "tests")]
    import bench
    import ring_key_forms as kf

    rpa = bench.load_pkg()
    L = rpa.lib()
    names = [bench.c2_addr(i) for i in range(65)]
    ring = rpa.HashRing()
    ring.addRemoveServers(names[:64])
    snap = ring.snapshot()
    ring.addRemoveServers(names[64:], names[8:9])
    idb = ring.id_bound()
    mark = torch.empty(64, dtype=torch.uint8, device="cuda")
    out = torch.empty(2055 * 8 * 4 + 2 * idb + 64, dtype=torch.int32, device="cuda")  # every device output
    host = np.empty(2055 * 8 * 4 + 2 * idb + 64, dtype=np.uint32)
    u32 = ctypes.c_uint32

    def end(section):
        torch.cuda.synchronize()
        rpa.gen_uuid_keys_dev(42, 0, 1, mark.data_ptr())
        torch.cuda.synchronize()
        print(section, "ok", flush=True)

    def sides(n):
        return [(form,) + kf.device_side(form, n) for form in kf.FORMS]

    o, h = out.data_ptr(), host.ctypes.data
    for n in (1, 1023, 1024, 1025, 2055):
        for form, ptr, extra, keep in sides(n):
            for nrep in NREPS:
                w = max(nrep, 1)
                if form == "hashes":
                    c = u32()
                    rpa.check(L.rp_ring_moved_hashes(ring._h, snap._h, keep.ctypes.data, n, nrep, n, h, h + 4 * n,
                                                     h + 4 * n * (1 + w), ctypes.byref(c)))
                else:
                    ring.moved_dev(snap, ptr, n, nrep, n, o, o + 4 * n, o + 4 * n * (1 + w), o + 4 * n * (1 + 2 * w),
                                   **extra)
            torch.cuda.synchronize()
    end("moved")
    for n in (1, 1023, 1024, 1025, 2055):
        for form, ptr, extra, keep in sides(n):
            for nrep in NREPS:
                m = n * max(nrep, 1)  # records at most; dests and group_off after the three record columns
                if form == "hashes":
                    c, nd = u32(), u32()
                    rpa.check(L.rp_ring_handoff_hashes(ring._h, snap._h, keep.ctypes.data, n, nrep, 0xFFFFFFFF, m,
                                                       h + 12 * m, h + 12 * m + 4 * idb, h, h + 4 * m, h + 8 * m,
                                                       ctypes.byref(nd), ctypes.byref(c)))
                else:
                    ring.handoff_dev(snap, ptr, n, nrep, m, o + 12 * m, o + 12 * m + 4 * idb, o, o + 4 * m, o + 8 * m,
                                     o + 12 * m + 8 * idb + 8, o + 12 * m + 8 * idb + 12, **extra)
            torch.cuda.synchronize()
    end("handoff")
    V = 3
    rows = torch.ones((V, idb), dtype=torch.uint8, device="cuda")
    rows[1, ::2] = 0
    rows[2, 1::3] = 0
    wrong = torch.zeros(2 * V, dtype=torch.int64, device="cuda")
    for n in (1, 257, 2055):
        for form, ptr, extra, keep in sides(n):
            if form == "hashes":
                hs = torch.from_numpy(np.array(keep).view(np.int32)).cuda()
                extra = {"hashes_ptr": hs.data_ptr(), "stride": 0}
            for owners in (False, True):
                ring.route_views_dev(n, rows.data_ptr(), idb, V, keys_ptr=ptr, wrong_ptr=wrong.data_ptr(),
                                     lost_ptr=wrong.data_ptr() + 8 * V, key_wrong_ptr=o, truth_owner_ptr=o + 4 * n,
                                     owners_ptr=o + 8 * n if owners else None, **extra)
            torch.cuda.synchronize()
    end("route")
    os.environ["RP_LOAD_CHUNK"] = "1024"
    load = torch.zeros(idb * 3, dtype=torch.int64, device="cuda")
    for form, ptr, extra, keep in sides(2055):
        if form == "hashes":
            ring.owner_load_hashes(keep, 3)
        elif form in ("aligned", "offsets"):
            ring.owner_load_dev(ptr, 2055, 3, load.data_ptr(), idb, **extra)
        torch.cuda.synchronize()
    os.environ.pop("RP_LOAD_CHUNK")
    end("load")
    print("%d sections done" % len(SECTIONS))


def listing(trace_dir):
    files = glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True)
    assert len(files) == 1, files
    rows = list(csv.DictReader(open(files[0])))
    rows.sort(key=lambda r: int(r["Dispatch_Id"]))

    def dims(r, what):
        if what in r:
            return r[what]
        return "x".join(r[what + "_" + a] for a in "XYZ")

    number, per = {}, [[]]
    for r in rows:
        name = re.sub(r"^void ", "", r["Kernel_Name"])
        if "at::" in name or "at_cuda" in name:  # PyTorch's own (fills, copies)
            continue
        name = re.sub(r"^(\w+::|\(anonymous namespace\)::)*", "", name)
        if name.endswith(")"):  # drop the parameter list: back to the bracket that closes last
            depth, i = 0, len(name)
            while i > 0 and (depth or i == len(name)):
                i -= 1
                depth += {")": 1, "(": -1}.get(name[i], 0)
            name = name[:i]
        if name.startswith("k_gen_uuid"):
            per.append([])
            continue
        launch = " ".join((name, dims(r, "Grid_Size"), dims(r, "Workgroup_Size"),
                           r.get("LDS_Block_Size", r.get("Group_Segment_Size"))))
        per[-1].append(number.setdefault(launch, len(number) + 1))
    assert len(per) == len(SECTIONS) + 1 and not per[-1], (len(per), len(SECTIONS))
    print("%d launches, %d distinct, %d sections" % (sum(map(len, per)), len(number), len(SECTIONS)))
    for launch, k in number.items():
        print(k, launch)
    for section, seq in zip(SECTIONS, per):
        print()
        print(section, len(seq))
        print(textwrap.fill(" ".join(map(str, seq)), 100, initial_indent="  ", subsequent_indent="  "))


if __name__ == "__main__":
    if sys.argv[1:2] == ["run"]:
        run()
    elif sys.argv[1:2] == ["list"] and len(sys.argv) == 3:
        listing(sys.argv[2])
    else:
        sys.exit(__doc__)
