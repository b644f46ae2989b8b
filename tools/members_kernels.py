"""Which kernels Membership.update, set and the checksum launch under every environment, launch by launch.

    rocprofv3 --kernel-trace --output-format csv -d DIR -o run -- python tools/members_kernels.py run
    python tools/members_kernels.py list DIR > kernels.txt

`run` plays one script under every environment of environments(): on 3,000 members with batches of
2,000 changes, plain device batches, a batch with an address of 17 changes (the overflow fold), an
empty batch, 500 names interned between batches, a Membership.set, a checksum read, a batch on a
second stream and twelve more batches (they wrap a pool of three or four slots); then a handle with
the checksum deferred, one with damp scoring and a ranged batch on a fourth. Under the environments
of LARGE it adds one batch of 2^19 changes over 2^19 members (the bucket path by size). The
environment `sorted-mid` sets RP_MEMBERS_SORTED_FOLD=1 for the batches marked so in the script and
for no other call. It checks no result, only that every call returns, and closes every environment
with a one-key k_gen_uuid launch that marks its end in the trace.

`list` takes name, grid, workgroup and LDS size of every launch of the library's (what PyTorch
launches itself is left out) and prints each distinct launch once, numbered by first use on a callers' stream, then every
environment's launches as those numbers: the callers' streams in launch order, and the side
streams (the chains' k_hash_long*, k_ck_commit and k_ck_hist, and k_mck_write under
RP_MEMBERS_SIDE_BUILD=1) as a sorted list, since they run beside the callers' and their place in
the trace is not fixed. Equal files from two builds mean equal kernel choices, launch for launch.
"""
import csv
import glob
import os
import re
import sys
import textwrap

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KNOBS = ("RP_MEMBERS_SORTED_FOLD", "RP_MEMBERS_BUCKET_FOLD", "RP_MEMBERS_FUSE", "RP_MEMBERS_SIDE_BUILD",
         "RP_MEMBERS_CK_BYTES", "RP_MEMBERS_GROUP_SLOTS", "RP_BK_REC8", "RP_BK_DIRECT", "RP_BK_SGRID")
LARGE = ("default", "bucket0", "direct0", "rec8-0", "sgrid48")
SIDE = ("k_hash_long", "k_ck_commit", "k_ck_hist")
N, K = 3000, 2000


def environments():
    """The empty environment, every value tests/ and tools/ab_fold.py / tools/c3_ab.py give these
    knobs, RP_MEMBERS_FUSE=1 and =2, and the sorted fold for single batches of a live handle."""
    g = lambda slots, gib: {"RP_MEMBERS_GROUP_SLOTS": str(slots), "RP_MEMBERS_CK_BYTES": str(gib << 30)}
    return [
        ("default", {}),
        ("bucket1", {"RP_MEMBERS_BUCKET_FOLD": "1"}),
        ("bucket0", {"RP_MEMBERS_BUCKET_FOLD": "0"}),
        ("sorted", {"RP_MEMBERS_SORTED_FOLD": "1"}),
        ("side0", {"RP_MEMBERS_SIDE_BUILD": "0"}),
        ("side1", {"RP_MEMBERS_SIDE_BUILD": "1"}),
        ("side2", {"RP_MEMBERS_SIDE_BUILD": "2"}),
        ("ck600k", {"RP_MEMBERS_CK_BYTES": "600000"}),  # tests/test_members_gpu.py: four slots here
        ("ck510k", {"RP_MEMBERS_CK_BYTES": "510000"}),  # three slots, before and after the 500 new names
        ("g256", g(256, 4)),
        ("g192", g(192, 3)),
        ("g512", g(512, 6)),
        ("side-g256", dict(g(256, 4), RP_MEMBERS_SIDE_BUILD="1")),
        ("side-g512", dict(g(512, 6), RP_MEMBERS_SIDE_BUILD="1")),
        ("noside-g256", dict(g(256, 4), RP_MEMBERS_SIDE_BUILD="0")),
        ("fused-g512", dict(g(512, 6), RP_MEMBERS_SIDE_BUILD="2")),
        ("direct0", {"RP_BK_DIRECT": "0"}),
        ("rec8-0", {"RP_BK_REC8": "0"}),
        ("sgrid48", {"RP_BK_SGRID": "48"}),
        ("bucket1-direct0", {"RP_MEMBERS_BUCKET_FOLD": "1", "RP_BK_DIRECT": "0"}),
        ("bucket1-rec8-0", {"RP_MEMBERS_BUCKET_FOLD": "1", "RP_BK_REC8": "0"}),
        ("fuse1", {"RP_MEMBERS_FUSE": "1"}),
        ("fuse2", {"RP_MEMBERS_FUSE": "2"}),
        ("sorted-mid", {}),
    ]


def run():
    import numpy as np
    import torch

    sys.path.insert(0, REPO)
    import bench

    rpa = bench.load_pkg()
    S = bench._synth()
    names = [S.c2_addr(i) for i in range(N + 500)]
    st0, inc0 = np.zeros(N, np.uint8), np.full(N, 100, np.int64)
    big = 1 << 19
    big_names, big_st, big_inc = S.c3_members(big)
    big_upd = S.c3_updates(big, big, seed=77, base_inc=big_inc + 3)
    mark = torch.empty(64, dtype=torch.uint8, device="cuda")
    app = torch.empty(big, dtype=torch.uint8, device="cuda")
    na = torch.zeros(1, dtype=torch.int32, device="cuda")
    main = torch.cuda.current_stream().cuda_stream
    second = torch.cuda.Stream()
    damp = {"dampScoringInitial": 0, "dampScoringPenalty": 500, "dampScoringSuppressLimit": 2500}
    keep = []

    def dev(ids, us, ui):
        d = [torch.from_numpy(np.asarray(ids, np.uint32).view(np.int32)).cuda(),
             torch.from_numpy(np.asarray(us, np.uint8)).cuda(), torch.from_numpy(np.asarray(ui, np.int64)).cuda()]
        keep.append(d)
        return [t.data_ptr() for t in d]

    for name, env in environments():
        for v in KNOBS:
            os.environ.pop(v, None)
        os.environ.update(env)
        rng = np.random.default_rng(4)
        step = [0]

        def batch(m, nn, k=K, hot=0, stream=main, rng_lo=None, sorted_now=False):
            step[0] += 1
            ids = rng.integers(0, nn, size=k).astype(np.uint32)
            if hot:
                ids[rng.choice(k, size=hot, replace=False)] = 7
            us = rng.integers(0, 4, size=k).astype(np.uint8)
            ui = (100 + step[0] + rng.integers(0, 3, size=k)).astype(np.int64)
            d = dev(ids, us, ui)
            if sorted_now and name == "sorted-mid":
                os.environ["RP_MEMBERS_SORTED_FOLD"] = "1"
            if rng_lo is None:
                m.update_dev(d[0], d[1], d[2], k, 1434500000000 + step[0], app.data_ptr(), None, None, na.data_ptr(),
                             stream)
            else:
                m.update_range_dev(d[0], d[1], d[2], k, 1434500000000 + step[0], rng_lo[0], rng_lo[1], app.data_ptr(),
                                   None, None, na.data_ptr(), stream)
            if name == "sorted-mid":
                os.environ.pop("RP_MEMBERS_SORTED_FOLD", None)

        def handle(n=N):
            m = rpa.Membership(whoami=names[0], capacity=n)
            m.intern(names[:n])
            m.update_ids(np.arange(n, dtype=np.uint32), st0[:n], inc0[:n], now_ms=1)
            return m

        m = handle()
        for _ in range(3):
            batch(m, N)
        batch(m, N, hot=17)
        batch(m, N, sorted_now=True)
        batch(m, N, hot=17, sorted_now=True)
        batch(m, N)
        batch(m, N, k=0)
        batch(m, N)
        m.intern(names[N:N + 500])
        batch(m, N + 500)
        batch(m, N + 500)
        _ = m.checksum
        batch(m, N + 500)
        torch.cuda.synchronize()
        with torch.cuda.stream(second):
            batch(m, N + 500, stream=second.cuda_stream)
        second.synchronize()
        for q in range(12):
            batch(m, N + 500, sorted_now=q == 5)
        _ = m.checksum
        m.close()
        # Membership.set: a handle that is not ready stashes its updates, set() merges them
        m = rpa.Membership(whoami=names[0], capacity=N)
        ids0 = np.asarray(m.intern(names[:N]), np.uint32)
        m.set_ready(False)
        for r in range(2):
            m.update_ids(ids0[r::2], st0[r::2], inc0[r::2] + r)
        m.set()
        m.set_ready(True)
        batch(m, N)
        _ = m.checksum
        m.close()
        # the checksum deferred
        m = handle()
        rpa.check(rpa.lib().rp_members_defer_checksum(m._h, 1))
        for _ in range(3):
            batch(m, N)
        m.compute_checksum()
        m.close()
        # damp scoring
        m = handle()
        m.damp_configure(damp)
        for q in range(3):
            batch(m, N, sorted_now=q == 1)
        _ = m.checksum
        m.close()
        # a ranged batch (not under the sorted fold, which refuses it), after a plain one
        if name != "sorted":
            m = handle()
            batch(m, N)
            batch(m, N, rng_lo=(0, 4096))
            batch(m, N, rng_lo=(4096, 8192))
            batch(m, N)
            _ = m.checksum
            m.close()
        if name in LARGE:
            m = rpa.Membership(whoami=big_names[0], capacity=big)
            ids0 = np.asarray(m.intern(big_names), np.uint32)
            m.update_ids(ids0, big_st, big_inc, now_ms=1)
            d = dev(*big_upd)
            m.update_dev(d[0], d[1], d[2], big, 1434500000999, app.data_ptr(), None, None, na.data_ptr(), main)
            _ = m.checksum
            m.close()
        torch.cuda.synchronize()
        rpa.gen_uuid_keys_dev(42, 0, 1, mark.data_ptr())  # end mark
        torch.cuda.synchronize()
        del keep[:]
        print(name, "ok", flush=True)
    print("%d environments done" % len(environments()))


def listing(trace_dir):
    files = glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True)
    assert len(files) == 1, files
    rows = list(csv.DictReader(open(files[0])))
    rows.sort(key=lambda r: int(r["Dispatch_Id"]))

    def dims(r, what):
        if what in r:
            return r[what]
        return "x".join(r[what + "_" + a] for a in "XYZ")

    envs = environments()
    number, per_env = {}, [([], [])]
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
            per_env.append(([], []))
            continue
        env = envs[len(per_env) - 1][1] if len(per_env) <= len(envs) else {}
        side = name.startswith(SIDE) or (name.startswith("k_mck_write") and env.get("RP_MEMBERS_SIDE_BUILD") == "1")
        launch = " ".join((name, dims(r, "Grid_Size"), dims(r, "Workgroup_Size"),
                           r.get("LDS_Block_Size", r.get("Group_Segment_Size"))))
        per_env[-1][1 if side else 0].append(launch)
    assert len(per_env) == len(envs) + 1 and not per_env[-1][0] and not per_env[-1][1], (len(per_env), len(envs))
    # numbered in the order of a callers' stream's first use, the side streams' after (their place varies)
    for which in (0, 1):
        for pair in per_env:
            for launch in (pair[which] if which == 0 else sorted(pair[which])):
                number.setdefault(launch, len(number) + 1)
    per_env = [([number[x] for x in a], [number[x] for x in b]) for a, b in per_env]
    print("%d launches, %d distinct, %d environments" % (sum(len(a) + len(b) for a, b in per_env), len(number), len(envs)))
    for launch, k in number.items():
        print(k, launch)
    fill = lambda seq: textwrap.fill(" ".join(map(str, seq)), 100, initial_indent="  ", subsequent_indent="  ")
    for (name, env), (seq, side) in zip(envs, per_env):
        print()
        print(name, " ".join("%s=%s" % kv for kv in sorted(env.items())))
        print(fill(seq))
        print(name, "side streams (sorted)")
        print(fill(sorted(side)))


if __name__ == "__main__":
    if sys.argv[1:2] == ["run"]:
        run()
    elif sys.argv[1:2] == ["list"] and len(sys.argv) == 3:
        listing(sys.argv[2])
    else:
        sys.exit(__doc__)
