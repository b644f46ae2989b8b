"""Which lookup kernel every environment runs: the calls, and the list of kernels they launched.

    rocprofv3 --kernel-trace --output-format csv -d DIR -o run -- python tools/lookup_kernels.py run
    python tools/lookup_kernels.py list DIR > kernels.txt

`run` builds a 100-server x 100-point ring (compact layout, hinted index and LDS index all
available) and, under every entry of tests/test_ring_gpu.py's LAYOUTS, every variant of
tools/ab_lookup.py and RP_LOOKUP_SORT = 0 | 256 | 512 | 1024, calls lookup and lookupN(n), n in 1, 2,
3, 4, 5, 9, on 700, 1,500 and 18,732 36-byte keys on the device (700: below the compact path's 1,024;
1,500: below the 2,048-key tile, so 4 keys a lane; 18,732 = 2 x 8,192 + 2,048 + 300: sorted tiles at
every thread count, a lean tile and a partial tail), then lookupN(3) once on caller hashes and once
on 20-byte keys. It checks no result (the ablation variants are wrong by design), only that every
call returns, and closes every environment with a one-key k_gen_uuid launch that marks its end in
the trace. `list` takes name, grid, workgroup and LDS size of every k_lookupn* launch of the trace, in
launch order, and prints each distinct launch once, numbered by first use, then every environment's
launches as those numbers; environments with the same launches share an entry. Equal files from two
builds mean equal kernel choices, launch for launch.
"""
import ast
import csv
import glob
import os
import re
import sys
import textwrap

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KNOBS = ("RP_RING_WIDE", "RP_RING_NOWINDOW", "RP_RING_LAYOUT", "RP_LOOKUP_ABLATE", "RP_LOOKUP_WPRED", "RP_LOOKUP_HINT",
         "RP_LOOKUP_LDS", "RP_LOOKUP_LDS_GRID", "RP_LOOKUP_LDS_STG", "RP_LOOKUP_LDS_ABL", "RP_LOOKUP_WS",
         "RP_LOOKUP_WS_GRID", "RP_LOOKUP_WS_ABL", "RP_LOOKUP_KPL", "RP_LOOKUP_SORT", "RP_LOOKUP_GRID", "RP_LOOKUP_LEAN",
         "RP_LOOKUP_HALF", "RP_LOOKUP_FUSEFIX", "RP_LOOKUP_STG", "RP_LOOKUP_LH", "RP_LOOKUP_STGHS", "RP_LOOKUP_DEBUG",
         "RP_LOOKUP_TICKET", "RP_LOOKUP_STAGGER", "RP_LOOKUP_TICKET_GRID")


def literal(path, name):
    """The dict literal assigned to `name` somewhere in the Python file at `path`."""
    for node in ast.walk(ast.parse(open(os.path.join(REPO, path)).read())):
        if isinstance(node, ast.Assign) and getattr(node.targets[0], "id", None) == name:
            return ast.literal_eval(node.value)
    raise KeyError(name)


def environments():
    envs = [("layout:" + k, v) for k, v in literal("tests/test_ring_gpu.py", "LAYOUTS").items()]
    envs += [("ab:" + k, v[0]) for k, v in literal("tools/ab_lookup.py", "variants").items()]
    envs += [("sort:" + s, {"RP_LOOKUP_SORT": s}) for s in ("0", "256", "512", "1024")]
    envs += [("ticket:" + s, {"RP_LOOKUP_TICKET": s}) for s in ("0", "1")]
    return envs


def run():
    import numpy as np
    import torch

    sys.path.insert(0, REPO)
    import bench

    rpa = bench.load_pkg()
    ring = rpa.HashRing()
    ring.addRemoveServers([bench.c2_addr(i) for i in range(100)])
    st = torch.cuda.current_stream()
    sizes = (700, 1500, 18732)
    keys = torch.empty(max(sizes) * 36, dtype=torch.uint8, device="cuda")
    rpa.gen_uuid_keys_dev(42, 0, max(sizes), keys.data_ptr(), st.cuda_stream)
    out = torch.empty(max(sizes) * 9, dtype=torch.int32, device="cuda")
    rng = np.random.default_rng(7)
    hashes = rng.integers(0, 1 << 32, 1500, dtype=np.uint64).astype(np.uint32)
    keys20 = rng.integers(0, 256, (1500, 20), dtype=np.uint8)
    for name, env in environments():
        for kn in KNOBS:
            os.environ.pop(kn, None)
        os.environ.update(env)
        for B in sizes:
            ring.lookup_dev(keys.data_ptr(), B, out.data_ptr(), 36, None, st.cuda_stream)
            for n in (1, 2, 3, 4, 5, 9):
                ring.lookupn_dev(keys.data_ptr(), B, n, out.data_ptr(), None, 36, None, st.cuda_stream)
        ring.lookupn_hashes(hashes, 3)
        ring.lookupn_ids(keys20, 3)
        rpa.gen_uuid_keys_dev(42, 0, 1, keys.data_ptr(), st.cuda_stream)  # end mark; key 0 gets its own bytes again
        torch.cuda.synchronize()
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

    number, per_env = {}, [[]]  # per_env[0]: before the first environment
    for r in rows:
        name = re.sub(r"^void ", "", r["Kernel_Name"])
        name = re.sub(r"^(\w+::|\(anonymous namespace\)::)*", "", name)
        if name.endswith(")"):  # drop the parameter list: back to the bracket that closes last
            depth, i = 0, len(name)
            while i > 0 and (depth or i == len(name)):
                i -= 1
                depth += {")": 1, "(": -1}.get(name[i], 0)
            name = name[:i]
        if name.startswith("k_gen_uuid"):
            per_env.append([])
        elif name.startswith("k_lookupn"):
            launch = " ".join((name, dims(r, "Grid_Size"), dims(r, "Workgroup_Size"),
                               r.get("LDS_Block_Size", r.get("Group_Segment_Size"))))
            per_env[-1].append(number.setdefault(launch, len(number) + 1))
    assert number, "no k_lookupn* launch among %d rows (first name: %s)" % (len(rows), rows[0]["Kernel_Name"] if rows else None)
    names = [name for name, _ in environments()]
    # marks: one from the key fill before the first environment, one at the end of each
    assert len(per_env) == len(names) + 2 and not per_env[0] and not per_env[-1], (len(per_env), len(names))
    shared = {}
    for name, seq in zip(names, per_env[1:]):
        shared.setdefault(tuple(seq), []).append(name)
    print("%d launches, %d distinct, %d environments" % (sum(map(len, per_env)), len(number), len(names)))
    for launch, k in number.items():
        print(k, launch)
    print()
    for seq, envs in shared.items():
        print(textwrap.fill(" ".join(envs), 100))
        print(textwrap.fill(" ".join(map(str, seq)), 100, initial_indent="  ", subsequent_indent="  "))


if __name__ == "__main__":
    if sys.argv[1:2] == ["run"]:
        run()
    elif sys.argv[1:2] == ["list"] and len(sys.argv) == 3:
        listing(sys.argv[2])
    else:
        sys.exit(__doc__)
