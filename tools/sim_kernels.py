"""Which checksum kernels the gossip simulator runs under every environment, launch by launch.

    rocprofv3 --kernel-trace --output-format csv -d DIR -o run -- python tools/sim_kernels.py run
    python tools/sim_kernels.py list DIR > kernels.txt

`run` steps, under the empty environment and every entry of tests/test_sim_tiny_gpu.py's KNOBS, a
900-node simulator with 60 nodes down for 12 rounds, as one handle and in 3 shards; and, under the
empty environment and RP_SIM_TWINS=0 only, a 20,000-node simulator with 200 down for 12 rounds
(313 groups of 64 views: more than the CUs, so the refresh takes the lane path by size, k_ck_lanes
while nearly every view is dirty and k_ck_pc<3, 2> after). It checks no result, only that every
call returns, and closes every (environment, shape) with a one-key k_gen_uuid launch that marks its
end in the trace. `list` takes name, grid, workgroup and LDS size of every k_ck_*, k_pass1,
k_twin_*, k_dirty_list, k_d1_list and k_early_list launch, and of every launch between
k_ck_sort_keys and the chains that follow it (the radix sort), and prints each distinct launch once,
numbered by first use, then every (environment, shape)'s launches as those numbers in launch
order. RP_SIM_EARLY=1 runs two streams side by side, so the order of its launches in the trace
is not fixed: that environment's are printed as a sorted list. Equal files from two builds mean
equal kernel choices, launch for launch.
"""
import ast
import csv
import glob
import os
import re
import sys
import textwrap

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LISTED = ("k_ck_", "k_pass1", "k_twin_", "k_dirty_list", "k_d1_list", "k_early_list")
LARGE = ("default", "twins0")


def environments():
    for node in ast.walk(ast.parse(open(os.path.join(REPO, "tests", "test_sim_tiny_gpu.py")).read())):
        if isinstance(node, ast.Assign) and getattr(node.targets[0], "id", None) == "KNOBS":
            knobs = ast.literal_eval(node.value)
    envs = [("default", {}), ("twins0", {"RP_SIM_TWINS": "0"})]
    envs += [(k, {a: b if b is not None else str(16 * 900) for a, b in v.items()}) for k, v in knobs.items()]
    return envs


def runs():
    """(environment name, its variables, shape name, nodes, down, shards)"""
    for name, env in environments():
        yield name, env, "n900", 900, 60, None
        yield name, env, "n900-g3", 900, 60, 3
        if name in LARGE:
            yield name, env, "n20000", 20000, 200, None


def run():
    import torch

    sys.path.insert(0, REPO)
    import bench

    rpa = bench.load_pkg()
    sys.path.insert(0, os.path.join(REPO, "ringpop-node_amd"))
    import synth as S

    names_of = {}
    mark = torch.empty(64, dtype=torch.uint8, device="cuda")
    touched = set()
    for name, env, shape, n, down, G in runs():
        for k in touched:
            os.environ.pop(k, None)
        os.environ.update(env)
        touched |= set(env)
        if n not in names_of:
            names_of[n] = ([S.c2_addr(i) for i in range(n)], S.c3_members(n)[2], S.kill_set(n, down, 5))
        args = names_of[n]
        kw = dict(seed=5, suspicion_rounds=6)
        sim = rpa.ShardedGossipSim(*args, G, **kw) if G else rpa.GossipSim(*args, **kw)
        sim.step(12)
        sim.close()
        rpa.gen_uuid_keys_dev(42, 0, 1, mark.data_ptr())  # end mark
        torch.cuda.synchronize()
        print(name, shape, "ok", flush=True)
    print("%d runs done" % len(list(runs())))


def listing(trace_dir):
    files = glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True)
    assert len(files) == 1, files
    rows = list(csv.DictReader(open(files[0])))
    rows.sort(key=lambda r: int(r["Dispatch_Id"]))

    def dims(r, what):
        if what in r:
            return r[what]
        return "x".join(r[what + "_" + a] for a in "XYZ")

    number, per_run, in_sort = {}, [[]], False
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
            per_run.append([])
            in_sort = False
            continue
        listed = name.startswith(LISTED)
        if listed or in_sort:
            launch = " ".join((name, dims(r, "Grid_Size"), dims(r, "Workgroup_Size"),
                               r.get("LDS_Block_Size", r.get("Group_Segment_Size"))))
            per_run[-1].append(number.setdefault(launch, len(number) + 1))
        if listed:
            in_sort = name.startswith("k_ck_sort_keys")
    assert number, "no listed launch among %d rows" % len(rows)
    todo = list(runs())
    assert len(per_run) == len(todo) + 1 and not per_run[-1], (len(per_run), len(todo))
    print("%d launches, %d distinct, %d runs" % (sum(map(len, per_run)), len(number), len(todo)))
    for launch, k in number.items():
        print(k, launch)
    for (name, env, shape, _, _, _), seq in zip(todo, per_run):
        print()
        if "RP_SIM_EARLY" in env:
            print(name, shape, "(sorted)")
            seq = sorted(seq)
        else:
            print(name, shape)
        print(textwrap.fill(" ".join(map(str, seq)), 100, initial_indent="  ", subsequent_indent="  "))


if __name__ == "__main__":
    if sys.argv[1:2] == ["run"]:
        run()
    elif sys.argv[1:2] == ["list"] and len(sys.argv) == 3:
        listing(sys.argv[2])
    else:
        sys.exit(__doc__)
