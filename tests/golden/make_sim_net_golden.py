"""Regenerate tests/golden/sim_net_golden.json: the partition cases of tests/sim_net_cases.py run
through the REFERENCE modules by tests/golden/ref_sim_net.js (needs the reference checkout and
node, as make_golden.py does; never runs on the GPU box).

    python tests/golden/make_sim_net_golden.py [rings]

`rings` instead writes tests/golden/sim_ring_golden.json (make_golden.py simring: every node's ring
after every round, for these cases through ref_sim_net.js and for the tiny and flap cases).

Outputs are data only: the cases and what the reference returned. Rerunning reproduces the
committed file byte for byte."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(HERE)))
import make_golden as mg  # noqa: E402
import sim_net_cases as net  # noqa: E402

BRANCHES = mg.BRANCHES + ("unreachable",)


def cases():
    """Final views of every node when n <= 8 (the length family: of nodes 0 and n-1), else of 0,
    n-1 and the joiners."""
    S = mg.synth()
    out = []
    for seed, family, (name, n, dead, rounds, susp, events) in net.all_cases():
        assert 2 <= n <= 17 and rounds <= 70 and susp in (2, 3) or family == "control", name
        joiners = sorted({e[2] for e in events if e[1] == "join"} - {0, n - 1})
        views = list(range(n)) if n <= 8 and family != "length" else [0, n - 1] + joiners
        out.append({"name": name, "family": family, "names": [S.c2_addr(i) for i in range(n)],
                    "inc0": [int(x) for x in S.c3_members(n)[2]], "dead": dead, "seed": seed,
                    "suspRounds": susp, "now0": S.NOW0, "rounds": rounds, "views": views, "events": events})
    return out


def main():
    cs = cases()
    outs = mg.run_node("ref_sim_net.js", cs)
    fixture = {"generator": "tests/golden/make_sim_net_golden.py + tests/sim_net_cases.py + "
                            "tests/golden/ref_sim_net.js",
               "reference": "as sim_golden.json",
               "note": "the schema of sim_tiny_golden.json, plus per case sideRuns = [[count, row], ...], every "
                       "node's side after each round; events are [round, kind, node] or [round, 'side', node, side]; "
                       "family is structured | length | random | control (control: a case of sim_tiny_golden.json, "
                       "no side event); branches.unreachable = how often a sender looked at a node on another "
                       "side (a ping target, a ping-req helper, a join responder)",
               "cases": []}
    total = dict.fromkeys(BRANCHES, 0)
    for c, o in zip(cs, outs):
        f = {k: c[k] for k in ("name", "family", "seed", "suspRounds", "now0", "rounds", "views")}
        f["n"] = len(c["names"])
        f["dead"] = c["dead"]
        f["events"] = c["events"]
        f["branches"] = {k: o["branches"][k] for k in BRANCHES}
        for k in BRANCHES:
            total[k] += o["branches"][k]
        assert o["sides"] == net.sides_after(f["n"], c["events"], c["rounds"]), c["name"]
        f["checksumRuns"] = mg.runs(o["rounds"])
        f["maxPiggybackRuns"] = mg.runs(o["maxPiggyback"])
        f["sideRuns"] = mg.runs(o["sides"])
        f["fullSyncs"] = o["fullSyncs"]
        f["finalViews"] = o["finalViews"]
        fixture["cases"].append(f)
    print("branches taken:", total)
    path = os.path.join(HERE, "sim_net_golden.json")
    with open(path, "w") as fh:
        json.dump(fixture, fh, separators=(",", ":"))
    print("wrote", path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 300_000


if __name__ == "__main__":
    if sys.argv[1:] == ["rings"]:
        mg.make_sim_ring()
    else:
        main()
