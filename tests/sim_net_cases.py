"""Network partitions for the gossip simulator: the structured families, the family that differs
only in the split's length, the seeded random event lists and two controls without any side event,
shared by the golden generator (tests/golden/make_sim_net_golden.py -> tests/golden/
sim_net_golden.json, the reference modules under tests/golden/ref_sim_net.js) and the tests that
replay them (tests/test_sim_net_golden.py, tests/test_sim_net_gpu.py).

Events are [round, kind, node] or [round, "side", node, side], applied in list order before that
round's phase A. A partition is a batch of "side" events in one round; [round, "heal", 0] puts
every node back on side 0."""
import random

import sim_tiny_cases

KINDS = sim_tiny_cases.KINDS
RANDOM_NS = (3, 4, 5, 6, 7, 8, 9, 12, 15, 17)
CONTROLS = ("n5-killrevive", "rand04-n6")
LENGTH_NS = {6: 2, 9: 3}  # n -> suspRounds of the length family
LENGTH_SPLIT = 4  # the round the length family splits in


def split(r, sides):
    """The batch that puts node v on side s at round r, for {v: s}."""
    return [[r, "side", v, s] for v, s in sorted(sides.items())]


def halves(n):
    return {v: 1 for v in range(n // 2, n)}


def structured_cases():
    """[(name, n, dead, rounds, susp, events)]"""
    out = []
    # two and three sides, never healed and healed late
    out.append(("n6-two", 6, [0] * 6, 40, 3, split(5, halves(6))))
    out.append(("n9-three", 9, [0] * 9, 45, 3, split(5, {3: 1, 4: 1, 5: 1, 6: 2, 7: 2, 8: 2})))
    out.append(("n9-three-healed", 9, [0] * 9, 60, 2,
                split(5, {3: 1, 4: 1, 5: 1, 6: 2, 7: 2, 8: 2}) + [[30, "heal", 0]]))
    out.append(("n17-three", 17, [0] * 17, 45, 3, split(6, {v: 1 + v % 2 for v in range(5, 17)})))
    # a side of one node (n = 2: every side is one node)
    out.append(("n2-alone", 2, [0, 0], 30, 2, split(3, {1: 1})))
    out.append(("n5-alone", 5, [0] * 5, 40, 3, split(4, {4: 7})))
    out.append(("n5-alone-healed", 5, [0] * 5, 50, 3, split(4, {4: 255}) + [[9, "heal", 0]]))
    # a side whose every node is down, then one of them comes back to an empty side
    out.append(("n6-side-all-down", 6, [0, 0, 0, 0, 1, 1], 40, 3, split(3, {4: 2, 5: 2})))
    out.append(("n6-side-all-down-revive", 6, [0, 0, 0, 0, 1, 1], 50, 3,
                [[2, "kill", 3]] + split(3, {3: 2, 4: 2, 5: 2}) + [[20, "revive", 4], [35, "heal", 0]]))
    # a node changing sides twice in one round
    out.append(("n6-twice", 6, [0] * 6, 40, 2, [[4, "side", 2, 1], [4, "side", 2, 2], [4, "side", 4, 1],
                                                 [4, "side", 5, 1]]))
    # a split in round 0
    out.append(("n7-round0", 7, [0] * 7, 40, 3, split(0, {0: 3, 1: 3, 2: 3})))
    # a heal in the same round as a split: after it (nothing is cut), then before it (the cut stays)
    out.append(("n6-heal-same-round", 6, [0] * 6, 50, 2,
                split(6, halves(6)) + [[6, "heal", 0], [12, "heal", 0]] + split(12, {0: 1, 1: 1})))
    # a join and a leave on each side during the split
    ev = split(3, {4: 1, 5: 1, 6: 1, 7: 1}) + [[8, "join", 3], [8, "join", 7], [10, "leave", 1], [10, "leave", 5]]
    out.append(("n8-join-leave", 8, [0, 0, 0, 1, 0, 0, 0, 1], 45, 3, ev))
    out.append(("n8-join-leave-healed", 8, [0, 0, 0, 1, 0, 0, 0, 1], 60, 3, ev + [[25, "heal", 0]]))
    return out


def length_cases():
    """The same cluster split in two halves at LENGTH_SPLIT and healed 1, 2, .. suspRounds + 10
    rounds later: [(name, n, dead, rounds, susp, events)]."""
    out = []
    for n, susp in LENGTH_NS.items():
        for length in range(1, susp + 11):
            ev = split(LENGTH_SPLIT, halves(n)) + [[LENGTH_SPLIT + length, "heal", 0]]
            out.append(("n%d-len%02d" % (n, length), n, [0] * n, LENGTH_SPLIT + length + 30, susp, ev))
    return out


def random_net_events(rng, dead, ev_rounds):
    """sim_tiny_cases.random_events plus partitions: 0 to 3 events a round, a uniform kind on a
    uniform node, and, by the case's plan, split batches and heals before or after them. "open":
    one split, never healed; "healed": one split and one heal; "many": a split at one round, and a split or a
    heal in about every sixth other round. Tracks who is up and on which side and skips a join that nobody on the
    joiner's side could answer (the model refuses it); nothing else is skipped."""
    n = len(dead)
    up = [not d for d in dead]
    side = [0] * n
    events = []
    plan = rng.choice(("open", "healed", "many"))
    r0 = rng.randrange(0, ev_rounds // 2)
    r1 = rng.randrange(r0 + 1, ev_rounds)

    def cut(r):
        k = rng.randint(1, 3)
        new = [rng.randint(0, k) for _ in range(n)]
        if len(set(new)) == 1:
            new[rng.randrange(n)] = new[0] + 1
        for v in range(n):
            if new[v] != side[v]:
                events.append([r, "side", v, new[v]])
                side[v] = new[v]

    def heal(r):
        events.append([r, "heal", 0])
        side[:] = [0] * n

    def net(r):
        if plan == "many":
            if r == r0 or rng.random() < 1 / 6:  # (a heal needs a cut to end)
                (cut if not any(side) or rng.random() < 0.6 else heal)(r)
        elif r == r0:
            cut(r)
        elif r == r1 and plan == "healed":
            heal(r)

    for r in range(ev_rounds):
        first = rng.random() < 0.5
        if first:
            net(r)
        for _ in range(rng.randint(0, 3)):
            kind = rng.choice(KINDS)
            v = rng.randrange(n)
            if kind == "join":
                if not any(up[u] and side[u] == side[v] for u in range(n) if u != v):
                    continue
                up[v] = True
            elif kind != "leave":
                up[v] = kind == "revive"
            events.append([r, kind, v])
        if not first:
            net(r)
    return events


def random_cases(count=20):
    """Case i from random.Random(3000 + i): n, who is down at the start, the events of rounds
    0..24, then the suspicion period; 40 rounds."""
    out = []
    for i in range(count):
        rng = random.Random(3000 + i)
        n = rng.choice(RANDOM_NS)
        dead = [1 if rng.random() < 0.15 else 0 for _ in range(n)]
        events = random_net_events(rng, dead, 25)
        susp = rng.choice((2, 3))
        out.append(("net-rand%02d-n%d" % (i, n), n, dead, 40, susp, events))
    return out


def control_cases():
    """Two cases of sim_tiny_cases, unchanged: [(seed, case)] with the seeds make_golden.py gives
    them, so that their checksums equal those committed in sim_tiny_golden.json."""
    fams = [(101 + i, c) for i, c in enumerate(sim_tiny_cases.structured_cases())]
    fams += [(1000 + i, c) for i, c in enumerate(sim_tiny_cases.random_cases())]
    out = [(seed, c) for seed, c in fams if c[0] in CONTROLS]
    assert len(out) == len(CONTROLS)
    return out


def all_cases():
    """[(seed, family, case)] in fixture order."""
    out = []
    for fam, cases in (("structured", structured_cases()), ("length", length_cases()), ("random", random_cases())):
        out += [(3001 + len(out) + i, fam, c) for i, c in enumerate(cases)]
    return out + [(seed, "control", c) for seed, c in control_cases()]


def sides_after(n, events, rounds):
    """[rounds][n]: every node's side after each round's events."""
    side = [0] * n
    out = []
    for r in range(rounds):
        for e in events:
            if e[0] == r and e[1] == "side":
                side[e[2]] = e[3]
            elif e[0] == r and e[1] == "heal":
                side = [0] * n
        out.append(list(side))
    return out


def open_split(n, events):
    """For a case whose one split is never healed (every side event in one round, no heal): (round,
    {node: side} after it), else None. The batch has to be contiguous in the list, as a partition
    is: the per-side comparison with a kill scenario holds for such batches only."""
    rounds = {e[0] for e in events if e[1] == "side"}
    if len(rounds) != 1 or any(e[1] == "heal" for e in events):
        return None
    r = rounds.pop()
    idx = [i for i, e in enumerate(events) if e[1] == "side"]
    assert idx == list(range(idx[0], idx[-1] + 1)), "a split is one contiguous batch"
    side = [0] * n
    for e in events:
        if e[1] == "side":
            side[e[2]] = e[3]
    return r, side


def kill_equivalent(n, events, s):
    """What side s lives through in a case open_split accepts, as a scenario without sides: at the
    split every node outside s is killed instead, and later events on those nodes are dropped."""
    r, side = open_split(n, events)
    first = next(i for i, e in enumerate(events) if e[1] == "side")
    out = [list(e) for e in events[:first] if e[0] <= r]
    assert out == [list(e) for e in events[:first]], "events are listed by round"
    out += [[r, "kill", v] for v in range(n) if side[v] != s]
    out += [list(e) for e in events[first:] if e[1] != "side" and side[e[2]] == s]
    return out


def load():
    """The fixture's cases by name, through golden_util.load_sim, with `sides` expanded to one row
    per round as checksums and maxPiggyback are. Parsed once per process; callers do not modify it."""
    import golden_util as gu
    cases = gu.load_sim("sim_net_golden.json")["cases"]
    for c in cases:
        if "sideRuns" in c:
            c["sides"] = [row for count, row in c.pop("sideRuns") for _ in range(count)]
        assert len(c["sides"]) == c["rounds"]
    return {c["name"]: c for c in cases}
