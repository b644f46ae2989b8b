"""Tiny and degenerate clusters for the gossip simulator: the structured families and the seeded
random event generator, shared by the golden generator (tests/golden/make_golden.py simtiny ->
tests/golden/sim_tiny_golden.json, the reference modules) and the GPU tests that draw larger
cases from the same generator (tests/test_sim_tiny_gpu.py, against the oracle).

Events are [round, kind, node], applied in list order before that round's phase A."""
import random

KINDS = ("kill", "revive", "leave", "join")
RANDOM_NS = (2, 2, 3, 3, 4, 5, 6, 7, 8, 9, 12, 15, 17)


def _all_but(n, up):
    return [0 if v in up else 1 for v in range(n)]


def structured_cases():
    """[(name, n, dead, rounds, susp, events)]: the families that reach the small-cluster
    branches (no ping target, 0 / 1 / 2 ping-req helpers, 1 / 2 join responders, everyone left,
    everyone but one down, several events of one node in one round)."""
    out = []
    for n in (2, 3, 4, 5, 6, 8, 15):
        out.append(("n%d-plain" % n, n, [0] * n, 30, 3, []))
    for n in range(2, 7):  # 0, 1, 2 and 3 helpers as n grows
        out.append(("n%d-lastdead" % n, n, _all_but(n, range(n - 1)), 40, 3, []))
    for n in range(2, 7):  # the iterator runs dry once the others are faulty
        out.append(("n%d-onlyone" % n, n, _all_but(n, [0]), 40, 3, [[20, "revive", n - 1]]))
    for n in (2, 3, 4, 5, 8):
        out.append(("n%d-one-responder" % n, n, _all_but(n, [0]), 50, 3,
                    [[5, "join", n - 1], [30, "kill", 0], [31, "join", 0]]))
    for n in (3, 4, 5, 8):
        out.append(("n%d-two-responders" % n, n, _all_but(n, [0, 1]), 50, 3,
                    [[5, "join", n - 1], [6, "leave", 0], [20, "join", 0]]))
    for n in (2, 3, 4, 5, 8):
        out.append(("n%d-all-leave" % n, n, [0] * n, 40, 2,
                    [[2, "leave", v] for v in range(n)] + [[20, "join", 0]]))
    for n in (2, 3, 4, 5, 8):
        out.append(("n%d-all-killed-midrun" % n, n, [0] * n, 40, 2,
                    [[4, "kill", v] for v in range(1, n)] + [[25, "revive", v] for v in range(1, n)]))
    for n in (2, 3, 4, 5, 8):
        out.append(("n%d-same-round" % n, n, [0] * n, 40, 2,
                    [[3, "kill", 1], [3, "revive", 1], [3, "leave", 1], [3, "join", 1], [3, "kill", 0],
                     [9, "join", 0], [9, "leave", 0]]))
    for n in range(2, 7):
        out.append(("n%d-killrevive" % n, n, [0] * n, 60, 2,
                    [[1, "kill", 0], [1, "leave", 1], [10, "revive", 0], [12, "join", 1], [30, "kill", n - 1],
                     [30, "revive", n - 1], [40, "leave", 0], [41, "join", 0]]))
    return out


def random_events(rng, dead, ev_rounds):
    """0 to 3 events in each of rounds 0..ev_rounds-1, a uniform kind on a uniform node. Tracks
    which nodes are up and skips a join that no other live node could answer (the model refuses
    it); nothing else is skipped."""
    n = len(dead)
    up = [not d for d in dead]
    events = []
    for r in range(ev_rounds):
        for _ in range(rng.randint(0, 3)):
            kind = rng.choice(KINDS)
            v = rng.randrange(n)
            if kind == "join":
                if not any(up[u] for u in range(n) if u != v):
                    continue
                up[v] = True
            elif kind != "leave":
                up[v] = kind == "revive"
            events.append([r, kind, v])
    return events


def random_dead_events(rng, n, p_dead, ev_rounds):
    """(dead, events): each node down at the start with probability p_dead, then random_events."""
    dead = [1 if rng.random() < p_dead else 0 for _ in range(n)]
    return dead, random_events(rng, dead, ev_rounds)


def random_cases(count=40):
    """Case i from random.Random(1000 + i): n, who is down at the start, the events of rounds
    0..34, then the suspicion period; 45 rounds."""
    out = []
    for i in range(count):
        rng = random.Random(1000 + i)
        n = rng.choice(RANDOM_NS)
        dead, events = random_dead_events(rng, n, 0.25, 35)
        susp = rng.choice((2, 3, 6))
        out.append(("rand%02d-n%d" % (i, n), n, dead, 45, susp, events))
    return out
