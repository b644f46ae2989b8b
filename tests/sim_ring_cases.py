"""Ring membership cases for the gossip simulator: the `flap` family, shared by the golden generator
(tests/golden/make_golden.py simring -> tests/golden/sim_ring_golden.json, the reference modules)
and the tests that replay it (tests/test_oracle_sim_ring.py, tests/test_sim_ring_gpu.py).

A node's hash ring keeps a member that turns suspect as it was (createUpdatedHandlerForRing,
lib/on_membership_event.js:106-134), so a suspect row outside the ring needs a history: the member
was faulty (out of the ring) and is then suspected at a newer incarnation. The recipe: some nodes
are killed at round 1 and declared faulty, revived at round 14 (they refute with a new incarnation)
and killed again a few rounds later, while some views still hold them faulty at the old
incarnation. Those views take `suspect` at the new incarnation and keep the member out of the ring.

Events are [round, kind, node], applied in list order before that round's phase A."""

SEED = 7
SUSP = 3
KILL, REVIVE, KILL2 = 1, 14, 17


def flap_events(flapping, kill2=KILL2, revive=REVIVE):
    flapping = list(flapping)
    return ([[KILL, "kill", v] for v in flapping] + [[revive, "revive", v] for v in flapping] +
            [[kill2, "kill", v] for v in flapping])


def every_eighth(n):
    return range(1, n, 8)


# n -> (flapping nodes, round of the second kill, round of the revival): chosen on the oracle so that
# the run holds a suspect row outside the ring (every eighth node gives none below 64 nodes); the
# fixture's own rows say whether the reference agrees (tests/test_oracle_sim_ring.py)
FLAP = {9: ([4], 16, 14), 17: ([1, 9], 16, 14), 33: ([1, 31], 17, 14), 65: (list(every_eighth(65)), 17, 14)}
FLAP_ROUNDS = 40


def flap_cases():
    """[(name, n, dead, rounds, susp, events)] as sim_tiny_cases gives them; the seed is SEED."""
    return [("flap-n%d" % n, n, [0] * n, FLAP_ROUNDS, SUSP, flap_events(nodes, kill2, revive))
            for n, (nodes, kill2, revive) in FLAP.items()]
