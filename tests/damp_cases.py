"""Deterministic hot-address inputs for the damp-scoring tests (seeded numpy, data only).

A case is a run of Membership.update batches and decayer ticks over a small member list in which
a few addresses are hot: in a hot batch they get 15, 16 (the last count the grouped fold takes on
its fast path), 17 (the first that overflows), 60 and about 1,100 changes, the long one spread
over the whole batch so that it lies in several 1,024-change chunks of the overflow fold. The
local member is hot too (no self-penalty, the timestamp is still stamped), and each hot batch
has one hot address that does not exist before it (created by its first change, penalized by
later ones of the same fold). After a hot batch comes one that touches every hot address once.
Incarnations and statuses rise often enough that most hot changes apply.

    case = {"name", "local", "names", "config", "ops", "roles", "hot_ops"}
    op   = {"type": "update", "now", "ids" u32[k], "status" u8[k], "inc" i64[k]}
         | {"type": "decay", "now"}

status is 0..3 = alive, suspect, faulty, leave. ids index `names`; a test that interns `names` in order gets the same ids from the device table.
tests/test_damp_inputs.py asserts on the CPU that the inputs reach what is claimed here.
"""
import numpy as np

T0 = 1434401518824
CHUNK = 1024  # positions per chunk of the overflow fold (k_fold_ovf)


def addr(i):
    return "10.%d.%d.%d:3000" % (i >> 16, (i >> 8) & 255, i & 255)


class _Gen:
    def __init__(self, seed, n):
        self.rng = np.random.default_rng(seed)
        self.n = n
        self.inc = T0 - 10 ** 6 + self.rng.integers(0, 10 ** 5, n).astype(np.int64)

    def change(self, a, local):
        """The next change about address id a: mostly a higher incarnation (applies unless the
        member has left and the status is suspect / faulty), sometimes an escalation at the same
        incarnation, sometimes a stale one. About the local member: mostly suspect / faulty,
        which it refutes (applied, whatever the incarnation)."""
        rng = self.rng
        r = rng.random()
        if a == local:
            if r < 0.7:
                return int(rng.integers(1, 3)), int(self.inc[a])
            return 0, int(self.inc[a]) - 1
        if r < 0.72:
            self.inc[a] += 1
            return int(rng.choice(4, p=[0.45, 0.25, 0.25, 0.05])), int(self.inc[a])
        if r < 0.86:
            return int(rng.integers(1, 3)), int(self.inc[a])
        return int(rng.integers(0, 4)), int(self.inc[a]) - 1

    def batch(self, ids, local, now):
        st = np.empty(len(ids), np.uint8)
        inc = np.empty(len(ids), np.int64)
        for j, a in enumerate(ids):
            st[j], inc[j] = self.change(int(a), local)
        return {"type": "update", "now": int(now), "ids": np.asarray(ids, np.uint32), "status": st, "inc": inc}

    def shuffled(self, counts, cold, fill):
        """ids with the given multiplicities plus `fill` random cold ones, in random order."""
        ids = [np.full(c, a, np.uint32) for a, c in counts.items()]
        if fill > 0:
            ids.append(self.rng.choice(cold, fill).astype(np.uint32))
        ids = np.concatenate(ids)
        return ids[self.rng.permutation(len(ids))]

    def once(self, hot, cold, k):
        """Every hot address once; cold ones round-robin (each about equally often) up to k."""
        fill = max(0, k - len(hot))
        reps = np.resize(self.rng.permutation(cold), fill).astype(np.uint32)
        ids = np.concatenate([np.asarray(hot, np.uint32), reps])
        return ids[self.rng.permutation(len(ids))]


def make_case(name, seed, n, config, hot_sizes, warm_k, once_k, long_counts):
    """n members; names[0] is the local one. hot_sizes: changes per hot batch (one newcomer each);
    long_counts: the long address's changes in each hot batch."""
    g = _Gen(seed, n)
    names = [addr(i + 1) for i in range(n)]
    local = 0
    nhot = len(hot_sizes)
    newcomers = list(range(n - nhot, n))
    roles = {"local": local, "long": 1, "c60": 2, "c15": [3, 4], "c16": [5, 6], "c17": [7, 8], "newcomers": newcomers}
    hot = [local, 1, 2, 3, 4, 5, 6, 7, 8]
    cold = np.arange(9, n - nhot, dtype=np.uint32)
    now = T0
    ops, hot_ops = [], []
    # every member but the newcomers is created, once each
    ops.append(g.batch(np.arange(0, n - nhot, dtype=np.uint32), local, now))
    if warm_k:  # a few changes per address, the hot ones three times: no overflow yet
        now += 4000 + int(g.rng.integers(1, 900))
        ops.append(g.batch(g.shuffled({a: 3 for a in hot}, cold, warm_k - 3 * len(hot)), local, now))
    gaps = [1500, 45_000, 2000]
    for b, (k, nlong) in enumerate(zip(hot_sizes, long_counts)):
        now += 4000 + int(g.rng.integers(1, 900))
        counts = {roles["long"]: nlong, roles["c60"]: 60, local: 30, newcomers[b]: 20}
        for key, c in (("c15", 15), ("c16", 16), ("c17", 17)):
            for a in roles[key]:
                counts[a] = c
        for a in newcomers[:b]:  # an earlier batch's newcomer stays warm
            counts[a] = 5
        hot_ops.append(len(ops))
        ops.append(g.batch(g.shuffled(counts, cold, k - sum(counts.values())), local, now))
        # the same addresses once: the grouped fold's per-address state must be clean again
        now += 1500 + int(g.rng.integers(1, 400))
        ops.append(g.batch(g.once(hot + newcomers[:b + 1], cold, once_k), local, now))
        now += gaps[b % len(gaps)]
        ops.append({"type": "decay", "now": int(now)})
    return {"name": name, "local": names[local], "names": names, "config": config, "ops": ops, "roles": roles,
            "hot_ops": hot_ops}


# scores clamp at max (4 applied penalties at one timestamp), cross the suppress limit (2), sit at
# min after the long gap (15 half-lives) and decay between batches
INT_CONFIG = {"dampScoringPenalty": 251, "dampScoringMax": 1000, "dampScoringSuppressLimit": 500,
              "dampScoringHalfLife": 3, "dampScoringMin": 25, "dampScoringInitial": 40}
FRAC_CONFIG = {"dampScoringPenalty": 333.25, "dampScoringMax": 1000.5, "dampScoringSuppressLimit": 500.5,
               "dampScoringHalfLife": 2.75, "dampScoringMin": 2.25, "dampScoringInitial": 17.5}

_cache = {}


def cases():
    """The generated cases (built once per process; treat them as read-only)."""
    if not _cache:
        _cache["cases"] = [
            make_case("hot-int", 7101, 300, INT_CONFIG, [2600, 2900, 2200], 2000, 2000, [1100, 1130, 1030]),
            make_case("hot-frac", 7102, 300, FRAC_CONFIG, [2400, 2700], 2000, 2000, [1100, 1090]),
        ]
    return _cache["cases"]


def golden_hot_inputs():
    """The inputs of the `hot` case of tests/golden/damp_hot_golden.json (make_damp_golden.py runs
    the reference over them): 40 members, under 6,000 changes in all."""
    return make_case("hot", 7103, 40, INT_CONFIG, [2300, 600], 0, 40, [1100, 200])
