"""The simulator's timeline (rp_sim_timeline_*) restated in numpy: one record of
cluster-wide aggregates per round from every observer's status row (or the per-member counts of
those rows), the observers' checksums, the cumulative stats and the up / left sets the event list
gives, plus first_seen carried across rounds. Shared by the CPU test (rows from the oracle) and the
GPU tests (rows from view(v) / ring_members(v) or census() of a twin handle stepped round by round).

Events are [round, kind, node] or [round, kind, node, arg], kind a name ("kill", "revive", "leave",
"join", "side", "heal")."""
import numpy as np

NEVER = 0xFFFFFFFF
ALIVE, SUSPECT, FAULTY, LEAVE = range(4)
STAT_NAMES = ("pings", "pingreqs", "fullsyncs", "applied")
SUMS = ("observers", "pairs", "in_ring", "unmet", "false_faulty", "stats")
FIELDS = ("round", "ck_min", "ck_max") + SUMS
_DTYPE = {"round": np.uint64, "observers": np.uint32, "ck_min": np.uint32, "ck_max": np.uint32, "pairs": np.uint64,
          "in_ring": np.uint64, "unmet": np.uint64, "false_faulty": np.uint64, "stats": np.uint64}


def counts_of(status_rows, ring_rows, obs):
    """(status [n, 4], in_ring [n] or None): per member, the observers' rows by status and in the ring."""
    st = np.asarray(status_rows)[obs]
    cnt = np.stack([(st == s).sum(axis=0) for s in range(4)], axis=1).astype(np.int64)
    ring = None if ring_rows is None else np.asarray(ring_rows, dtype=bool)[obs].sum(axis=0).astype(np.int64)
    return cnt, ring


class Timeline:
    def __init__(self, n, dead, events, start=0):
        """start: the first recorded round (events before it are applied at once)."""
        self.n = n
        self.events = [list(e) for e in events]
        self.up = np.array([not d for d in dead])
        self.left = np.zeros(n, dtype=bool)
        self.first_seen = np.full((n, 3), NEVER, dtype=np.uint32)
        self.records = []
        self.round = 0
        for _ in range(start):
            self._events()
            self.round += 1

    def _events(self):
        """The rule of _observers in tests/test_sim_net_gpu.py: a leave counts when the node is up,
        a join starts a fresh process."""
        for e in self.events:
            if e[0] != self.round:
                continue
            kind, v = e[1], e[2]
            if kind in ("kill", "revive"):
                self.up[v] = kind == "revive"
            elif kind == "leave" and self.up[v]:
                self.left[v] = True
            elif kind == "join":
                self.up[v], self.left[v] = True, False

    def observers(self):
        """The observers of the round about to be recorded (its events applied): bool[n]."""
        up, left = self.up.copy(), self.left.copy()
        self._events()
        obs = self.up & ~self.left
        self.up, self.left = up, left
        return obs

    def record(self, cks, stats, status_rows=None, ring_rows=None, counts=None):
        """Append the record of the round that just ran. status_rows [n, n] (row v: node v's view)
        with optional ring_rows, or counts = (status [n, 4], in_ring [n]) over the observers.
        stats: the cumulative {pings, pingreqs, fullsyncs, applied}."""
        self._events()
        obs = self.up & ~self.left
        if counts is None:
            cnt, ring = counts_of(status_rows, ring_rows, obs)
        else:
            cnt, ring = np.asarray(counts[0], dtype=np.int64), np.asarray(counts[1], dtype=np.int64)
        n_obs = int(obs.sum())
        assert (cnt.sum(axis=1) == n_obs).all()
        c = np.asarray(cks, dtype=np.uint32)[obs]
        want = np.where(self.left, LEAVE, np.where(~self.up, FAULTY, 0))
        wanted = np.flatnonzero(want)
        rec = {"round": self.round, "observers": n_obs,
               "ck_min": int(c.min()) if n_obs else 0xFFFFFFFF, "ck_max": int(c.max()) if n_obs else 0,
               "pairs": cnt.sum(axis=0), "in_ring": 0 if ring is None else int(ring.sum()),
               "unmet": int((n_obs - cnt[wanted, want[wanted]]).sum()),
               "false_faulty": int(cnt[obs][:, [FAULTY, LEAVE]].sum()),
               "stats": np.array([stats[k] for k in STAT_NAMES], dtype=np.uint64)}
        seen = (cnt[:, 1:] > 0) & (self.first_seen == NEVER)
        self.first_seen[seen] = self.round
        self.records.append(rec)
        self.round += 1
        return rec

    def result(self, last=None):
        """What GossipSim.timeline() returns for these records (the newest `last` of them)."""
        recs = self.records if last is None else self.records[len(self.records) - min(last, len(self.records)):]
        res = {k: np.array([r[k] for r in recs], dtype=_DTYPE[k]).reshape((len(recs), 4) if k in ("pairs", "stats")
                                                                           else (len(recs),)) for k in FIELDS}
        res["converged"] = (res["observers"] == 0) | ((res["ck_min"] == res["ck_max"]) & (res["unmet"] == 0))
        res["first_seen"] = self.first_seen.copy()
        return res


def same(got, want, skip=()):
    """None when the two timelines are equal in value, shape and dtype, else the first field that is not."""
    for k in list(FIELDS) + ["converged", "first_seen"]:
        if k in skip:
            continue
        g, w = got[k], want[k]
        if g.dtype != w.dtype or g.shape != w.shape or not np.array_equal(g, w):
            return k
    return None
