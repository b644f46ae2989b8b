"""The reference's damp bookkeeping, change by change (a plain module shared by the CPU and GPU
damp tests; not a conftest).

Restates what Membership.update / set / _decayMembersDampScore do to every Member's dampScore,
lastUpdateDampScore and lastUpdateTimestamp (lib/membership/index.js:208-324,374-383;
member.js:28-66,98-153), sequentially, with the oracle's arithmetic (orc.damp_penalized,
orc.damp_decayed, orc.damp_cfg). Which changes were applied is an input: the per-change applied
flags of the batch (orc.Members.update_ids, or the reference's own applied list). Existence is
tracked here, per address.

    a created member starts at (initial, initial, null);
    an applied update of a member other than the local one is penalized when `enabled`;
    every applied update of an existing member stamps the timestamp, local and disabled included;
    an unapplied change reports the member's current score and no flag.

Pinned against the reference's own run in tests/test_oracle_damp.py (CPU); never against the
code under test. A null lastUpdateTimestamp is 0, as in the device table and orc_damp.c.
"""
import numpy as np

_runs = {}


def reference_run(orc, case):
    """A case of tests/damp_cases.py through the oracle's Membership (applied flags, checksum) and
    the model below, once per process (the result is shared: do not write to it). Per op a dict:
    update ops have "applied" (0 / 1 / 2 = created, as the device reports it), "napplied",
    "new_status" / "new_inc" (the updates as applied), "score" and "flag" per change and
    "checksum"; every op has "columns", the (dampScore,
    lastUpdateDampScore, lastUpdateTimestamp) arrays over case["names"], and "exists"."""
    if case["name"] in _runs:
        return _runs[case["name"]]
    names = case["names"]
    om = orc.Members(names, local=case["local"])
    model = DampModel(orc, case["config"], local=names.index(case["local"]))
    out = []
    for op in case["ops"]:
        o = {}
        if op["type"] == "decay":
            model.decay(op["now"])
        else:
            ids = op["ids"]
            app, nst, ninc, n = om.update_ids(ids, op["status"], op["inc"], now_ms=op["now"])
            o.update(new_status=nst, new_inc=ninc)
            before = set(model.state)
            score, flag = model.update([int(i) for i in ids], app, op["now"])
            code = app.copy()
            seen = set()
            for j, (i, a) in enumerate(zip(ids, app)):
                i = int(i)
                if a and i not in before and i not in seen:
                    code[j] = 2
                    seen.add(i)
            o.update(applied=code, napplied=int(n), score=score, flag=flag, checksum=om.checksum)
        o["columns"] = model.columns(range(len(names)))
        o["exists"] = np.array([model.exists(i) for i in range(len(names))])
        out.append(o)
    _runs[case["name"]] = out
    return out


class DampModel:
    def __init__(self, orc, config=None, local=None):
        self.orc = orc
        self.local = local
        self.cfg = orc.damp_cfg(config)
        self.state = {}  # address (any hashable key) -> [dampScore, lastUpdateDampScore, lastUpdateTimestamp]

    def reconfigure(self, config=None):
        """A new config from now on; every member's state is kept."""
        self.cfg = self.orc.damp_cfg(config)

    def update(self, addresses, applied, now):
        """One Membership.update batch at Date.now() = now. applied: a flag per change (any
        non-zero value = applied). Returns (score after each change float64[k], suppress flag
        uint8[k])."""
        k = len(addresses)
        score = np.empty(k, np.float64)
        flag = np.zeros(k, np.uint8)
        cfg, state = self.cfg, self.state
        for i, (a, ap) in enumerate(zip(addresses, applied)):
            st = state.get(a)
            if not ap:
                score[i] = st[0] if st is not None else cfg.initial
                continue
            if st is None:  # _createMember: a fresh Member, no penalty, null timestamp
                state[a] = [cfg.initial, cfg.initial, 0]
                score[i] = cfg.initial
                continue
            if cfg.enabled and a != self.local:
                s, exc = self.orc.damp_penalized(cfg, st[1], st[2], now)
                st[0] = st[1] = s
                flag[i] = 1 if exc else 0
            st[2] = now
            score[i] = st[0]
        return score, flag

    def set(self, picked):
        """Membership.set: every picked address becomes a fresh Member (it restarts)."""
        for a in picked:
            self.state[a] = [self.cfg.initial, self.cfg.initial, 0]

    def decay(self, now):
        """The decayer tick: dampScore only; the last score and timestamp stay."""
        for st in self.state.values():
            st[0] = self.orc.damp_decayed(self.cfg, st[1], st[2], now)

    def exists(self, a):
        return a in self.state

    def snapshot(self):
        return {a: tuple(v) for a, v in self.state.items()}

    def columns(self, addresses):
        """The three columns over `addresses` (float64, float64, int64); an address that was never
        created reads as a fresh member would: (initial, initial, 0)."""
        n = len(addresses)
        sc = np.full(n, self.cfg.initial, np.float64)
        ls = np.full(n, self.cfg.initial, np.float64)
        ts = np.zeros(n, np.int64)
        for i, a in enumerate(addresses):
            st = self.state.get(a)
            if st is not None:
                sc[i], ls[i], ts[i] = st
        return sc, ls, ts
