"""The timeline model (tests/timeline_model.py) against the CPU oracle's simulator on the random
tiny cases: its derived `converged` is the oracle's converged() after every round, the pairs add
up, and a killed member is seen suspect no later than faulty. (The oracle keeps no ring rows and
no sides: in_ring and the partition cases are checked on the GPU.)"""
import numpy as np
import pytest

import sim_tiny_cases
import timeline_model as tm
from test_oracle_sim import synth

CASES = sim_tiny_cases.random_cases()


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_model_matches_oracle_convergence(orc, case):
    name, n, dead, rounds, susp, events = case
    S = synth()
    names = [S.c2_addr(i) for i in range(n)]
    sim = orc.Sim(names, S.c3_members(n)[2], np.array(dead, dtype=np.uint8), seed=1000, susp_rounds=susp,
                  now0=1434401518824 + 10 ** 9, events=events)
    model = tm.Timeline(n, dead, events)
    for r in range(rounds):
        sim.step()
        rows = np.stack([sim.view(v)[0] for v in range(n)])
        rec = model.record(sim.checksums(), sim.stats(), status_rows=rows)
        assert rec["round"] == r
        assert int(rec["pairs"].sum()) == rec["observers"] * n, (name, r)
        conv = rec["observers"] == 0 or (rec["ck_min"] == rec["ck_max"] and rec["unmet"] == 0)
        assert conv == sim.converged(), (name, r)
    tl = model.result()
    assert tl["round"].tolist() == list(range(rounds)) and tl["converged"].dtype == bool
    assert (np.diff(tl["stats"].astype(np.int64), axis=0) >= 0).all()
    only_killed = [a for a in range(n) if {e[1] for e in events if e[2] == a} <= {"kill"}]
    fs = tl["first_seen"]
    for a in only_killed:
        assert fs[a, tm.FAULTY - 1] >= fs[a, tm.SUSPECT - 1], (name, a)
        assert fs[a, tm.LEAVE - 1] == tm.NEVER, (name, a)


def test_model_sees_every_kind_of_record(orc):
    """Across the cases the model produces converged and unconverged records, unmet > 0,
    false_faulty > 0 and a round nobody observes, so the checks above are not vacuous."""
    seen = set()
    S = synth()
    for name, n, dead, rounds, susp, events in CASES:
        sim = orc.Sim([S.c2_addr(i) for i in range(n)], S.c3_members(n)[2], np.array(dead, dtype=np.uint8),
                      seed=1000, susp_rounds=susp, now0=1434401518824 + 10 ** 9, events=events)
        model = tm.Timeline(n, dead, events)
        for _ in range(rounds):
            sim.step()
            model.record(sim.checksums(), sim.stats(), status_rows=np.stack([sim.view(v)[0] for v in range(n)]))
        tl = model.result()
        seen |= {"converged"} if tl["converged"].any() else set()
        seen |= {"unconverged"} if (~tl["converged"]).any() else set()
        seen |= {"unmet"} if tl["unmet"].any() else set()
        seen |= {"false_faulty"} if tl["false_faulty"].any() else set()
        seen |= {"nobody"} if (tl["observers"] == 0).any() else set()
        seen |= {"first_seen"} if (tl["first_seen"] != tm.NEVER).any() else set()
    assert seen == {"converged", "unconverged", "unmet", "false_faulty", "nobody", "first_seen"}, seen


def test_model_ring_window_and_counts_form():
    """result(last) keeps the newest records and first_seen; counts = (status, in_ring) gives the
    record the rows give."""
    n = 4
    rows = np.array([[0, 1, 2, 0], [0, 0, 2, 3], [0, 0, 0, 0], [1, 1, 1, 1]], dtype=np.uint8)
    ring = rows != 2
    a, b = tm.Timeline(n, [0, 0, 0, 1], []), tm.Timeline(n, [0, 0, 0, 1], [])
    stats = dict.fromkeys(tm.STAT_NAMES, 3)
    for _ in range(3):
        ra = a.record([5, 5, 7, 9], stats, status_rows=rows, ring_rows=ring)
        obs = np.array([True, True, True, False])
        rb = b.record([5, 5, 7, 9], stats, counts=tm.counts_of(rows, ring, obs))
        assert all(np.array_equal(ra[k], rb[k]) for k in ra)
    assert ra["observers"] == 3 and (ra["ck_min"], ra["ck_max"]) == (5, 7)
    assert ra["pairs"].tolist() == [8, 1, 2, 1] and ra["in_ring"] == 10
    assert ra["unmet"] == 3  # member 3 is down and wanted faulty: no observer holds it there
    assert ra["false_faulty"] == 2  # member 2 is up and faulty in two views
    tl = a.result(last=2)
    assert tl["round"].tolist() == [1, 2] and tl["first_seen"].tolist() == [[tm.NEVER] * 3, [0, tm.NEVER, tm.NEVER],
                                                                            [tm.NEVER, 0, tm.NEVER], [tm.NEVER, tm.NEVER, 0]]
    assert tm.same(tl, b.result(last=2)) is None and tm.same(tl, a.result()) == "round"
