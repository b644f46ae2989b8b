"""The hot-address damp inputs (tests/damp_cases.py) reach what they claim. CPU only, on the
oracle's Membership and the sequential model (tests/damp_model.py): conditions on the inputs,
not on the device code. The GPU tests (tests/test_damp_paths_gpu.py) run the same cases."""
import numpy as np
import pytest

import damp_cases
import golden_util as gu
from damp_model import reference_run

CHUNK = damp_cases.CHUNK


@pytest.mark.parametrize("case", damp_cases.cases(), ids=lambda c: c["name"])
def test_hot_inputs_reach_every_fold_path(orc, case):
    ref = reference_run(orc, case)
    cfg = orc.damp_cfg(case["config"])
    roles = case["roles"]
    assert 6 <= sum(op["type"] == "update" for op in case["ops"]) <= 8
    assert len({op["now"] for op in case["ops"]}) == len(case["ops"])
    saw_max = saw_min = False
    for op, o in zip(case["ops"], ref):
        sc = o["columns"][0][o["exists"]]
        saw_max |= bool((sc == cfg.max).any()) or ("score" in o and bool((o["score"] == cfg.max).any()))
        saw_min |= bool((sc == cfg.min).any()) or ("score" in o and bool((o["score"] == cfg.min).any()))
    assert saw_max and saw_min
    for b, t in enumerate(case["hot_ops"]):
        op, o = case["ops"][t], ref[t]
        ids, app, flag = op["ids"], o["applied"], o["flag"]
        cnt = np.bincount(ids, minlength=len(case["names"]))
        assert cnt.max() >= 1024
        for c in (15, 16, 17):
            assert (cnt == c).sum() >= 1, c
        assert cnt[roles["c60"]] == 60
        # the long address: at least 3 chunks of 1,024 positions, at least 500 applied
        lp = np.flatnonzero(ids == roles["long"])
        assert len(np.unique(lp // CHUNK)) >= 3
        assert (app[lp] != 0).sum() >= 500
        # a suppress flag in an overflow address's second or later chunk (of its own changes)
        late = False
        for a in np.flatnonzero(cnt > 16):
            p = np.flatnonzero(ids == a)
            chunks = np.unique(p // CHUNK)
            late |= len(chunks) > 1 and bool(flag[p[p // CHUNK > chunks[0]]].any())
        assert late
        # the local member is hot: applied, never flagged, its score never moves
        lo = np.flatnonzero(ids == roles["local"])
        assert len(lo) > 16 and (app[lo] != 0).sum() >= 10 and not flag[lo].any()
        assert len(np.unique(o["score"][lo].view(np.uint64))) == 1
        assert o["columns"][2][roles["local"]] == op["now"]
        # the newcomer is created by its first change and applied at least twice after it
        nw = np.flatnonzero(ids == roles["newcomers"][b])
        assert len(nw) > 16 and not ref[t - 1]["exists"][roles["newcomers"][b]]
        assert app[nw[0]] == 2 and (app[nw[1:]] == 1).sum() >= 2
        assert (o["score"][nw[1:]] > cfg.initial).any()
        # the batch after it touches every hot address once
        nxt = np.bincount(case["ops"][t + 1]["ids"], minlength=len(case["names"]))
        hot = [roles["local"], roles["long"], roles["c60"], roles["newcomers"][b]] + roles["c15"] + roles["c16"] + \
            roles["c17"]
        assert all(cnt[a] >= 15 and nxt[a] == 1 for a in hot)
        assert nxt.max() <= 16
    # scores cross the suppress limit on hot addresses and decay between batches
    assert sum(int(o["flag"].sum()) for o in ref if "flag" in o) > 100
    decays = [t for t, op in enumerate(case["ops"]) if op["type"] == "decay"]
    assert any((ref[t]["columns"][0] != ref[t - 1]["columns"][0]).any() for t in decays)


def test_hot_golden_has_the_hot_shape():
    """tests/golden/damp_hot_golden.json (the reference's own run): one batch with an address past
    1,024 changes and addresses with 16 and 17, under 6,000 changes in all, about 40 members."""
    g = gu.load("damp_hot_golden.json")
    (case,) = g["cases"]
    assert case["name"] == "hot"
    ups = [(op, o) for op, o in zip(case["ops"], case["out"]) if op["type"] == "update"]
    assert sum(len(op["changes"]) for op, _ in ups) < 6000
    assert 30 <= len(case["out"][-1]["members"]) <= 50
    best = max(ups, key=lambda x: len(x[0]["changes"]))
    addrs = [c[0] for c in best[0]["changes"]]
    cnt = {}
    for a in addrs:
        cnt[a] = cnt.get(a, 0) + 1
    assert max(cnt.values()) > 1024 and 16 in cnt.values() and 17 in cnt.values()
    long_addr = max(cnt, key=cnt.get)
    assert sum(addrs[i] == long_addr for i in best[1]["applied"]) >= 500
    assert len(best[1]["suppressed"]) > 100
    # the inputs are the ones damp_cases generates (the golden is their reference run)
    want = damp_cases.golden_hot_inputs()
    assert case["config"] == want["config"] and case["local"] == want["local"]
    for op, w in zip(case["ops"], want["ops"]):
        assert op["now"] == w["now"] and op["type"] == w["type"]
        if op["type"] == "update":
            assert [want["names"].index(c[0]) for c in op["changes"]] == w["ids"].tolist()
            assert [c[2] for c in op["changes"]] == w["inc"].tolist()
