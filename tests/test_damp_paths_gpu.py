"""Damp scoring on every path a batch can take through Membership.update, against the sequential
model (tests/damp_model.py: the reference's bookkeeping with the oracle's arithmetic, pinned to
the reference's own run in tests/test_oracle_damp.py) and the oracle's Membership.

Paths: the grouped fold (k_fold_fast for an address with at most 16 changes in the batch, the
overflow fold for more: in the string build's length launch, or k_fold_ovf when the checksum is
deferred), the sorted fold (RP_MEMBERS_SORTED_FOLD=1) and RP_MEMBERS_BUCKET_FOLD=1, which with damp
on must stay on the grouped path. Inputs: the hot-address cases of tests/damp_cases.py (what they
reach is asserted on the CPU in tests/test_damp_inputs.py) and the reference's run of the hot
shape, tests/golden/damp_hot_golden.json.

Tolerance: none. Scores are compared as uint64 views of the doubles, after every batch: the
applied flags and count and the checksum with the oracle; damp_last (all k entries) and damp_dump
(all three columns, every member) with the model.
"""
import numpy as np
import pytest

import damp_cases
import golden_util as gu
from damp_model import DampModel, reference_run
from test_damp_gpu import run_case

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

PATHS = ["grouped", "sorted", "bucket-forced", "grouped-deferred"]
T0 = damp_cases.T0
RP_EINVAL = -1


def u64(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


@pytest.fixture(params=PATHS)
def make(request, gpu, monkeypatch):
    """A handle factory for the fold path of this parameter (every knob is read when the handle is
    created and again at the top of every update, set and checksum call, MemberKnobs of
    csrc/rp_members_plan.h; it is set first and stays for the test)."""
    for v in ("RP_MEMBERS_SORTED_FOLD", "RP_MEMBERS_BUCKET_FOLD", "RP_MEMBERS_FUSE"):
        monkeypatch.delenv(v, raising=False)
    if request.param == "sorted":
        monkeypatch.setenv("RP_MEMBERS_SORTED_FOLD", "1")
    elif request.param == "bucket-forced":
        monkeypatch.setenv("RP_MEMBERS_BUCKET_FOLD", "1")

    def factory(whoami, **kw):
        m = gpu.Membership(whoami=whoami, **kw)
        m.deferred = request.param == "grouped-deferred"
        if m.deferred:  # no string build per batch: the overflow fold is k_fold_ovf's
            gpu.check(gpu.lib().rp_members_defer_checksum(m._h, 1))
        return m
    return factory


@pytest.fixture
def make_default(gpu, monkeypatch):
    for v in ("RP_MEMBERS_SORTED_FOLD", "RP_MEMBERS_BUCKET_FOLD", "RP_MEMBERS_FUSE"):
        monkeypatch.delenv(v, raising=False)

    def factory(whoami, **kw):
        m = gpu.Membership(whoami=whoami, **kw)
        m.deferred = False
        return m
    return factory


def checksum_of(m):
    return m.compute_checksum() if getattr(m, "deferred", False) else m.checksum


def check_state(m, want_cols, want_exists, what):
    """damp_dump's three columns and the existence of every id against the model's."""
    sc, ls, ts = m.damp_dump()
    ex, _, _ = m.dump()
    n = len(want_exists)
    assert len(sc) == n, what
    assert np.array_equal(ex != 0, want_exists), what
    wsc, wls, wts = want_cols
    for name, g, w in (("dampScore", u64(sc), u64(wsc)), ("lastUpdateDampScore", u64(ls), u64(wls)),
                       ("lastUpdateTimestamp", ts, wts)):
        bad = np.flatnonzero(g != w)
        assert len(bad) == 0, (what, name, len(bad), [(int(i), float(sc[i]), float(wsc[i]), float(ls[i]),
                                                         float(wls[i]), int(ts[i]), int(wts[i])) for i in bad[:5]])


def check_batch(m, k, got, want, what):
    """got: (applied, n applied) of the batch just folded; want: its entry of reference_run."""
    app, na = got
    assert na == want["napplied"], what
    bad = np.flatnonzero(app != want["applied"])
    assert len(bad) == 0, (what, "applied", len(bad), bad[:5])
    sc, exc = m.damp_last(k)
    bad = np.flatnonzero(u64(sc) != u64(want["score"]))
    assert len(bad) == 0, (what, "damp_last score", len(bad),
                           [(int(i), float(sc[i]), float(want["score"][i])) for i in bad[:5]])
    assert np.array_equal(exc, want["flag"]), (what, "damp_last flag", np.flatnonzero(exc != want["flag"])[:5])
    check_state(m, want["columns"], want["exists"], what)
    assert checksum_of(m) == want["checksum"], what


def run_hot_case(m, case, ref, fold):
    """fold(op, want) -> (applied u8[k], n applied): one update batch through the handle."""
    m.damp_configure(case["config"])
    assert m.intern(case["names"]) == list(range(len(case["names"])))
    for t, (op, want) in enumerate(zip(case["ops"], ref)):
        what = (case["name"], t)
        if op["type"] == "decay":
            m.damp_decay(op["now"])
            check_state(m, want["columns"], want["exists"], what)
        else:
            check_batch(m, len(op["ids"]), fold(op, want), want, what)
    m.close()


@pytest.mark.parametrize("case", damp_cases.cases(), ids=lambda c: c["name"])
def test_hot_addresses_on_every_fold_path(make, orc, case):
    """15, 16, 17, 60 and about 1,100 changes of one address in a batch (the long one in several
    chunks of the overflow fold, its damp state carried between them through memory), the local
    member hot, a member created inside the hot batch; then every hot address once."""
    ref = reference_run(orc, case)
    m = make(case["local"])

    def fold(op, want):
        app, _, _, na = m.update_ids(op["ids"], op["status"], op["inc"], now_ms=op["now"])
        return app, na
    run_hot_case(m, case, ref, fold)


def test_hot_golden_on_every_fold_path(make, gpu, orc):
    """The reference's own run of the hot shape (damp_hot_golden.json), on every path."""
    (case,) = gu.load("damp_hot_golden.json")["cases"]
    run_case(gpu, orc, case, make=make)


@pytest.mark.parametrize("alias", [False, True], ids=["own-outputs", "outputs-alias-inputs"])
def test_device_form_with_damp_on(make_default, orc, alias):
    """rp_members_update_dev with damp on (device buffers, stream-ordered), synchronized before the
    host reads; once with the status / incarnation outputs being the input arrays. The results
    are the model's and the oracle's, as the host form's are (the test above)."""
    case = damp_cases.cases()[0]
    ref = reference_run(orc, case)
    m = make_default(case["local"])
    stream = torch.cuda.current_stream().cuda_stream

    def fold(op, want):
        k = len(op["ids"])
        d_ids = torch.from_numpy(op["ids"].view(np.int32).copy()).cuda()
        d_st = torch.from_numpy(op["status"].copy()).cuda()
        d_inc = torch.from_numpy(op["inc"].copy()).cuda()
        d_app = torch.empty(k, dtype=torch.uint8, device="cuda")
        d_nst = d_st if alias else torch.empty(k, dtype=torch.uint8, device="cuda")
        d_ninc = d_inc if alias else torch.empty(k, dtype=torch.int64, device="cuda")
        d_na = torch.zeros(1, dtype=torch.int32, device="cuda")
        m.update_dev(d_ids.data_ptr(), d_st.data_ptr(), d_inc.data_ptr(), k, op["now"], d_app.data_ptr(),
                     d_nst.data_ptr(), d_ninc.data_ptr(), d_na.data_ptr(), stream)
        torch.cuda.synchronize()
        assert np.array_equal(d_nst.cpu().numpy(), want["new_status"])
        assert np.array_equal(d_ninc.cpu().numpy(), want["new_inc"])
        return d_app.cpu().numpy(), int(d_na.item())
    run_hot_case(m, case, ref, fold)


class Live:
    """A device handle, the oracle's Membership and the model side by side over `names`."""

    def __init__(self, m, orc, names, config, n_interned=None):
        self.m, self.orc, self.names = m, orc, names
        self.om = orc.Members(names, local=names[0])
        self.model = DampModel(orc, config, local=0)
        m.damp_configure(config)
        self.n = 0
        self.intern(n_interned or len(names))

    def intern(self, n):
        assert self.m.intern(self.names[:n]) == list(range(n))
        self.n = n

    def configure(self, config):
        self.m.damp_configure(config)
        self.model.reconfigure(config)

    def want_state(self):
        return self.model.columns(range(self.n)), np.array([self.model.exists(i) for i in range(self.n)])

    def update(self, ids, st, inc, now, what):
        ids = np.asarray(ids, np.uint32)
        oa, _, _, ona = self.om.update_ids(ids, st, inc, now_ms=now)
        wsc, wfl = self.model.update([int(i) for i in ids], oa, now)
        ga, _, _, gna = self.m.update_ids(ids, st, inc, now_ms=now)
        assert gna == ona and np.array_equal(ga != 0, oa != 0), what
        sc, exc = self.m.damp_last(len(ids))
        assert np.array_equal(u64(sc), u64(wsc)) and np.array_equal(exc, wfl), what
        self.check(what)
        return oa, wsc, wfl

    def decay(self, now, what):
        self.m.damp_decay(now)
        self.model.decay(now)
        self.check(what)

    def check(self, what):
        cols, ex = self.want_state()
        check_state(self.m, cols, ex, what)
        assert checksum_of(self.m) == self.om.checksum, what


def rising(rng, ids, inc, p_up=0.8):
    """Changes about ids (in order) whose incarnations mostly rise: (status, inc) arrays."""
    st = np.empty(len(ids), np.uint8)
    out = np.empty(len(ids), np.int64)
    for j, a in enumerate(ids):
        if rng.random() < p_up:
            inc[a] += 1
        st[j] = rng.integers(0, 3)
        out[j] = inc[a]
    return st, out


def test_growth_keeps_damp_state_and_fills_new_ids(make_default, orc):
    """A table that grows twice with damp on and initial = 120 (capacity 1,024 -> 2,048 -> 4,096
    ids): earlier scores, last scores and timestamps survive, ids that were never updated read
    (120, 120, null), and members created after a growth start at 120."""
    cfg = {"dampScoringInitial": 120, "dampScoringPenalty": 251, "dampScoringMax": 1000, "dampScoringSuppressLimit": 500,
           "dampScoringHalfLife": 5, "dampScoringMin": 10}
    names = [damp_cases.addr(i + 1) for i in range(3000)]
    rng = np.random.default_rng(11)
    inc = np.full(len(names), 100, np.int64)
    L = Live(make_default(names[0], capacity=1024), orc, names, cfg, n_interned=900)
    now = T0
    lo = 0
    for stage, (n_int, n_upd) in enumerate([(900, 700), (1500, 1300), (3000, 2700)]):
        L.intern(n_int)  # past the capacity at stages 1 and 2; ids n_upd.. are never updated
        L.check(("interned", stage))
        now += 3000
        new = np.arange(lo, n_upd, dtype=np.uint32)  # created, once each: they start at 120
        oa, wsc, _ = L.update(new, np.zeros(len(new), np.uint8), inc[new], now, ("create", stage))
        assert oa.all() and (wsc == 120).all()
        for r in range(2):  # penalties over old and new members, some addresses several times
            now += 1200
            ids = rng.integers(0, n_upd, 1500).astype(np.uint32)
            st, ui = rising(rng, ids, inc)
            _, wsc, wfl = L.update(ids, st, ui, now, ("penalize", stage, r))
            assert (wsc > 120).any() and wfl.any()
        now += 700
        L.decay(now, ("decay", stage))
        sc, ls, ts = L.m.damp_dump()
        assert (sc[n_upd:] == 120).all() and (ls[n_upd:] == 120).all() and (ts[n_upd:] == 0).all()
        assert (lo == 0 or (ts[:lo] != 0).sum() > lo // 2) and len(np.unique(ls[:n_upd])) > 3
        lo = n_upd
    L.m.close()


def test_reconfigure_on_a_live_handle(make, orc):
    """rp_members_damp_configure again on a live handle: new penalty and half-life from then on,
    then enabled = 0 (no penalty, timestamps still stamped), then back. State is kept."""
    base = {"dampScoringInitial": 30, "dampScoringPenalty": 251, "dampScoringMax": 1000,
            "dampScoringSuppressLimit": 500, "dampScoringHalfLife": 4, "dampScoringMin": 5}
    names = [damp_cases.addr(i + 1) for i in range(60)]
    rng = np.random.default_rng(12)
    inc = np.full(len(names), 7, np.int64)
    L = Live(make(names[0]), orc, names, base)
    now = T0
    L.update(np.arange(60, dtype=np.uint32), np.zeros(60, np.uint8), inc.copy(), now, "create")
    steps = [base, dict(base, dampScoringPenalty=77.5, dampScoringHalfLife=1.5),
             dict(base, dampScoringPenalty=77.5, dampScoringHalfLife=1.5, dampScoringEnabled=False),
             dict(base, dampScoringPenalty=400, dampScoringHalfLife=9)]
    for s, cfg in enumerate(steps):
        L.configure(cfg)
        L.check(("configured", s))  # the new config alone changes no state
        before = L.model.snapshot()
        for r in range(2):
            now += 900
            ids = rng.integers(0, 60, 400).astype(np.uint32)  # about 7 changes per address
            ids[::9] = 5  # one address past 16: the overflow fold under the new config
            st, ui = rising(rng, ids, inc)
            oa, _, wfl = L.update(ids, st, ui, now, ("batch", s, r))
            assert oa.sum() > 200
        after = L.model.snapshot()
        if cfg.get("dampScoringEnabled", True):
            assert any(after[a][1] != before[a][1] for a in before)
        else:  # disabled: scores stand still, the timestamps move
            assert all(after[a][:2] == before[a][:2] for a in before) and not wfl.any()
            assert sum(after[a][2] == now for a in before) > 30
        now += 500
        L.decay(now, ("decay", s))
    L.m.close()


def test_set_on_a_damp_handle_restarts_the_picked_members(make, orc):
    """Membership.set over a stash of 3,000 changes with repeated addresses on a handle with damp
    on and members that already carry scores: every picked member restarts at (initial, initial,
    null), the others keep their state; then a hot batch."""
    cfg = {"dampScoringInitial": 60, "dampScoringPenalty": 251, "dampScoringMax": 1000, "dampScoringSuppressLimit": 500,
           "dampScoringHalfLife": 6, "dampScoringMin": 20}
    names = [damp_cases.addr(i + 1) for i in range(260)]
    rng = np.random.default_rng(13)
    inc = np.full(len(names), 50, np.int64)
    m = make(names[0])
    L = Live(m, orc, names, cfg)
    now = T0
    first = np.arange(0, 120, dtype=np.uint32)
    L.update(first, np.zeros(120, np.uint8), inc[first], now, "create")
    now += 1000
    ids = rng.integers(0, 120, 600).astype(np.uint32)
    st, ui = rising(rng, ids, inc)
    L.update(ids, st, ui, now, "penalize")
    # not ready: remote changes are stashed (nothing applied, no damp change), set() merges them
    m.set_ready(False)
    L.om.set_ready(False)
    for b in range(3):
        ids = rng.integers(40, 260, 1000).astype(np.uint32)  # ids 1..39 are not in the stash
        if b == 1:
            ids[:220] = np.arange(40, 260)  # every other id is, most of them many times
            ids = ids[rng.permutation(1000)]
        st, ui = rising(rng, ids, inc)
        ga, _, _, gna = m.update_ids(ids, st, ui, now_ms=now + b)
        oa, _, _, ona = L.om.update_ids(ids, st, ui, now_ms=now + b)
        assert gna == ona == 0 and not ga.any() and not oa.any()
    L.check("stashed")
    picked = m.set()
    assert L.om.set() == len(picked) and len(picked) == 220
    L.model.set([names.index(a) for a, _, _ in picked])
    L.check("set")
    sc, ls, ts = m.damp_dump()
    assert (sc[40:] == 60).all() and (ts[40:] == 0).all() and (ts[1:40] != 0).sum() > 20 and (ls[1:40] > 60).any()
    m.set_ready(True)
    L.om.set_ready(True)
    now += 2500
    ids = np.concatenate([np.full(70, 200), np.full(17, 41), np.full(16, 10), rng.integers(0, 260, 1900)]).astype(np.uint32)
    ids = ids[rng.permutation(len(ids))]
    st, ui = rising(rng, ids, inc)
    _, wsc, wfl = L.update(ids, st, ui, now, "hot after set")
    assert wfl.any() and (wsc == 1000).any()
    m.close()


def test_refusals_leave_the_state_alone(make_default, gpu, orc):
    """update_range_dev with damp on, damp_last for more changes than the last batch had, and
    damp_last(k > 0) after an empty batch are RP_EINVAL with nothing applied and no state
    change; damp_last with a null score or a null flag pointer still fills the other."""
    cfg = {"dampScoringPenalty": 251, "dampScoringMax": 1000, "dampScoringSuppressLimit": 500, "dampScoringHalfLife": 5}
    names = [damp_cases.addr(i + 1) for i in range(50)]
    rng = np.random.default_rng(14)
    inc = np.full(len(names), 3, np.int64)
    m = make_default(names[0])
    L = Live(m, orc, names, cfg)
    lib = gpu.lib()
    L.update(np.arange(50, dtype=np.uint32), np.zeros(50, np.uint8), inc.copy(), T0, "create")
    ids = rng.integers(0, 50, 300).astype(np.uint32)
    st, ui = rising(rng, ids, inc)
    _, wsc, wfl = L.update(ids, st, ui, T0 + 800, "penalize")
    assert wfl.any()
    k = len(ids)

    def last(kk, want_score=True, want_flag=True):
        sc = np.full(max(kk, 1), -1.0)
        fl = np.full(max(kk, 1), 9, np.uint8)
        rc = lib.rp_members_damp_last(m._h, sc.ctypes.data if want_score else None,
                                      fl.ctypes.data if want_flag else None, kk)
        return rc, sc[:kk], fl[:kk]

    # update_range_dev with damp on
    d_ids = torch.from_numpy(ids.view(np.int32).copy()).cuda()
    d_st = torch.from_numpy(st.copy()).cuda()
    d_inc = torch.from_numpy(ui + 5).cuda()
    d_app = torch.full((k,), 7, dtype=torch.uint8, device="cuda")
    d_na = torch.full((1,), 77, dtype=torch.int32, device="cuda")
    rc = lib.rp_members_update_range_dev(m._h, d_ids.data_ptr(), d_st.data_ptr(), d_inc.data_ptr(), k, T0 + 900, 0, 4096,
                                         d_app.data_ptr(), None, None, d_na.data_ptr(),
                                         torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == RP_EINVAL and b"damp" in lib.rp_last_error()
    assert (d_app.cpu().numpy() == 7).all() and int(d_na.item()) == 77
    L.check("after the refused range update")
    # the last batch is still the penalizing one, all k entries; k + 1 is refused
    rc, sc, fl = last(k)
    assert rc == 0 and np.array_equal(u64(sc), u64(wsc)) and np.array_equal(fl, wfl)
    rc, sc, fl = last(k + 1)
    assert rc == RP_EINVAL and (sc == -1.0).all() and (fl == 9).all()
    with pytest.raises(gpu.RingpopAmdError):
        m.damp_last(k + 1)
    # a null score or a null flag pointer: the other is filled
    rc, sc, fl = last(k, want_score=False)
    assert rc == 0 and np.array_equal(fl, wfl) and (sc == -1.0).all()
    rc, sc, fl = last(k, want_flag=False)
    assert rc == 0 and np.array_equal(u64(sc), u64(wsc)) and (fl == 9).all()
    L.check("after damp_last")
    # an empty batch is the last batch now: no scores to hand back (host and device forms)
    for form in ("host", "device"):
        if form == "host":
            ga, _, _, gna = m.update_ids(np.empty(0, np.uint32), np.empty(0, np.uint8), np.empty(0, np.int64),
                                         now_ms=T0 + 1000)
            assert gna == 0 and len(ga) == 0
        else:
            m.update_dev(None, None, None, 0, T0 + 1100, None, None, None, d_na.data_ptr(),
                         torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            assert int(d_na.item()) == 0
        assert last(0)[0] == 0
        for kk in (1, k):
            rc, sc, fl = last(kk)
            assert rc == RP_EINVAL and (sc == -1.0).all() and (fl == 9).all(), (form, kk)
        L.check(("after an empty batch", form))
        # and a real batch makes damp_last answer again
        ids2 = rng.integers(0, 50, 40).astype(np.uint32)
        st2, ui2 = rising(rng, ids2, inc)
        L.update(ids2, st2, ui2, T0 + 1500 + (form == "device") * 500, ("batch after the empty one", form))
        assert last(40)[0] == 0 and last(41)[0] == RP_EINVAL
    m.close()
