"""GPU tests of the membership checksum string and the name table on short, long and ragged
names (tests/name_cases.py; tests/test_name_cases.py shows from the inputs which branches they
reach: the byte-loop name copy, tiles written straight to global memory between staged ones, the
string pool regrown with strings pending, the radix sort over prefixes and a growing longest name).

Reference: generateChecksumString restated in Python (name_cases.checksum_string: the existing
members sorted by address bytes, address + status + incarnation joined by ';') over the CPU
oracle's member table, hashed by the oracle's farmhash32; and the oracle's own string and checksum.
Exact comparisons."""
import numpy as np
import pytest

import name_cases as nc

pytestmark = pytest.mark.gpu

MODES = {"deferred": None, "inline": "0", "stream": "1"}


def _knobs(monkeypatch, mode, fold):
    monkeypatch.delenv("RP_MEMBERS_SIDE_BUILD", raising=False)
    if MODES[mode] is not None:
        monkeypatch.setenv("RP_MEMBERS_SIDE_BUILD", MODES[mode])
    if fold == "bucket":
        monkeypatch.setenv("RP_MEMBERS_BUCKET_FOLD", "1")


def _state(orc, o, names):
    out = {}
    for a in names:
        m = o.member(a)
        if m is not None:
            out[a] = (orc.STATUS[m["status"]], m["incarnationNumber"])
    return out


def _compare(orc, m, o, names, what):
    want = nc.checksum_string(_state(orc, o, names))
    assert want.decode() == o.checksum_string(), what
    assert m.checksum == orc.hash32(want) == o.checksum, what
    assert m.generate_checksum_string().encode() == want, what
    assert m.checksum == o.checksum, what  # (again: after the string was read back)


@pytest.mark.parametrize("fold", ["default", "bucket"])
@pytest.mark.parametrize("mode", list(MODES))
def test_mixed_names_checksum_string(gpu, orc, mode, fold, monkeypatch):
    """About 1,100 names of 1..262 bytes interned in shuffled order, every fifth left non-existent;
    three batches through the four statuses and incarnations of 1..19 characters. After every
    batch the string and the checksum, in the three string modes and both folds."""
    _knobs(monkeypatch, mode, fold)
    names = nc.mixed_names()
    m = gpu.Membership()
    ids = np.asarray(m.intern(names), dtype=np.uint32)
    o = orc.Members(names)
    for j, (idx, st, inc) in enumerate(nc.mixed_batches(names)):
        ga, gs, gi, gna = m.update_ids(ids[idx], st, inc, now_ms=1434500000000 + j)
        oa, os_, oi, ona = o.update_ids(idx, st, inc, False, 1434500000000 + j)
        assert gna == ona and np.array_equal(ga > 0, oa > 0), j
        _compare(orc, m, o, names, (mode, fold, j))
    ex, dst, dinc = m.dump()
    state = _state(orc, o, names)
    assert {a: (int(dst[i]), int(dinc[i])) for a, i in zip(names, ids) if ex[i]} == state
    m.close()


@pytest.mark.parametrize("mode", list(MODES))
def test_mixed_names_unread_batches(gpu, orc, mode, monkeypatch):
    """The same batches without a read in between (the strings wait in their slots; in the default
    mode batch b's string rides on batch b + 1's fold launch): one comparison at the end."""
    _knobs(monkeypatch, mode, "default")
    names = nc.mixed_names()
    m = gpu.Membership()
    ids = np.asarray(m.intern(names), dtype=np.uint32)
    o = orc.Members(names)
    for j, (idx, st, inc) in enumerate(nc.mixed_batches(names)):
        m.update_ids(ids[idx], st, inc, now_ms=1434500000000 + j)
        o.update_ids(idx, st, inc, False, 1434500000000 + j)
    _compare(orc, m, o, names, mode)
    m.close()


@pytest.mark.parametrize("slots", [None, "3"], ids=["default-pool", "three-slots"])
def test_growing_table_checksum_string(gpu, orc, slots, monkeypatch):
    """Four steps, each interning one more family and folding one batch: c2-style names; every
    length 1..70; a run of 90..130-byte names that sorts into the middle and raises the longest
    name; host names past 200 bytes with names that sort before everything held. The string and
    the checksum are compared after every step. After the comparison two more batches are folded
    and left unread, so the next step's first fold, whose string outgrows the slots, finds strings
    pending (flush, release and re-plan of the pool under pending strings; with
    RP_MEMBERS_GROUP_SLOTS=3 the two pending strings are most of a group). After step 2 the wire
    decoder also runs on the same handle over a pending string (it builds the name index and the
    sort), and the checksum is compared again."""
    if slots:
        monkeypatch.setenv("RP_MEMBERS_GROUP_SLOTS", slots)
    import pywire
    steps = nc.growing_steps()
    every = [a for fam, _ in steps for a in fam]
    o = orc.Members(every)
    oidx = {a: i for i, a in enumerate(every)}
    m = gpu.Membership()
    held = []
    now = [1434500000000]

    def fold(names, st, inc):
        now[0] += 1
        _, _, _, gna = m.update_ids(m.intern(names), st, inc, now_ms=now[0])
        _, _, _, ona = o.update_ids([oidx[a] for a in names], st, inc, False, now[0])
        assert gna == ona > 0
        return gna

    for j, (fam, upd) in enumerate(steps):
        m.intern(fam)  # with two strings pending from the step before
        held += fam
        st = [(i + j) % 4 for i in range(len(upd))]
        inc = [nc.INCARNATIONS[(7 * i + j) % len(nc.INCARNATIONS)] for i in range(len(upd))]
        fold(upd, st, inc)  # the string outgrows its slot here
        _compare(orc, m, o, held, (slots, j))
        sel = [i for i in range(len(upd)) if inc[i] < (1 << 60) - 4]
        bump = lambda k: fold([upd[i] for i in sel[k::3]], [0] * len(sel[k::3]), [inc[i] + 1 for i in sel[k::3]])  # noqa: E731
        if j == 1:
            bump(2)  # unread: its string is pending while the decoder builds the index and the sort
            recs = [pywire.full_sync_record(held[0], a, "suspect", 5 + i) for i, a in enumerate(held[::97])]
            texts = [pywire.body(recs), pywire.body(recs[:3], "ping", checksum=7, source=held[401], source_inc=9)]
            d = gpu.wire_decode(m, texts)
            assert (d["err"] == 0).all()
            assert [m.address(int(x)) for x in d["addr"][:len(recs)]] == held[::97]
            assert m.address(int(d["source"][1])) == held[401]
            _compare(orc, m, o, held, (slots, j, "after the decoder"))
        bump(0)  # two unread batches: pending when the next step interns and folds
        bump(1)
    _compare(orc, m, o, held, (slots, "end"))
    assert len(held) == len(every) <= 1500
    m.close()


def test_mixed_names_membership_set(gpu, orc):
    """Membership.set over a stash of the mixed set's batches (received before the node is ready):
    the picks, the member table's string and the checksum."""
    names = nc.mixed_names()
    m = gpu.Membership()
    ids = np.asarray(m.intern(names), dtype=np.uint32)
    o = orc.Members(names)
    m.set_ready(False)
    o.set_ready(False)
    for idx, st, inc in nc.mixed_batches(names):
        m.update_ids(ids[idx], st, inc)
        o.update_ids(idx, st, inc)
    picks = m.set()
    assert o.set() == len(picks) > 800
    m.set_ready(True)
    o.set_ready(True)
    _compare(orc, m, o, names, "set")
    state = _state(orc, o, names)
    assert {a: (orc.STATUS[s], i) for a, s, i in picks} == state
    m.close()
