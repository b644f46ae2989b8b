"""CPU checks of the boundary rings (tests/ring_boundary_cases.py): every construction claim a GPU
test relies on, and the oracle's lookupN on those rings against a plain numpy walk.

The reference below knows nothing of buckets, windows or fingerprints: the first ring position
with token >= hash (np.searchsorted, "left"), wrapped past the end, then the first n distinct
owners in ring order. Every key is compared, for n = -1..4 (n <= 0: lookupN's single step, which
does not wrap, lib/ring/index.js:157-189).
"""
import numpy as np
import pytest

import ring_boundary_cases as rb

NIL = 0xFFFFFFFF


def ref_lookupn(T, O, nserv, H, n):
    """(owners [k, max(n, 1)], counts [k]) of lookupN(hash, n) over the sorted ring (T, O)."""
    M = len(T)
    pos = np.searchsorted(T, H, "left")
    w = max(n, 1)
    out = np.full((len(H), w), NIL, dtype=np.uint32)
    cnt = np.zeros(len(H), dtype=np.uint8)
    if n <= 0:
        hit = pos < M
        out[hit, 0] = O[pos[hit]]
        cnt[hit] = 1
        return out, cnt
    need = min(n, nserv)
    for step in range(M):
        o = O[(pos + step) % M]
        new = (cnt < need) & (out != o[:, None]).all(axis=1)
        out[new, cnt[new]] = o[new]
        cnt[new] += 1
        if (cnt >= need).all():
            break
    return out, cnt


def test_reference_walk_on_a_hand_ring():
    """The numpy walk itself, on a ring small enough to read."""
    T = np.array([10, 20, 20, 30, 40], dtype=np.uint32)
    O = np.array([0, 1, 2, 1, 0], dtype=np.uint32)
    H = np.array([0, 10, 11, 20, 21, 40, 41], dtype=np.uint32)
    own, cnt = ref_lookupn(T, O, 3, H, 3)
    assert own.tolist() == [[0, 1, 2], [0, 1, 2], [1, 2, 0], [1, 2, 0], [1, 0, 2], [0, 1, 2], [0, 1, 2]]
    assert cnt.tolist() == [3] * 7
    own, cnt = ref_lookupn(T, O, 3, H, 0)
    assert own[:, 0].tolist() == [0, 0, 1, 1, 1, 0, NIL] and cnt.tolist() == [1, 1, 1, 1, 1, 1, 0]
    own, cnt = ref_lookupn(T, O, 3, H, 4)
    assert own[0].tolist() == [0, 1, 2, NIL] and cnt.tolist() == [3] * 7


@pytest.fixture(scope="module")
def hashes(orc):
    return rb.keys_and_hashes(orc)[1]


@pytest.mark.parametrize("name", rb.CASE_NAMES)
def test_construction(orc, hashes, name):
    c = rb.cases(orc)[name]
    H = hashes
    T, O = c.sorted_ring()
    assert c.rows.shape == (c.nserv, c.R) and len(T) == c.M
    assert (np.diff(T.astype(np.int64)) > 0).all()
    assert c.M == c.rows.size or name.startswith("edge-values")
    assert (c.fsh == 0) == (c.regime == "exact")
    assert c.hint_fits()  # the sorted kernel can take the tiles
    counts = c.bucket_counts()
    assert (counts.max() <= 15) == c.compact
    assert counts.max() == (15 if c.dense and c.compact else 16 if c.dense else counts.max())
    nlists = rb.NKEYS // rb.LIST
    ties = c.tie_keys(H)
    per_list = ties[:nlists * rb.LIST].reshape(nlists, rb.LIST).sum(axis=1)

    if name.startswith("at-") and name != "at-fp-sparse":
        # a third of the keys on a token, a third just under one, a third just over one
        inring = c.on_token(H)
        assert inring.sum() >= (c.M + 2) // 3
        assert np.isin(H + np.uint32(1), T).sum() >= c.M // 3 - 1
        assert np.isin(H - np.uint32(1), T).sum() >= c.M // 3 - 1
        assert (per_list > rb.SLOTS).all()  # every list holds more tie keys than it has slots
        assert (c.cb, c.fsh) == (14, 0 if c.regime == "exact" else 4)
    if name == "at-fp-sparse":
        assert per_list.tolist() == rb.SPARSE_TIES and len(rb.SPARSE_TIES) == nlists
        assert ties[nlists * rb.LIST:].sum() == 0
        assert c.fsh == 4
        # the three kinds in equal parts (a token on, one over, one under the key's hash)
        on, over, under = c.on_token(H), np.isin(H + np.uint32(1), T), np.isin(H - np.uint32(1), T)
        assert not (on & over).any() and not (on & under).any() and not (over & under).any()
        assert np.array_equal(ties, on | over | under)
        assert [int(x.sum()) for x in (on, under, over)] == [sum((t - k + 2) // 3 for t in rb.SPARSE_TIES) for k in (0, 1, 2)]
    if name in ("at-exact", "at-fp", "at-fp-sparse", "buckets", "buckets-fp"):
        assert (O[1:] != O[:-1]).all()  # rr: successive owners differ
    if name.endswith("-runs"):
        run = np.diff(np.flatnonzero(np.concatenate([[True], O[1:] != O[:-1], [True]])))
        assert sorted(set(run.tolist())) == sorted(set(rb.RUN_LENGTHS))
    if name == "ends-quarter" or name.startswith("edge-values"):
        inner = T[(T != 0) & (T != NIL)]
        assert inner.min() >= (1 << 30) and inner.max() < (3 << 30)
        assert 0.2 < (H < inner.min()).mean() < 0.3 and 0.2 < (H > inner.max()).mean() < 0.3
    if name == "ends-quarter":
        assert not c.on_token(H).any()
        assert c.must_defer(H).sum() > rb.NKEYS // 5
    if name == "ends-sliver":
        n = rb.NKEYS
        assert 0.0045 * n < (H < T[0]).sum() < 0.0055 * n and 0.0045 * n < (H > T[-1]).sum() < 0.0055 * n
        assert c.fsh > 0 and not c.on_token(H).any()
    if name.startswith("edge-values"):
        assert T[0] == 0 and T[-1] == NIL and O[-1] == 3 and c.nserv == 4 and c.ob == 2
        for d in c.dup:  # a key hash, in two servers' rows: the ring keeps the one inserted first
            assert d in H
            srv = np.flatnonzero((c.rows == d).any(axis=1))
            assert len(srv) == 2 and O[T == d].tolist() == [srv[0]]
        assert c.M == c.rows.size - 3
        rmask = (1 << (32 - c.cb)) - 1
        last = (((int(T[-1]) & rmask) >> c.fsh) << c.ob) | int(O[-1])
        if name == "edge-values-pad":  # 22 fingerprint bits in full: the last entry is k_pack3's pad value
            assert c.cb == 10 and last == 0xFFFFFF
        else:
            assert last == (1 << (32 - c.cb + c.ob)) - 1  # all ones
    if c.dense:
        assert c.cb == 13
        hist = np.bincount(counts, minlength=17)
        want = {}
        for b, place, n in c.dense:
            want[n] = want.get(n, 0) + 1
            assert counts[b] == n
            base = b << 19
            t = T[(T >> np.uint32(19)) == b].astype(np.int64)
            if place == "low":
                assert t.max() < base + (1 << 15)
            if place == "high":
                assert t.min() >= base + (1 << 19) - (1 << 15)
            if place == "even":  # no sixteenth of the range holds more than two of them
                assert np.bincount((t - base) >> 15, minlength=16).max() <= 2
        for n, k in want.items():
            assert hist[n] == k and (k >= 100 or n == 16)
        assert hist[2:].sum() == len(c.dense)  # every other bucket holds 0 or 1
        kinds = {(p, n) for _, p, n in c.dense}
        assert kinds >= set(rb.DENSE_KINDS)
        for kind in rb.DENSE_KINDS:
            assert sum((p, n) == kind for _, p, n in c.dense) >= 100
        in_dense = np.isin(H >> np.uint32(19), [b for b, _, _ in c.dense])
        assert in_dense.sum() >= 1000
        on = c.on_token(H)
        assert (on & in_dense).sum() >= 100  # keys on a token inside the long buckets
        # ... at every depth: a tie token at bucket positions 0..14
        depth = set()
        for h in H[on & in_dense]:
            j = int(np.searchsorted(T, h, "left"))
            depth.add(j - int(np.searchsorted(T, np.uint32((int(h) >> 19) << 19), "left")))
        assert depth >= set(range(15))


@pytest.mark.parametrize("name", rb.CASE_NAMES)
def test_oracle_vs_numpy_walk(orc, hashes, name):
    c = rb.cases(orc)[name]
    T, O = c.sorted_ring()
    oracle = rb.oracle_ring(orc, c)
    assert oracle.token_count() == c.M and oracle.server_count() == c.nserv
    assert [oracle.name(i) for i in range(c.nserv)] == c.servers  # ids are the row numbers
    ot, oo = oracle.dump()
    assert np.array_equal(ot, T) and np.array_equal(oo, O)
    for n in (-1, 0, 1, 2, 3, 4):
        want, wcnt = ref_lookupn(T, O, c.nserv, hashes, n)
        got, gcnt = rb.oracle_rows(orc, c, n)
        assert np.array_equal(gcnt, wcnt), n
        assert np.array_equal(got, want), n


@pytest.mark.parametrize("name", rb.CASE_NAMES)
def test_lower_bounds(orc, hashes, name):
    """What the GPU test asserts against: from the tokens and hashes alone."""
    c = rb.cases(orc)[name]
    nlists = rb.NKEYS // rb.LIST
    deferred, over = c.deferred_lower_bound(hashes, nlists * rb.LIST)
    above = int((hashes[:nlists * rb.LIST] > c.rows.max()).sum())
    ties = int(c.tie_keys(hashes)[:nlists * rb.LIST].sum())
    assert ties >= int(c.on_token(hashes)[:nlists * rb.LIST].sum())
    assert deferred == above + (ties if c.fsh > 0 else 0)  # (no key is both)
    if name == "at-fp":
        assert over == nlists and deferred >= 8000 * 2
    if name == "at-fp-sparse":
        assert over >= sum(t > rb.SLOTS for t in rb.SPARSE_TIES) == 4 and over < nlists
        assert 0 < deferred < nlists * rb.LIST
    if name in ("ends-quarter",):
        assert over == nlists
    if name == "ends-sliver":
        assert 0 < deferred and over == 0
    if name.startswith("edge-values"):
        assert (deferred, over) == (0, 0)  # 2^32 - 1 is a token: no key lies above the last one
    if c.regime == "exact" and name.startswith("at-"):
        assert deferred == above  # a key on a token resolves on the fast path


@pytest.mark.parametrize("name", rb.CASE_NAMES)
def test_thin_order(orc, hashes, name):
    """The second key order of the GPU test: a permutation whose first lists hold few keys that a
    fast path has to defer, for every case whose natural order overflows lists by its design."""
    c = rb.cases(orc)[name]
    order = c.thin_order(hashes)
    nlists = rb.NKEYS // rb.LIST
    heavy = c.heavy_keys(hashes)
    assert (heavy | ~c.must_defer(hashes)).all()
    if order is None:
        per = heavy[:nlists * rb.LIST].reshape(nlists, rb.LIST).sum(axis=1)
        assert name in ("at-exact", "at-exact-runs", "at-fp", "ends-sliver", "at-fp-sparse"), per
        return
    assert np.array_equal(np.sort(order), np.arange(rb.NKEYS))
    per = heavy[order][:nlists * rb.LIST].reshape(nlists, rb.LIST).sum(axis=1)
    assert (per[:rb.THIN_LISTS] == rb.THIN_HEAVY).all() and rb.THIN_HEAVY < rb.SLOTS
    if c.dense:  # the long buckets' keys that two windows can resolve, in the thin lists
        in_dense = np.isin(hashes >> np.uint32(19), [b for b, _, _ in c.dense])
        assert (in_dense & ~heavy)[order][:rb.THIN_LISTS * rb.LIST].sum() >= 500


# -- the wide variants: the same token sets on ids that follow id_base filler names

WIDE_OB = {16384: 14, 16385: 15, 32769: 16, 65534: 16, 65536: 16, 65537: 17}
SPARSE_FSH = {16384: 8, 16385: 9, 32769: 10, 65536: 10, 65537: 11}  # M = 25,000: cb 14; 4 at 1,000 names


@pytest.mark.parametrize("name", rb.WIDE_CASE_NAMES + [rb.SERVICE_TABLE_CASE])
def test_wide_construction(orc, hashes, name):
    c = rb.cases(orc)[name]
    H = hashes
    base, N = name.split("@")[0], int(name.split("@")[1])
    narrow = rb.cases(orc)[base]
    T, O = c.sorted_ring()
    assert c.N == N == c.id_base + c.nserv and c.nserv == rb.WIDE_SERVERS
    assert len(T) == c.M and (np.diff(T.astype(np.int64)) > 0).all()
    # the layout parameters: ids in ob bits, 24 - ob fingerprint bits of the 32 - cb below the bucket
    cb = int(np.log2(c.M))
    assert (1 << cb) <= c.M < (2 << cb)
    assert (c.cb, c.ob, c.fsh) == (cb, WIDE_OB[N], (32 - cb) - (24 - WIDE_OB[N]))
    assert (1 << (c.ob - 1)) < N <= (1 << c.ob) and c.fsh > 0
    assert c.compact == (N <= 65536) and c.bucket_counts().max() <= 15
    assert c.hint_fits()
    # every id of id_base .. N - 1 owns tokens, the highest one too
    assert np.array_equal(np.unique(O), np.arange(c.id_base, N))
    assert (O[1:] != O[:-1]).all()
    ft = c.filler_tokens()
    assert len(ft) == c.id_base * c.R and len(np.unique(ft)) == len(ft)
    assert len(set(c.filler_names())) == c.id_base and not set(c.filler_names()) & set(c.servers)
    nlists = rb.NKEYS // rb.LIST
    ties = c.tie_keys(H)
    deferred, over = c.deferred_lower_bound(H, nlists * rb.LIST)
    above = int((H[:nlists * rb.LIST] > c.rows.max()).sum())
    assert deferred == above + int(ties[:nlists * rb.LIST].sum())
    order = c.thin_order(H)
    assert order is not None and np.array_equal(np.sort(order), np.arange(rb.NKEYS))
    heavy = c.heavy_keys(H)
    assert (heavy | ~c.must_defer(H)).all()
    per = heavy[order][:nlists * rb.LIST].reshape(nlists, rb.LIST).sum(axis=1)
    assert (per[:rb.THIN_LISTS] == rb.THIN_HEAVY).all()

    if base == "at-fp-sparse":
        assert c.fsh == SPARSE_FSH[N] and narrow.fsh == 4 and c.M == narrow.M == 25000
        per_list = ties[:nlists * rb.LIST].reshape(nlists, rb.LIST).sum(axis=1)
        assert per_list.tolist() == rb.SPARSE_TIES and ties[nlists * rb.LIST:].sum() == 0
        on, over_, under = c.on_token(H), np.isin(H + np.uint32(1), T), np.isin(H - np.uint32(1), T)
        assert np.array_equal(ties, on | over_ | under) and np.array_equal(under, c.under_ties(H))
        assert [int(x.sum()) for x in (on, under, over_)] == [sum((t - k + 2) // 3 for t in rb.SPARSE_TIES) for k in (0, 1, 2)]
        assert over >= sum(t > rb.SLOTS for t in rb.SPARSE_TIES) == 4 and over < nlists
        # the thin lists each hold designed one-under ties: a fast path that does not defer them
        # leaves a wrong row that no whole-list redo repairs
        thin_under = under[order][:rb.THIN_LISTS * rb.LIST].reshape(rb.THIN_LISTS, rb.LIST).sum(axis=1)
        assert (thin_under >= 1).all(), thin_under
    if base == "edge-values":
        assert np.array_equal(np.sort(c.rows.reshape(-1)), np.sort(rb.edge_tokens(H, rb.WIDE_SERVERS, 1)[0]))
        assert T[0] == 0 and T[-1] == NIL and O[-1] == N - 1  # the highest id owns 2^32 - 1
        assert c.M == c.rows.size - 3 and c.R <= 12
        for d in c.dup:
            srv = np.flatnonzero((c.rows == d).any(axis=1))
            assert d in H and len(srv) == 2 and O[T == d].tolist() == [c.id_base + srv[0]]
        inner = T[(T != 0) & (T != NIL)]
        assert 0.2 < (H < inner.min()).mean() < 0.3 and 0.2 < (H > inner.max()).mean() < 0.3
        rmask = np.uint32((1 << (32 - c.cb)) - 1)
        ent = (((T & rmask) >> np.uint32(c.fsh)) << np.uint32(c.ob)) | O
        assert ent.max() < (1 << 24) or not c.compact
        if N in (16384, 65536):  # ids fill the owner field: the last entry is k_pack3's pad value
            assert N == 1 << c.ob and np.flatnonzero(ent == 0xFFFFFF).tolist() == [c.M - 1]
        else:
            assert not (ent == 0xFFFFFF).any()
    if base == "buckets-fp":
        assert np.array_equal(c.rows, narrow.rows) and c.dense == narrow.dense
        counts = c.bucket_counts()
        assert all(counts[b] == n for b, _, n in c.dense) and counts.max() == 15
        assert deferred >= 200 and over == 0


@pytest.mark.parametrize("name", rb.WIDE_CASE_NAMES + [rb.SERVICE_TABLE_CASE])
def test_wide_oracle_vs_numpy_walk(orc, hashes, name):
    """The oracle after the filler call (one add_remove that adds and removes every filler): the
    names keep their ids, the ring is the servers' alone, and its rows are the numpy walk's."""
    c = rb.cases(orc)[name]
    T, O = c.sorted_ring()
    oracle = rb.oracle_ring(orc, c)
    assert oracle.token_count() == c.M and oracle.server_count() == c.nserv
    assert [oracle.name(c.id_base + i) for i in range(c.nserv)] == c.servers
    assert [oracle.name(i) for i in (0, c.id_base - 1)] == ["fill-0:1", "fill-%d:1" % (c.id_base - 1)]
    ot, oo = oracle.dump()
    assert np.array_equal(ot, T) and np.array_equal(oo, O)
    for n in (-1, 0, 1, 2, 3, 4):
        want, wcnt = ref_lookupn(T, O, c.nserv, hashes, n)
        got, gcnt = rb.oracle_rows(orc, c, n)
        assert np.array_equal(gcnt, wcnt), n
        assert np.array_equal(got, want), n
