"""Rings whose tokens sit where the batch lookup kernels branch (rp_ring.hip: LkStages::resolve /
finish2 and their older copies), built from caller tokens so that device keys, which the device
always farmhashes, meet them: a key hash equal to a token, one below and one above it, in the exact
(fsh == 0) and the fingerprint (fsh > 0) regime of the compact layout; keys below the first and
above the last token; tokens 0 and 2^32 - 1; a token in two servers' rows (the first one stays);
buckets of 6, 10, 11 and 15 tokens spread or clustered, and one of 16 (the compact layout is then
not built).

A case may sit at an id base: that many filler names (`fill-<i>:1`) are interned before its
servers, by one add_remove call that adds and removes them with distinct caller tokens, so the
ring is empty again and the servers' ids are id_base + row. The wide variants (WIDE_CASE_NAMES,
`<case>@<names>`) put three of the token sets on ids of 14, 15, 16 and 17 bits, where the layouts
change: the LDS index is built up to 14 bits, the compact layout up to 16 with fingerprints of
24 - ob bits, and at exactly 2^ob names the highest id is all ones in the owner field, so that
with token 2^32 - 1 a real entry equals the value k_pack3 pads the entries with.

No torch, no GPU: everything derives from the sorted tests' keys, uuid_keys(42, 0, NKEYS), and
their host hashes H. A case holds the per-server token rows; hash_func() turns them into the
dict-backed hashFunc of the device HashRing, and the same rows go to the oracle's add_remove, so
both rings are built from one table. tests/test_ring_boundary_cases.py checks every construction
claim made here and the oracle against a numpy walk; tests/test_ring_boundary_gpu.py runs the
kernels.
"""
import numpy as np

NKEYS = 3 * 8 * 1024 + 777  # test_ring_sorted_gpu.NMAX: three 1024-thread tiles and a tail
LIST = 2048                 # keys per deferred-key list of the lean and sorted kernels
SLOTS = 32                  # kSlowPerTile: a list with more deferred keys overflows
# tie keys per whole list of at-fp-sparse: none, one, one under / at / over the list's slots, two lists' worth
SPARSE_TIES = [0, 1, 31, 32, 33, 64] * 2
# thin_order: the first THIN_LISTS lists hold at most THIN_HEAVY keys that a fast path has to defer
THIN_LISTS, THIN_HEAVY = 8, 16
# runs: run k of consecutive sorted tokens has RUN_LENGTHS[k % 6] tokens of server k % nserv
RUN_LENGTHS = [1, 1, 2, 3, 5, 8]
# the dense buckets of the `buckets` cases: (placement, tokens), bucket k of them has kind k % 6
DENSE_KINDS = [("even", 10), ("even", 11), ("even", 15), ("low", 15), ("high", 15), ("high", 6)]
N_DENSE = 612  # 102 buckets of each kind


def compact_params(M, nnames):
    """(cb, ob, fsh) as ring_build_compact computes them: 2^cb buckets with cb = floor(log2 M),
    owner ids in ob bits, fingerprints of 24 - ob bits shifted down by fsh."""
    ob = 1
    while (1 << ob) < nnames:
        ob += 1
    cb = 3
    while cb < 24 and (2 << cb) <= M:
        cb += 1
    rb, fb = 32 - cb, 24 - ob
    return cb, ob, 0 if fb >= rb else rb - fb


class Case:
    def __init__(self, name, rows, regime, compact=True, dense=(), ties_per_list=None, id_base=0):
        self.name = name
        self.id_base = id_base    # filler names interned before the servers: their ids are id_base + row
        self.rows = np.ascontiguousarray(rows, dtype=np.uint32)  # [servers, R]: server s's tokens in add order
        self.nserv, self.R = self.rows.shape
        self.servers = ["bnd-%d:3000" % s for s in range(self.nserv)]
        self.regime = regime      # "exact": fsh == 0; "fp": fsh > 0
        self.compact = compact    # False: a bucket of 16 tokens or ids past 16 bits, the compact layout is not built
        self.dense = list(dense)  # [(bucket, placement, tokens)] of the designed buckets
        self.ties_per_list = ties_per_list  # designed tie keys per whole list, or None
        self.M = len(np.unique(self.rows))  # ring size: a token already in the ring is not inserted again
        self.N = id_base + self.nserv  # names interned once the ring is built
        self.cb, self.ob, self.fsh = compact_params(self.M, self.N)

    def filler_names(self):
        return ["fill-%d:1" % i for i in range(self.id_base)]

    def filler_tokens(self):
        """R distinct caller tokens per filler (an odd multiplier permutes the 32-bit values)."""
        return filler_tokens(0, self.id_base, self.R)

    def add_tokens(self):
        """The rows as orc.Ring.add_remove(servers, [], add_tokens, None) takes them."""
        return self.rows.reshape(-1)

    def hash_func(self, fallback):
        """hashFunc of the device HashRing: server + str(i) -> rows[server][i]; any other string
        (the checksum string) goes to `fallback` (farmhash32, as the oracle hashes it). The fillers
        never reach it: their tokens go to rp_ring_add_remove as an array (filler_tokens)."""
        table = {s + str(i): int(t) for s, row in zip(self.servers, self.rows) for i, t in enumerate(row)}
        return lambda x: table[x] if x in table else fallback(x)

    def sorted_ring(self):
        """(tokens, owners) in ring order. Of equal tokens the first inserted stays (RBTree.insert
        finds the value and adds no node, lib/ring/rbtree.js:70-137; servers are added in row order)."""
        flat = self.rows.reshape(-1)
        order = np.argsort(flat, kind="stable")
        order = order[np.concatenate([[True], np.diff(flat[order].astype(np.int64)) > 0])]
        return flat[order], (self.id_base + order // self.R).astype(np.uint32)

    def bucket_counts(self):
        """Tokens per bucket of the compact layout."""
        return np.bincount(self.sorted_ring()[0] >> np.uint32(32 - self.cb), minlength=1 << self.cb)

    def hint_fits(self):
        """k_cindex_hint's condition: every group's first position within 14 signed bits of
        g * M >> (cb - 3). The sorted kernel needs the hinted index."""
        T, _ = self.sorted_ring()
        g = np.arange(1 << (self.cb - 3), dtype=np.int64)
        base = np.searchsorted(T, (g << (35 - self.cb)).astype(np.uint32), "left")
        delta = base - ((g * self.M) >> (self.cb - 3))
        return bool((delta >= -8192).all() and (delta <= 8191).all())

    # -- what a fast-path kernel must defer, from the tokens and the key hashes alone
    def on_token(self, H):
        """Keys whose hash equals a token."""
        return np.isin(H, self.rows.reshape(-1))

    def tie_keys(self, H):
        """Keys with a token of their own fingerprint right at their ring position: the hash itself,
        or one under or one over it with the same hash >> fsh (in the exact regime only the hash
        itself). One under is the entry just below the key's position and one over the entry at it,
        in the key's bucket, so every window that finds the position holds that entry."""
        t = self.rows.reshape(-1)
        sh = np.uint32(self.fsh)
        under, over = H - np.uint32(1), H + np.uint32(1)
        return (np.isin(H, t) | (np.isin(under, t) & (under >> sh == H >> sh)) |
                (np.isin(over, t) & (over >> sh == H >> sh)))

    def under_ties(self, H):
        """The one-under kind of tie_keys alone: a token one under the hash, with its fingerprint."""
        under = H - np.uint32(1)
        return np.isin(under, self.rows.reshape(-1)) & (under >> np.uint32(self.fsh) == H >> np.uint32(self.fsh))

    def must_defer(self, H):
        """A lower bound of the deferred set: a key above the last token (its bucket ends the ring:
        lo + 20 > M), and in the fingerprint regime a tie key (equal fingerprints, tie && !exact).
        Other causes exist (a full second-window list, a position past the second window, the last
        20 ring entries, fingerprints equal further off); they only add to it."""
        m = H > self.rows.max()
        if self.fsh > 0:
            m = m | self.tie_keys(H)
        return m

    def heavy_keys(self, H):
        """Keys a two-window kernel very likely defers: must_defer, a bucket that starts within the
        last 20 ring entries, any token of the key's bucket and fingerprint (fsh > 0), and a
        position 10 or more entries into its bucket. Only thin_order uses it: nothing is asserted
        of it."""
        T, _ = self.sorted_ring()
        bsh = np.uint32(32 - self.cb)
        lo = np.searchsorted(T, (H >> bsh) << bsh, "left")
        m = self.must_defer(H) | (lo + 20 > self.M) | (np.searchsorted(T, H, "left") - lo >= 10)
        if self.fsh > 0:
            m = m | np.isin(H >> np.uint32(self.fsh), T >> np.uint32(self.fsh))
        return m

    def thin_order(self, H):
        """A key order in which the first THIN_LISTS lists hold at most THIN_HEAVY heavy keys each
        (a list with more than SLOTS deferred keys is redone whole by the exact pass, which would
        hide what the fast path made of its keys) and the other lists the rest; None where the
        natural order is already that thin or too few light keys exist."""
        heavy = self.heavy_keys(H)
        nlists = len(H) // LIST
        per = heavy[:nlists * LIST].reshape(nlists, LIST).sum(axis=1)
        hv, lt = np.flatnonzero(heavy), np.flatnonzero(~heavy)
        if (per <= THIN_HEAVY).all() or len(lt) < THIN_LISTS * LIST or len(hv) < THIN_LISTS * THIN_HEAVY:
            return None
        if self.id_base and self.ties_per_list:
            # a wide fingerprint shift makes many undesigned keys heavy: deal the designed one-under
            # ties over the thin lists first, so that each of them holds some
            u = np.flatnonzero(self.under_ties(H))
            rest = np.setdiff1d(hv, u)
            k = min(len(u) // THIN_LISTS, THIN_HEAVY)
            head = np.concatenate([np.concatenate([u[l * k:(l + 1) * k], rest[l * (THIN_HEAVY - k):(l + 1) * (THIN_HEAVY - k)]])
                                   for l in range(THIN_LISTS)])
            hv = np.concatenate([head, np.setdiff1d(hv, head)])
        order, h0, l0 = [], 0, 0
        for l in range(nlists):
            nh = THIN_HEAVY if l < THIN_LISTS else (len(hv) - THIN_LISTS * THIN_HEAVY) // (nlists - THIN_LISTS)
            nh = min(nh, LIST)
            part = np.concatenate([hv[h0:h0 + nh], lt[l0:l0 + LIST - nh]])
            order.append(np.sort(part))
            h0, l0 = h0 + nh, l0 + LIST - nh
        order.append(np.sort(np.concatenate([hv[h0:], lt[l0:]])))
        order = np.concatenate(order)
        assert np.array_equal(np.sort(order), np.arange(len(H)))
        return order

    def deferred_lower_bound(self, H, done):
        """(deferred keys, overflowed lists) at least, among the first `done` keys (whole lists)."""
        assert done % LIST == 0
        per = self.must_defer(H)[:done].reshape(-1, LIST).sum(axis=1)
        return int(per.sum()), int((per > SLOTS).sum())


def rows_rr(tok, nserv):
    """Sorted tokens dealt round-robin: successive ring entries have different owners."""
    assert len(tok) % nserv == 0
    return tok.reshape(len(tok) // nserv, nserv).T


def rows_runs(tok, nserv):
    """Sorted tokens in runs of RUN_LENGTHS tokens of one server, run k on server k % nserv:
    a row of distinct owners needs a walk past a whole run (up to 8 entries)."""
    block = sum(RUN_LENGTHS) * nserv
    assert len(tok) % block == 0 and nserv % len(RUN_LENGTHS) != 0
    nruns = len(tok) // block * len(RUN_LENGTHS) * nserv
    k = np.arange(nruns)
    owner = np.repeat(k % nserv, np.array(RUN_LENGTHS)[k % len(RUN_LENGTHS)])
    return np.stack([tok[owner == s] for s in range(nserv)])


def _sorted_u32(x):
    x = np.sort(np.asarray(x, dtype=np.int64), kind="stable")
    assert x[0] >= 0 and x[-1] <= 0xFFFFFFFF
    return x.astype(np.uint32)


def at_tokens(H):
    """H[i], H[i] + 1, H[i] - 1 by i % 3 over the sorted hashes: a third of the keys sit on a
    token, a third one below one, a third one above one."""
    hs = np.sort(H).astype(np.int64)
    t = _sorted_u32(hs + np.array([0, 1, -1])[np.arange(len(hs)) % 3])
    assert (np.diff(t.astype(np.int64)) > 0).all()  # no two key hashes within 2 of each other
    return t


def midpoints(hs):
    """A token strictly between each pair of neighbouring sorted hashes (none where they touch)."""
    hs = hs.astype(np.int64)
    gap = np.diff(hs)
    return (hs[:-1] + gap // 2)[gap >= 2].astype(np.uint32)


def pick(a, k):
    """k of a's entries, evenly."""
    assert 0 < k <= len(a)
    return a[(np.arange(k) * len(a)) // k]


def sparse_tokens(H, M, fsh=4):
    """at-fp-sparse: list l of 2,048 consecutive keys has SPARSE_TIES[l] tie keys (spread through the
    list): a token on the key's hash, one under it or one over it in turn, the last two with the
    key's fingerprint at the ring's fsh (the hash's low fsh bits are neither all zeros nor all
    ones; 4 for the 1,000 names of at-fp-sparse). Every other token
    is a midpoint between neighbouring hashes. A kernel that does not defer the one-under kind
    answers it wrongly, and the lists of 32 ties or fewer do not overflow, so the exact pass
    cannot repair it."""
    ones = np.uint32((1 << fsh) - 1)
    low = H & ones
    ok = (low != 0) & (low != ones)
    ties = []
    for l, c in enumerate(SPARSE_TIES):
        cand = l * LIST + np.flatnonzero(ok[l * LIST:(l + 1) * LIST])
        idx = pick(cand, c) if c else cand[:0]
        ties.append(H[idx].astype(np.int64) + np.array([0, -1, 1])[np.arange(c) % 3])
    ties = np.concatenate(ties)
    mids = pick(midpoints(np.sort(H)), M - len(ties))
    t = _sorted_u32(np.concatenate([ties, mids]))
    assert (np.diff(t.astype(np.int64)) > 0).all()
    return t


def middle_half(H):
    hs = np.sort(H)
    return hs[(hs >= (1 << 30)) & (hs < (3 << 30))]


def edge_tokens(H, nserv, thin):
    """Midpoints in [2^30, 3 * 2^30) (every thin-th), tokens 0 and 2^32 - 1, and three key hashes
    twice each; a multiple of nserv tokens."""
    hin = middle_half(H)
    dup = hin[[len(hin) // 4, len(hin) // 2, 3 * len(hin) // 4]]
    mids = midpoints(hin)[::thin]
    mids = mids[:len(mids) - (len(mids) + 8) % nserv]
    return _sorted_u32(np.concatenate([[0, 0xFFFFFFFF], dup, dup, mids])), dup


def bucket_tokens(H, M, sixteen=False):
    """cb = 13 (M in [8192, 16384)): N_DENSE buckets of DENSE_KINDS, every other bucket 0 or 1
    token. In every second dense bucket the tokens just above key hashes move onto them (keys
    on a token at every depth of a long bucket) where that keeps the placement. sixteen: dense
    bucket 300 holds 16 tokens."""
    assert 8192 <= M < 16384
    W = 1 << 19
    buckets = [13 * k for k in range(N_DENSE - 1)] + [8191]  # the first and the last bucket too
    hs = np.sort(H).astype(np.int64)
    toks, dense = [], []
    for k, b in enumerate(buckets):
        place, c = DENSE_KINDS[k % len(DENSE_KINDS)]
        if sixteen and k == 300:
            place, c = "even", 16
        base = b * W
        span, start = (W, base) if place == "even" else (W // 16, base if place == "low" else base + W - W // 16)
        t = start + ((2 * np.arange(c) + 1) * span) // (2 * c)
        if (k // len(DENSE_KINDS)) % 2:
            moved = np.zeros(c, dtype=bool)
            for h in hs[np.searchsorted(hs, start):np.searchsorted(hs, start + span)]:
                j = int(np.searchsorted(t, h, "left"))
                if j < c and not moved[j] and t[j] - h < span // (2 * c):  # stays in its c-th of the span
                    t[j], moved[j] = h, True
        assert (np.diff(t) > 0).all() and t[0] >= start and t[-1] < start + span
        toks.append(t)
        dense.append((b, place, c))
    ndense = sum(len(t) for t in toks)
    rest = np.setdiff1d(np.arange(8192), buckets)
    single = pick(rest, M - ndense).astype(np.int64)
    toks.append(single * W + (single * 2654435761) % W)
    return _sorted_u32(np.concatenate(toks)), dense


def build_cases(H):
    """Every case, by name, from the NKEYS host hashes."""
    assert len(H) == NKEYS and len(np.unique(H)) == NKEYS
    at = at_tokens(H)
    cases = [
        Case("at-exact", rows_rr(at, 3), "exact"),
        Case("at-exact-runs", rows_runs(at[:25340], 7), "exact"),
        Case("at-fp", rows_rr(at[:25000], 1000), "fp"),
        Case("at-fp-sparse", rows_rr(sparse_tokens(H, 25000), 1000), "fp", ties_per_list=SPARSE_TIES),
    ]
    q = midpoints(middle_half(H))
    cases.append(Case("ends-quarter", rows_rr(q[:len(q) - len(q) % 3], 3), "exact"))
    m = midpoints(np.sort(H))
    cases.append(Case("ends-sliver", rows_rr(m[126:126 + 25100], 1004), "fp"))
    for name, thin in (("edge-values", 1), ("edge-values-pad", 8)):
        t, dup = edge_tokens(H, 4, thin)
        c = Case(name, rows_rr(t, 4), "exact")
        c.dup = dup
        cases.append(c)
    t, dense = bucket_tokens(H, 10500)
    cases.append(Case("buckets", rows_rr(t, 3), "exact", dense=dense))
    cases.append(Case("buckets-runs", rows_runs(t, 7), "exact", dense=dense))
    t, dense = bucket_tokens(H, 11000)
    cases.append(Case("buckets-fp", rows_rr(t, 1000), "fp", dense=dense))
    t, dense = bucket_tokens(H, 10500, sixteen=True)
    cases.append(Case("buckets-16", rows_rr(t, 3), "exact", compact=False, dense=dense))
    return {c.name: c for c in cases}


CASE_NAMES = ["at-exact", "at-exact-runs", "at-fp", "at-fp-sparse", "ends-quarter", "ends-sliver", "edge-values",
              "edge-values-pad", "buckets", "buckets-runs", "buckets-fp", "buckets-16"]

# The wide variants: three token sets on 1,000 servers whose ids follow id_base filler names, so
# that N = id_base + 1000 names are interned: the last count with 14-bit ids (the LDS index may be
# built), the first with 15, the first with 16, the last
# with 16 (the highest id is all ones in the owner field) and the first with 17 (no compact layout,
# no direct table of the service, the packed layout at B = 17). More than 2^24 names (no packed
# layout either) would take 16 M interned strings: out of a test's reach.
WIDE_N = [16384, 16385, 32769, 65536, 65537]
WIDE_SETS = ["at-fp-sparse", "edge-values", "buckets-fp"]
WIDE_SERVERS = 1000
WIDE_CASE_NAMES = ["%s@%d" % (s, n) for s in WIDE_SETS for n in WIDE_N]
# the most names with which the lookup service builds its direct table (it keeps id 0xFFFF free)
SERVICE_TABLE_CASE = "edge-values@65534"


def filler_tokens(first, count, R, avoid=None):
    """R caller tokens for each of the fillers first .. first + count - 1, all distinct (an odd
    multiplier permutes the 32-bit values) and none of them in `avoid`."""
    spare = 0 if avoid is None else len(avoid)
    t = ((np.arange(first * R, (first + count) * R + spare, dtype=np.uint64) * np.uint64(2654435761)) &
         np.uint64(0xFFFFFFFF)).astype(np.uint32)
    if avoid is not None:
        t = t[~np.isin(t, avoid)]
    return np.ascontiguousarray(t[:count * R])


def build_wide_cases(H):
    """The wide variants, by name. The ids change neither M nor the tokens of edge-values and
    buckets-fp; at-fp-sparse designs its ties for the variant's fsh."""
    te, dup = edge_tokens(H, WIDE_SERVERS, 1)
    tb, dense = bucket_tokens(H, 11000)
    out = {}
    for n in WIDE_N + [int(SERVICE_TABLE_CASE.split("@")[1])]:
        kw = dict(compact=n <= 65536, id_base=n - WIDE_SERVERS)
        fsh = compact_params(25000, n)[2]
        sparse = Case("at-fp-sparse@%d" % n, rows_rr(sparse_tokens(H, 25000, fsh), WIDE_SERVERS), "fp",
                      ties_per_list=SPARSE_TIES, **kw)
        assert sparse.fsh == fsh
        edge = Case("edge-values@%d" % n, rows_rr(te, WIDE_SERVERS), "fp", **kw)
        edge.dup = dup
        buckets = Case("buckets-fp@%d" % n, rows_rr(tb, WIDE_SERVERS), "fp", dense=dense, **kw)
        for c in (sparse, edge, buckets):
            out[c.name] = c
    return {name: out[name] for name in WIDE_CASE_NAMES + [SERVICE_TABLE_CASE]}


_CACHE = {}


def keys_and_hashes(orc):
    """(keys [NKEYS, 36] uint8, host hashes [NKEYS] uint32), made once."""
    if "keys" not in _CACHE:
        u = orc.uuid_keys(42, 0, NKEYS)
        _CACHE["keys"] = (u, np.array([orc.hash32(bytes(k)) for k in u], dtype=np.uint32))
    return _CACHE["keys"]


def cases(orc):
    if "cases" not in _CACHE:
        H = keys_and_hashes(orc)[1]
        _CACHE["cases"] = {**build_cases(H), **build_wide_cases(H)}
        assert list(_CACHE["cases"]) == CASE_NAMES + WIDE_CASE_NAMES + [SERVICE_TABLE_CASE]
    return _CACHE["cases"]


def build_oracle(orc, case):
    """A new oracle ring of a case: the fillers added and removed in one call (their names stay
    interned, the ring is empty again), then the servers."""
    ring = orc.Ring(case.R)
    if case.id_base:
        fill, ft = case.filler_names(), case.filler_tokens()
        assert ring.add_remove(fill, fill, ft, ft)
        assert ring.token_count() == 0 and ring.server_count() == 0
    assert ring.add_remove(case.servers, [], case.add_tokens(), None)
    return ring


def oracle_ring(orc, case):
    """The oracle ring of a case, built once."""
    key = ("oracle", case.name)
    if key not in _CACHE:
        _CACHE[key] = build_oracle(orc, case)
    return _CACHE[key]


def oracle_rows(orc, case, nrep):
    """(owners, counts) of the oracle's lookupN(key, nrep) of every key, computed once."""
    key = ("rows", case.name, nrep)
    if key not in _CACHE:
        own, cnt = oracle_ring(orc, case).lookupn_keys(keys_and_hashes(orc)[0], nrep, threads=8)
        own.setflags(write=False)
        cnt.setflags(write=False)
        _CACHE[key] = (own, cnt)
    return _CACHE[key]
