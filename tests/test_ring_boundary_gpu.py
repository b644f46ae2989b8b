"""GPU parity tests of the batch lookups on the boundary rings (tests/ring_boundary_cases.py): caller
tokens placed on, one under and one over the hashes of the device keys, at the ring's ends, at 0
and 2^32 - 1, and in buckets of 6..16 tokens, so that every fixed-36 kernel meets the 32-bit
boundaries its per-key code branches on with thousands of keys instead of by luck.

Every comparison is bit for bit against the CPU oracle (pyoracle.Ring over the same token rows),
which tests/test_ring_boundary_cases.py pins against a numpy walk on every key. Under
RP_LOOKUP_DEBUG=1 the default and the lean kernel also have to report the deferred keys and the
overflowed lists that the tokens and hashes alone predict (lower bounds: other causes of deferral
exist, so nothing is bounded from above).

A list of 2,048 keys with more than 32 deferred keys is redone whole by the exact pass, which
repairs whatever the fast path wrote for its keys. So each case whose own key order overflows
lists by design is also run in its thin order (Case.thin_order): eight lists with 16 such keys
each, where a wrong fast-path row stays wrong.

Measured on an MI355X, default kernel (the lean one within +-0.3 %), of 24,576 keys in 12 lists:
deferred (bound) / overflowed lists (bound); then the same in the thin order.
    at-exact          16 (1) / 0 (0)
    at-exact-runs     21,564 (12) / 12 (0)
    at-fp             23,608 (23,606) / 12 (12)
    at-fp-sparse      339 (323) / 6 (5); thin 340 / 4
    ends-quarter      6,212 (6,185) / 12 (12); thin 6,392 / 4
    ends-sliver       142 (124) / 0 (0)
    edge-values       6,212 (0) / 12 (0); thin 6,392 / 4
    edge-values-pad   6,349 (0) / 12 (0); thin 6,532 / 4
    buckets           689 (0) / 12 (0); thin 701 / 5
    buckets-runs      21,607 (0) / 12 (0); thin 21,621 / 12
    buckets-fp        843 (223) / 12 (0); thin 865 / 4
    buckets-16        no compact layout (a bucket of 16 tokens): the packed window kernel
With `e[j] < K` made `e[j] <= K` in LkStages::resolve, 8,157 rows of at-exact differ (all of them
keys on a token of server 0) under the sorted, lean and wave-specialised kernels, and 33 of
buckets in its thin order (none in its own: every list is redone). With `tie && !cv.exact` made
`false` there, at-fp fails at lookupN(1) (its lookupN(3) lists all overflow and are redone) and 97
rows of at-fp-sparse differ at lookupN(3), the keys with a token one under their hash.

The wide variants (<case>@N: the same token sets on 1,000 servers whose ids follow N - 1,000
interned filler names) take the owner field through 14, 15, 16 and 17 bits. A ring's name table
only grows, so a long-lived ring gets there; more than 2^24 names (no packed layout either, the
wide kernels alone) would take 16 M interned strings and is not tested. The LDS-index kernel is
not the default (kLdsDefault is false), so which kernel answered is asserted for RP_LOOKUP_LDS=1
as well: its own census line at N = 16,384 and the compact line (the default sorted kernel) from
16,385 on; for the default and the lean kernel the compact line up to 65,536; no line at 65,537.
Measured as above (default kernel; the lean one gave the same counts), N = 16384 / 16385 /
32769 and 65536 (ob 16 both, the same figures):
    at-fp-sparse@N    408 / 485 / 640 (323) / 8, 8, 9 (5); thin 408 / 488 / 644 / 4
    edge-values@N     6,866 / 6,941 / 7,072 (3) / 12 (0); thin 7,064 / 7,136 / 7,272 / 4
    buckets-fp@N      864 / 891 / 933 (223) / 12 (0); thin 886 / 912 / 958 / 4
    RP_LOOKUP_LDS=1 at 16384, of 25,088 keys in 49 wave-tiles: at-fp-sparse 508 / 0,
    edge-values 7,681 / 49, buckets-fp 21,976 / 49
    @65537            no compact layout (ids past 16 bits): the packed window kernel at B = 17
With omask made the constant 0x3FFF in LkStages (the sorted and the lean kernel), all 54 tests of
N = 16385, 32769, 65536 x {default, lds, sort512, sort1024, sort0, ws} fail (ws in its lookup and
lookupN(1, 2, 4), which the lean kernel serves; its own lookupN(3) kernel keeps its mask), and so
do the wide snapshot test's load and the life cycle at its first step (10-bit ids: the mask is
too wide there). Rows that differ, lookupN(1) / lookupN(3), own order then thin order:
    at-fp-sparse@16385 22 / 31, thin 18 / 51; @32769 and @65536 19,026 / 6,057, thin 19,328 / 16,256
    edge-values@16385 0 / 0, thin 9 / 30; @32769 and @65536 0 / 0, thin 16,256 / 16,252
    buckets-fp@16385 4 / 0, thin 12 / 28; @32769 and @65536 7,960 / 0, thin 19,328 / 16,175
(at 16385 only ids 16384 is cut; in their own order every list of edge-values and buckets-fp
overflows and is redone whole: the thin orders catch it). At N = 16384 the mutant is the kernel.
With `ob <= 14` dropped from lds_pending nothing changes, ring_build_lds checks the width again;
with both checks dropped the LDS-index kernel answers at ob 15 and 16 and answers every row
correctly (fingerprints of 9 and 8 bits: 684 and 1,027 deferred keys of at-fp-sparse), so only the
census assertion of the nine `lds` tests at N = 16385, 32769, 65536 fails.
"""
import ctypes
import re

import numpy as np
import pytest

import ring_boundary_cases as rb
from test_group_gpu import ref_group_by
from test_ring_gpu import LAYOUTS, set_layout
from test_ring_load_gpu import load_dev, want_load
from test_ring_moved_gpu import assert_moved, moved_dev
from test_ring_sorted_gpu import key_counts, lookupn, sort_env

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

# kernel id -> (RP_LOOKUP_SORT or None: unset, layout of test_ring_gpu.LAYOUTS)
KERNELS = {"default": (None, "compact"), "sort512": (512, "compact"), "sort1024": (1024, "compact"),
           "sort0": (0, "compact")}
KERNELS.update({name: (None, name) for name in ("lds", "ws", "ws-4-12", "round1", "hint0", "wpred0", "fusefix", "stg2",
                                                "quarter-kpl8-grid3", "window", "packed", "wide")})
assert all(layout in LAYOUTS for _, layout in KERNELS.values())
WIDE_KERNELS = ["default", "lds", "sort512", "sort1024", "sort0", "ws", "round1", "window", "packed", "wide"]
assert all(k in KERNELS for k in WIDE_KERNELS)
NREPS = (-1, 0, 1, 2, 3, 4)
CONSUMER_CASES = ["at-exact", "at-fp", "edge-values", "at-fp-sparse@65536", "at-fp-sparse@65537"]
SERVICE_CASES = ["edge-values@65534", "edge-values@65536", "edge-values@65537"]
DEBUG_LINE = re.compile(r"compact lookupN: (\d+) keys, (\d+) deferred, (\d+) overflowed tiles "
                        r"\(cb (\d+) ob (\d+) fsh (\d+) sort (\d+)\)")
LDS_LINE = re.compile(r"lds lookupN: (\d+) keys, (\d+) deferred, (\d+) overflowed tiles \(ng (\d+) fb (\d+) ob (\d+)\)")
LIFE_CYCLE_N = (16384, 16385, 65536, 65537)

_PAIRS = {}
_DKEYS = {}


def add_remove_tokens(gpu, ring, add, rem, add_tok, rem_tok):
    """rp_ring_add_remove with the caller tokens as arrays: HashRing.addRemoveServers would ask
    its hashFunc for each of the fillers' 1.6 M tokens, twice. The names in both lists leave the
    host's servers map as it was."""
    assert set(add) == set(rem) and len(add_tok) == len(add) * ring.replicaPoints == len(rem_tok)
    ab, ao = gpu._pack(add)
    rmb, ro = gpu._pack(rem)
    changed = ctypes.c_int()
    gpu.check(gpu.lib().rp_ring_add_remove(ring._h, ab, ao.ctypes.data, len(add), add_tok.ctypes.data, rmb,
                                           ro.ctypes.data, len(rem), rem_tok.ctypes.data, ctypes.byref(changed)))
    return bool(changed.value)


def device_ring(gpu, orc, case):
    """A device ring of the case's rows (the dict-backed hashFunc), checked against the oracle's:
    checksum, dump, and the interned ids (id_base + the row numbers on both sides). The fillers of
    a wide case go in and out in one call first, as on the oracle."""
    oracle = rb.oracle_ring(orc, case)
    ring = gpu.HashRing({"replicaPoints": case.R, "hashFunc": case.hash_func(orc.hash32)})
    if case.id_base:
        fill, ft = case.filler_names(), case.filler_tokens()
        assert add_remove_tokens(gpu, ring, fill, fill, ft, ft)
        assert ring.size == 0 and ring.getServerCount() == 0 and ring.id_bound() == case.id_base
    assert ring.addRemoveServers(case.servers)
    assert ring.checksum == oracle.checksum
    assert ring.size == case.M
    t, o = ring.dump()
    ot, oo = oracle.dump()
    assert np.array_equal(t, ot) and np.array_equal(o, oo)
    assert [ring.server_id(s) for s in case.servers] == list(range(case.id_base, case.N))
    assert ring.id_bound() == case.N
    return ring


def pair(gpu, orc, name):
    if name not in _PAIRS:
        case = rb.cases(orc)[name]
        _PAIRS[name] = (case, device_ring(gpu, orc, case))
    return _PAIRS[name]


def device_keys(orc, name="keys", order=None):
    """The keys on the device, in their own order or (cached by case name) in `order`."""
    if name not in _DKEYS:
        keys = rb.keys_and_hashes(orc)[0]
        _DKEYS[name] = torch.from_numpy(keys if order is None else np.ascontiguousarray(keys[order])).cuda()
    return _DKEYS[name]


@pytest.mark.parametrize("kernel", list(KERNELS))
@pytest.mark.parametrize("name", rb.CASE_NAMES)
def test_lookups_vs_oracle(gpu, orc, name, kernel, monkeypatch, capfd):
    check_lookups(gpu, orc, name, kernel, monkeypatch, capfd)


@pytest.mark.parametrize("kernel", WIDE_KERNELS)
@pytest.mark.parametrize("name", rb.WIDE_CASE_NAMES)
def test_wide_id_lookups_vs_oracle(gpu, orc, name, kernel, monkeypatch, capfd):
    """The same on the wide variants: ids of 14 bits (the last count at which the LDS index is
    built), 15 and 16 (the sorted, lean and wave-specialised kernels serve RP_LOOKUP_LDS=1 too;
    fingerprints of 9 and 8 bits) and 17 (no compact layout: the packed probe at B = 17)."""
    check_lookups(gpu, orc, name, kernel, monkeypatch, capfd)


def check_lookups(gpu, orc, name, kernel, monkeypatch, capfd):
    case, ring = pair(gpu, orc, name)
    sort, layout = KERNELS[kernel]
    set_layout(monkeypatch, layout)
    monkeypatch.delenv("RP_LOOKUP_SORT", raising=False)
    monkeypatch.delenv("RP_LOOKUP_DEBUG", raising=False)
    env = {} if sort is None else {"RP_LOOKUP_SORT": sort}
    sorted_t = {None: 256}.get(sort, sort) if layout == "compact" else 0
    d_keys = device_keys(orc)
    # the sorted shapes: their tile edges, and every key; elsewhere every key (a partial last tile
    # goes to the generic kernel)
    counts_n = sorted(set(key_counts(sorted_t) + [rb.NKEYS])) if sorted_t else [rb.NKEYS]
    assert max(counts_n) == rb.NKEYS
    with sort_env(**env):
        for n in counts_n:
            for nrep in NREPS:
                want, wcnt = rb.oracle_rows(orc, case, nrep)
                for with_counts in (True, False):
                    got, gcnt = lookupn(ring, d_keys, n, nrep=nrep, counts=with_counts)
                    assert np.array_equal(got, want[:n]), (n, nrep, with_counts)
                    if with_counts:
                        assert np.array_equal(gcnt, wcnt[:n]), (n, nrep)
        d_l = torch.full((rb.NKEYS,), -2, dtype=torch.int32, device="cuda")
        ring.lookup_dev(d_keys.data_ptr(), rb.NKEYS, d_l.data_ptr())
        torch.cuda.synchronize()
        assert np.array_equal(d_l.cpu().numpy().view(np.uint32), rb.oracle_rows(orc, case, 1)[0][:, 0])
        # the thin key order: lists that the exact pass does not redo whole, so a wrong fast-path
        # row stays wrong
        order = case.thin_order(rb.keys_and_hashes(orc)[1])
        if order is not None:
            d_thin = device_keys(orc, name, order)
            for nrep in NREPS:
                want, wcnt = rb.oracle_rows(orc, case, nrep)
                got, gcnt = lookupn(ring, d_thin, rb.NKEYS, nrep=nrep)
                assert np.array_equal(got, want[order]), ("thin", nrep)
                assert np.array_equal(gcnt, wcnt[order]), ("thin", nrep)
    if kernel not in ("default", "sort0") and not (kernel == "lds" and case.id_base):
        return
    # which kernel ran, and what it deferred
    capfd.readouterr()
    with sort_env(RP_LOOKUP_DEBUG=1, **env):
        got, gcnt = lookupn(ring, d_keys, rb.NKEYS)
    err = capfd.readouterr().err
    m, lds = DEBUG_LINE.search(err), LDS_LINE.search(err)
    want, wcnt = rb.oracle_rows(orc, case, 3)
    assert np.array_equal(got, want) and np.array_equal(gcnt, wcnt)
    if kernel == "lds" and case.ob <= 14:
        # the LDS-index kernel answers where it is asked for (RP_LOOKUP_LDS=1) and ids fit 14 bits
        assert lds and m is None, err
        done, deferred, over, ng, fb, ob = (int(x) for x in lds.groups())
        with capfd.disabled():
            print("\nboundary %s lds: %d keys, deferred %d, overflowed wave-tiles %d (ng %d)" % (name, done, deferred, over, ng))
        assert (done, fb, ob) == (rb.NKEYS // 512 * 512, 24 - case.ob, case.ob)
        return
    assert lds is None, err  # ... and nowhere else: past 14 bits the compact layout's own kernels answer
    if not case.compact:
        assert m is None  # a bucket of 16 tokens, or ids past 16 bits: the compact layout is not built
        return
    assert m, "no RP_LOOKUP_DEBUG line"
    done, deferred, over, cb, ob, fsh, ran = (int(x) for x in m.groups())
    nlists = rb.NKEYS // rb.LIST
    low, over_low = case.deferred_lower_bound(rb.keys_and_hashes(orc)[1], nlists * rb.LIST)
    with capfd.disabled():  # the figures, before anything is asserted of them
        print("\nboundary %s %s: %d keys, deferred %d (at least %d), overflowed lists %d of %d (at least %d)"
              % (name, kernel, done, deferred, low, over, nlists, over_low))
    assert ran == (256 if kernel == "lds" else sorted_t)  # (lds: it fell through to the default kernel)
    assert (cb, ob, fsh) == (case.cb, case.ob, case.fsh)
    assert done == nlists * rb.LIST  # the tiles took every whole list
    assert deferred >= low
    assert over >= over_low
    if name == "at-fp":
        assert over == nlists  # every list overflowed: its tile's slots redo all its keys
    if name.split("@")[0] == "at-fp-sparse":
        assert over >= sum(t > rb.SLOTS for t in rb.SPARSE_TIES) > 0
        assert deferred > 0 and over < nlists  # ... and a list that did not: the per-key redo ran too
    if order is not None:  # the figures of the thin order (nothing is asserted of them)
        capfd.readouterr()
        with sort_env(RP_LOOKUP_DEBUG=1, **env):
            lookupn(ring, d_thin, rb.NKEYS)
        m = DEBUG_LINE.search(capfd.readouterr().err)
        with capfd.disabled():
            print("boundary %s %s thin order: deferred %s, overflowed lists %s of %d" % (name, kernel, m.group(2), m.group(3), nlists))


@pytest.mark.parametrize("name", CONSUMER_CASES)
def test_snapshot_load_and_group_vs_oracle(gpu, orc, name):
    """The consumers with their own find / walk code: a snapshot's lookupN, the owner load, the
    keys grouped by owner."""
    case, ring = pair(gpu, orc, name)
    d_keys = device_keys(orc)
    n = rb.NKEYS
    snap = ring.snapshot()
    for nrep in (1, 3):
        want, wcnt = rb.oracle_rows(orc, case, nrep)
        got, gcnt = lookupn(snap, d_keys, n, nrep=nrep)
        assert np.array_equal(got, want) and np.array_equal(gcnt, wcnt), nrep
        assert ring.id_bound() == snap.id_bound() == case.N
        for h in (ring, snap):  # (a wide case: N counters, past the 20,480 LDS bins)
            load = load_dev(h, d_keys.data_ptr(), n, nrep, case.N)
            assert np.array_equal(load, want_load(want, case.N)), nrep
    snap.close()
    want = ref_group_by(rb.oracle_rows(orc, case, 1)[0][:, 0])
    dests = torch.full((n,), -2, dtype=torch.int32, device="cuda")
    goff = torch.full((n + 1,), -2, dtype=torch.int32, device="cuda")
    perm = torch.full((n,), -2, dtype=torch.int32, device="cuda")
    nd = torch.zeros(1, dtype=torch.int32, device="cuda")
    ring.group_dev(d_keys.data_ptr(), n, dests.data_ptr(), goff.data_ptr(), perm.data_ptr(), nd.data_ptr())
    torch.cuda.synchronize()
    k = int(nd.item())
    assert dests[:k].cpu().numpy().view(np.uint32).tolist() == list(want)
    g, p = goff[:k + 1].cpu().numpy(), perm.cpu().numpy()
    assert {d: p[g[i]:g[i + 1]].tolist() for i, d in enumerate(want)} == want


@pytest.mark.parametrize("name", CONSUMER_CASES)
def test_moved_keys_vs_oracle(gpu, orc, name):
    """A snapshot, then the server with the most tokens on key hashes leaves: the moved keys are
    exactly those whose oracle rows differ between the two oracle rings."""
    case = rb.cases(orc)[name]
    keys, H = rb.keys_and_hashes(orc)
    gone = int(np.argmax(np.isin(case.rows, H).sum(axis=1)))
    ring = device_ring(gpu, orc, case)
    snap = ring.snapshot()
    assert ring.addRemoveServers(None, [case.servers[gone]])
    after = rb.build_oracle(orc, case)
    after.add_remove([], [case.servers[gone]], None, case.rows[gone])
    assert ring.checksum == after.checksum
    t, o = ring.dump()
    at, ao = after.dump()
    assert np.array_equal(t, at) and np.array_equal(o, ao)
    d_keys = device_keys(orc)
    for nrep in (1, 3):
        wb = rb.oracle_rows(orc, case, nrep)[0]
        wa = after.lookupn_keys(keys, nrep, threads=8)[0]
        cnt, idx, br, ar = moved_dev(ring, snap, d_keys.data_ptr(), rb.NKEYS, nrep, rb.NKEYS, rb.NKEYS)
        assert cnt == assert_moved((idx[:cnt], br[:cnt], ar[:cnt]), wb, wa, rb.NKEYS) > 0
    snap.close()
    ring.close()


@pytest.mark.parametrize("name", SERVICE_CASES)
def test_wide_id_service_vs_oracle(gpu, orc, name):
    """The resident lookup service at its id limits: 65,534 names (the most with which it builds
    its direct table, which keeps id 0xFFFF free), 65,536 (no table; the compact window, and the
    owner 65,535 of token 2^32 - 1) and 65,537 (no table and no compact layout). 300 one-hash
    lookupN(1..8) and lookup calls: key hashes, tokens, tokens - 1 and + 1, 0 and 2^32 - 1."""
    case, ring = pair(gpu, orc, name)
    oracle = rb.oracle_ring(orc, case)
    H = rb.keys_and_hashes(orc)[1]
    T, _ = case.sorted_ring()
    tok = np.concatenate([rb.pick(T, 50), T[-2:]]).astype(np.int64)
    hs = np.concatenate([[0, 0xFFFFFFFF], tok, (tok - 1) & 0xFFFFFFFF, (tok + 1) & 0xFFFFFFFF])
    hs = np.concatenate([hs, rb.pick(np.sort(H), 300 - len(hs))]).astype(np.uint32)
    assert len(hs) == 300
    ring.service(200)
    try:
        last = 0
        for i, h in enumerate(hs.tolist()):
            n = 1 + i % 8
            g, gc = ring.lookupn_hashes([h], n)
            want = oracle.lookupn_hash(h, n)
            assert g[0][:gc[0]].tolist() == want and len(want) == n, (i, h, n)
            assert ring.lookup_hashes([h]).tolist() == [oracle.lookup_hash(h)], (i, h)
            last += want[0] == case.N - 1
        # the highest id answered: every hash above the inner tokens is its own (2^32 - 1, the two
        # hashes just under it, the one over the last inner token, and over a fifth of the key hashes)
        assert last >= 4 + (300 - 2 - 3 * len(tok)) // 5
    finally:
        ring.service(0)
    # the service off: the host forms' staged batch and their small batch (at most 64 keys)
    for batch in (hs, hs[:7], hs[-64:]):
        g, gc = ring.lookupn_hashes(batch, 3)
        assert g.tolist() == [oracle.lookupn_hash(h, 3) for h in batch.tolist()] and (gc == 3).all()


def test_id_width_life_cycle(gpu, orc, monkeypatch):
    """One ring through every id width: 1,000 live servers x 25 caller tokens (at-fp-sparse), and
    filler batches (each added and removed in one call) that take the interned names to 16,384,
    16,385, 65,536 and 65,537. After each batch, and again after the live set was removed and
    re-added, the ring is the live set's under ids 0..999: checksum, dump, lookupN(-1, 1, 3, 4)
    and lookup of every key on the default path. Nothing built for a narrower id width may
    survive a rebuild: the LDS index, the hinted index, the service's table, the packed B."""
    set_layout(monkeypatch, "compact")
    monkeypatch.delenv("RP_LOOKUP_SORT", raising=False)
    monkeypatch.delenv("RP_LOOKUP_DEBUG", raising=False)
    live = rb.cases(orc)["at-fp-sparse"]
    keys = rb.keys_and_hashes(orc)[0]
    d_keys = device_keys(orc)
    ring = gpu.HashRing({"replicaPoints": live.R, "hashFunc": live.hash_func(orc.hash32)})
    oracle = orc.Ring(live.R)
    T, O = live.sorted_ring()

    def check(step):
        assert ring.checksum == oracle.checksum, step
        assert ring.size == oracle.token_count() == live.M, step
        t, o = ring.dump()
        ot, oo = oracle.dump()
        assert np.array_equal(t, ot) and np.array_equal(o, oo), step
        assert np.array_equal(t, T) and np.array_equal(o, O), step
        for nrep in (-1, 1, 3, 4):
            want, wcnt = oracle.lookupn_keys(keys, nrep, threads=8)
            got, gcnt = lookupn(ring, d_keys, rb.NKEYS, nrep=nrep)
            assert np.array_equal(got, want) and np.array_equal(gcnt, wcnt), (step, nrep)
        d_l = torch.full((rb.NKEYS,), -2, dtype=torch.int32, device="cuda")
        ring.lookup_dev(d_keys.data_ptr(), rb.NKEYS, d_l.data_ptr())
        torch.cuda.synchronize()
        assert np.array_equal(d_l.cpu().numpy().view(np.uint32), oracle.lookup_keys(keys)), step

    assert ring.addRemoveServers(live.servers) and oracle.add_remove(live.servers, [], live.add_tokens(), None)
    names = live.nserv
    check(names)
    for target in LIFE_CYCLE_N:
        first, count = names - live.nserv, target - names
        fill = ["fill-%d:1" % i for i in range(first, first + count)]
        ft = rb.filler_tokens(first, count, live.R, avoid=live.add_tokens())  # the live tokens stay
        assert len(np.unique(ft)) == count * live.R
        assert add_remove_tokens(gpu, ring, fill, fill, ft, ft) and oracle.add_remove(fill, fill, ft, ft)
        names = target
        assert ring.id_bound() == names
        check((names, "fillers"))
        assert ring.addRemoveServers(None, live.servers) and oracle.add_remove([], live.servers, None, live.add_tokens())
        assert ring.size == 0 and oracle.token_count() == 0
        assert ring.addRemoveServers(live.servers) and oracle.add_remove(live.servers, [], live.add_tokens(), None)
        assert ring.id_bound() == names and [ring.server_id(s) for s in live.servers[::333]] == [0, 333, 666, 999]
        check((names, "re-added"))
    ring.close()
