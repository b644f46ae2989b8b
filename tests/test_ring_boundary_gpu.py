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
"""
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
NREPS = (-1, 0, 1, 2, 3, 4)
CONSUMER_CASES = ["at-exact", "at-fp", "edge-values"]
DEBUG_LINE = re.compile(r"compact lookupN: (\d+) keys, (\d+) deferred, (\d+) overflowed tiles "
                        r"\(cb (\d+) ob (\d+) fsh (\d+) sort (\d+)\)")

_PAIRS = {}
_DKEYS = {}


def device_ring(gpu, orc, case):
    """A device ring of the case's rows (the dict-backed hashFunc), checked against the oracle's:
    checksum, dump, and the interned ids (the row numbers on both sides)."""
    oracle = rb.oracle_ring(orc, case)
    ring = gpu.HashRing({"replicaPoints": case.R, "hashFunc": case.hash_func(orc.hash32)})
    assert ring.addRemoveServers(case.servers)
    assert ring.checksum == oracle.checksum
    assert ring.size == case.M
    t, o = ring.dump()
    ot, oo = oracle.dump()
    assert np.array_equal(t, ot) and np.array_equal(o, oo)
    assert [ring.server_id(s) for s in case.servers] == list(range(case.nserv))
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
    if kernel not in ("default", "sort0"):
        return
    # which kernel ran, and what it deferred
    capfd.readouterr()
    with sort_env(RP_LOOKUP_DEBUG=1, **env):
        got, gcnt = lookupn(ring, d_keys, rb.NKEYS)
    m = DEBUG_LINE.search(capfd.readouterr().err)
    want, wcnt = rb.oracle_rows(orc, case, 3)
    assert np.array_equal(got, want) and np.array_equal(gcnt, wcnt)
    if not case.compact:
        assert m is None  # a bucket of 16 tokens: the compact layout is not built
        return
    assert m, "no RP_LOOKUP_DEBUG line"
    done, deferred, over, cb, ob, fsh, ran = (int(x) for x in m.groups())
    nlists = rb.NKEYS // rb.LIST
    low, over_low = case.deferred_lower_bound(rb.keys_and_hashes(orc)[1], nlists * rb.LIST)
    with capfd.disabled():  # the figures, before anything is asserted of them
        print("\nboundary %s %s: %d keys, deferred %d (at least %d), overflowed lists %d of %d (at least %d)"
              % (name, kernel, done, deferred, low, over, nlists, over_low))
    assert ran == sorted_t
    assert (cb, ob, fsh) == (case.cb, case.ob, case.fsh)
    assert done == nlists * rb.LIST  # the tiles took every whole list
    assert deferred >= low
    assert over >= over_low
    if name == "at-fp":
        assert over == nlists  # every list overflowed: its tile's slots redo all its keys
    if name == "at-fp-sparse":
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
        assert ring.id_bound() == case.nserv
        for h in (ring, snap):
            load = load_dev(h, d_keys.data_ptr(), n, nrep, case.nserv)
            assert np.array_equal(load, want_load(want, case.nserv)), nrep
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
    after = orc.Ring(case.R)
    after.add_remove(case.servers, [], case.add_tokens(), None)
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
