"""GPU tests of the hash ring over servers whose names run from 1 byte to 262 bytes and hold bytes
past 0x7F (tests/name_cases.py): the replica strings name + str(i) then fall into every farmhash
length class and straddle every word of its 20-byte chunk loop, and the checksum string copies
names longer than 64 bytes.

References: pyoracle.hash32 over Python strings for the tokens and the checksum, the oracle ring
for the lookups. Exact comparisons."""
import random

import numpy as np
import pytest

import name_cases as nc

pytestmark = pytest.mark.gpu

R = 100


def _servers():
    return nc.ring_servers()


def _keys():
    rng = random.Random(77)
    keys = ["".join(rng.choice("abcdef0123456789:-./") for _ in range(rng.randint(1, 60))) for _ in range(1900)]
    return keys + [s + "0" for s in _servers()[::3]][:100]  # and keys that sit on a token


def _check(gpu, orc, ring, oracle, held, keys):
    held = sorted(held, key=nc.b)
    # tokens and owners: the sorted (hash32(name + str(i)), name); a token shared by two servers
    # (none here) would make the order of its owners a matter of the ring's tie rule
    pts = sorted((orc.hash32(nc.b(s) + str(i).encode()), nc.b(s)) for s in held for i in range(R))
    assert len({t for t, _ in pts}) == len(pts)
    tok, own = ring.dump()
    assert tok.tolist() == [t for t, _ in pts]
    assert [nc.b(ring.name(x)) for x in own] == [s for _, s in pts]
    want = b";".join(nc.b(s) for s in held)
    assert ring.checksum_string().encode() == want
    assert ring.checksum == orc.hash32(want) == oracle.checksum
    assert ring.getServerCount() == len(held) == oracle.server_count()
    hs = [orc.hash32(k) for k in keys]
    got = ring.lookup_ids(keys)
    assert [ring.name(x) for x in got] == [oracle.name(oracle.lookup_hash(h)) for h in hs]
    g, gc = ring.lookupn_ids(keys, 3)
    for k, (row, c) in enumerate(zip(g, gc)):
        assert [ring.name(x) for x in row[:c]] == [oracle.name(x) for x in oracle.lookupn_hash(hs[k], 3)], keys[k]
    for k in keys[:5] + keys[-5:]:  # the one-key forms
        assert ring.lookup(k) == oracle.name(oracle.lookup_hash(orc.hash32(k)))
        assert ring.lookupN(k, 3) == [oracle.name(x) for x in oracle.lookupn_hash(orc.hash32(k), 3)]


def test_ring_of_short_long_and_high_names(gpu, orc):
    servers = _servers()
    rng = random.Random(5)
    rng.shuffle(servers)
    keys = _keys()
    ring = gpu.HashRing()
    oracle = orc.Ring(R)
    assert ring.addRemoveServers(servers, None) == oracle.add_remove(servers, None)
    _check(gpu, orc, ring, oracle, servers, keys)
    gone = servers[::2]
    back = gone[::3]
    assert ring.addRemoveServers(None, gone) == oracle.add_remove(None, gone)
    _check(gpu, orc, ring, oracle, [s for s in servers if s not in set(gone)], keys)
    assert ring.addRemoveServers(back, None) == oracle.add_remove(back, None)
    _check(gpu, orc, ring, oracle, [s for s in servers if s not in set(gone) or s in set(back)], keys)
    ring.close()
