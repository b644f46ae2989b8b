"""GPU parity tests of the sorted-tile lookupN(3) kernel (k_lookupn_sorted, RP_LOOKUP_SORT = 256 |
512 | 1024 threads; rp_ring.hip).

The kernel orders each tile of 8 x threads keys by hash before the index and window trips and
addresses rows by the key's tile slot, so the owners, the counts and the deferred set must not
depend on the order. Every comparison is bit for bit, against the CPU oracle
(pyoracle.Ring.lookupn_keys) and against the same call under RP_LOOKUP_SORT=0 (the lean kernel).
"""
import os
import re

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

SHAPES = [256, 512, 1024]
NMAX = 3 * 8 * 1024 + 777  # the longest key count of any shape
# (servers, replica points): 300 tokens (few bins used, long runs of equal bins); C1; runs of one
# owner and long buckets (the exact fallbacks, as test_ring_gpu's slow-path rings); 192 tokens
RINGS = {"3x100": (3, 100), "1000x100": (1000, 100), "3x700": (3, 700), "64x3": (64, 3)}
KEYSETS = ["uuid", "same", "asc", "desc"]


def key_counts(T):
    # one tile; a tile plus a remainder; three tiles and a tail; one short of a tile (falls back)
    return [8 * T, 8 * T + 1, 3 * 8 * T + 777, 8 * T - 1]


class sort_env:
    """RP_LOOKUP_SORT (and more) in the process environment around a call."""

    def __init__(self, **kv):
        self.kv = {k: str(v) for k, v in kv.items()}

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kv}
        os.environ.update(self.kv)

    def __exit__(self, *exc):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


_KEYS = {}


def keyset(orc, name):
    """(NMAX, 36) uint8 host keys of a key set, made once."""
    if not _KEYS:
        u = orc.uuid_keys(42, 0, NMAX)
        h = np.array([orc.hash32(bytes(k)) for k in u], dtype=np.uint32)  # host hashes
        order = np.argsort(h, kind="stable")
        _KEYS["uuid"] = u
        _KEYS["same"] = np.ascontiguousarray(np.broadcast_to(u[7], (NMAX, 36)))  # one bin holds the tile
        _KEYS["asc"] = np.ascontiguousarray(u[order])
        _KEYS["desc"] = np.ascontiguousarray(u[order[::-1]])
        assert (np.diff(h[order].astype(np.int64)) >= 0).all()
    return _KEYS[name]


_RINGS = {}


def ring_pair(gpu, orc, name):
    """(device ring, oracle ring, {key set: (owners, counts) of the oracle's lookupN(3)})."""
    if name not in _RINGS:
        nserv, R = (10000, 100) if name == "c2" else RINGS[name]
        servers = [orc.c2_addr(i + 17) for i in range(nserv)]
        ring, oracle = gpu.HashRing({"replicaPoints": R}), orc.Ring(R)
        ring.addRemoveServers(servers)
        oracle.add_remove(servers)
        assert ring.checksum == oracle.checksum
        _RINGS[name] = (ring, oracle, {})
    return _RINGS[name]


def want_for(orc, pair, ks):
    ring, oracle, cache = pair
    if ks not in cache:
        cache[ks] = oracle.lookupn_keys(keyset(orc, ks), 3, threads=8)
    return cache[ks]


def lookupn(ring, d_keys, n, nrep=3, counts=True):
    w = max(nrep, 1)
    d_o = torch.full((n * w,), -2, dtype=torch.int32, device="cuda")
    d_c = torch.full((n,), 77, dtype=torch.uint8, device="cuda") if counts else None
    ring.lookupn_dev(d_keys.data_ptr(), n, nrep, d_o.data_ptr(), d_c.data_ptr() if counts else None)
    torch.cuda.synchronize()
    return d_o.cpu().numpy().view(np.uint32).reshape(n, w), (d_c.cpu().numpy() if counts else None)


@pytest.mark.parametrize("ks", KEYSETS)
@pytest.mark.parametrize("ring_name", list(RINGS))
@pytest.mark.parametrize("T", SHAPES)
def test_sorted_tiles_vs_oracle_and_lean(gpu, orc, T, ring_name, ks):
    pair = ring_pair(gpu, orc, ring_name)
    ring = pair[0]
    want, wcnt = want_for(orc, pair, ks)
    d_keys = torch.from_numpy(keyset(orc, ks)).cuda()
    for n in key_counts(T):
        for counts in (True, False):
            with sort_env(RP_LOOKUP_SORT=T):
                got, gcnt = lookupn(ring, d_keys, n, counts=counts)
            with sort_env(RP_LOOKUP_SORT=0):
                lean, lcnt = lookupn(ring, d_keys, n, counts=counts)
            assert np.array_equal(got, want[:n]), (n, counts)
            assert np.array_equal(got, lean), (n, counts)
            if counts:
                assert np.array_equal(gcnt, wcnt[:n]), n
                assert np.array_equal(gcnt, lcnt), n


@pytest.mark.parametrize("T", SHAPES)
def test_sorted_tiles_c2_ring(gpu, orc, T, capfd):
    """The full 10k x 100 ring, 2^18 device-generated keys: owners, counts, and under
    RP_LOOKUP_DEBUG=1 the sorted kernel ran, deferred as many keys as the lean kernel and
    overflowed no list."""
    pair = ring_pair(gpu, orc, "c2")
    ring, oracle, cache = pair
    n = 1 << 18
    if "c2" not in cache:
        cache["c2"] = oracle.lookupn_keys(orc.uuid_keys(42, 0, n), 3, threads=8)
    want, wcnt = cache["c2"]
    d_keys = torch.empty(n * 36, dtype=torch.uint8, device="cuda")
    gpu.gen_uuid_keys_dev(42, 0, n, d_keys.data_ptr())
    line = re.compile(r"compact lookupN: (\d+) keys, (\d+) deferred, (\d+) overflowed tiles \(.* sort (\d+)\)")
    seen = {}
    for s in (T, 0):
        capfd.readouterr()
        with sort_env(RP_LOOKUP_SORT=s, RP_LOOKUP_DEBUG=1):
            got, gcnt = lookupn(ring, d_keys, n)
        m = line.search(capfd.readouterr().err)
        assert m, "no RP_LOOKUP_DEBUG line"
        seen[s] = tuple(int(x) for x in m.groups())
        assert np.array_equal(got, want), s
        assert np.array_equal(gcnt, wcnt), s
    assert seen[T][3] == T and seen[0][3] == 0  # which kernel took the tiles
    assert seen[T][0] == seen[0][0] == n
    assert seen[T][1] == seen[0][1] > 0  # the deferred set is the lean kernel's
    assert seen[T][2] == 0 and seen[0][2] == 0


@pytest.mark.parametrize("ring_name", list(RINGS))
def test_sorted_kernel_is_taken_on_every_ring(gpu, orc, ring_name, capfd):
    """The rings above do reach the sorted kernel (a ring without the hinted index would fall
    back to the lean kernel and the parity tests would compare it with itself)."""
    ring = ring_pair(gpu, orc, ring_name)[0]
    d_keys = torch.from_numpy(keyset(orc, "uuid")).cuda()
    capfd.readouterr()
    with sort_env(RP_LOOKUP_SORT=256, RP_LOOKUP_DEBUG=1):
        lookupn(ring, d_keys, 8 * 256)
    assert re.search(r"compact lookupN: 2048 keys, .* sort 256\)", capfd.readouterr().err)
    with sort_env(RP_LOOKUP_SORT=256, RP_LOOKUP_DEBUG=1):
        lookupn(ring, d_keys, 8 * 256 - 1)  # less than a tile: the lean kernel
    assert re.search(r"compact lookupN: 1024 keys, .* sort 0\)", capfd.readouterr().err)


@pytest.mark.parametrize("T", SHAPES)
def test_other_widths_do_not_take_the_sorted_path(gpu, orc, T):
    pair = ring_pair(gpu, orc, "1000x100")
    ring, oracle = pair[0], pair[1]
    keys = keyset(orc, "uuid")
    d_keys = torch.from_numpy(keys).cuda()
    n = 3 * 8 * T + 777
    for nrep in (1, 2, 4):
        want, wcnt = oracle.lookupn_keys(keys[:n], nrep)
        with sort_env(RP_LOOKUP_SORT=T):
            got, gcnt = lookupn(ring, d_keys, n, nrep=nrep)
        assert np.array_equal(got, want), nrep
        assert np.array_equal(gcnt, wcnt), nrep
