"""GPU parity tests of the ticketed form of the 256-thread sorted-tile lookupN(3) kernel
(k_lookupn_sorted_ticket, RP_LOOKUP_TICKET, RP_LOOKUP_STAGGER; rp_ring.hip).

The ticketed form runs the strided kernel's tiles on a grid of resident workgroups that draw
their tiles from a device counter. Rows, counts and the deferred lists are addressed by the tile
index, so nothing a caller sees may depend on which workgroup ran a tile, on the grid, or on the
start stagger. Every comparison is bit for bit: against the CPU oracle
(pyoracle.Ring.lookupn_keys) and against the same call under RP_LOOKUP_TICKET=0 (the strided
kernel), rows, counts and the deferred total of RP_LOOKUP_DEBUG=1. The outputs are prefilled, so a
tile nobody drew (a counter that was not put back after the launch before) fails the comparison.
"""
import os
import re

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

TILE = 2048
# one tile; tiles, then the lean kernel's and the generic kernel's remainder; more tiles than a
# forced grid of 1 or 3 draws in one round
KEY_COUNTS = [TILE, TILE * 5 + 77, TILE * 33]
NMAX = max(KEY_COUNTS)
# None: the launcher's own grid; 1 and 3: every workgroup draws many tickets; 64: more
# workgroups than any of the key counts has tiles (the surplus must write nothing)
GRIDS = [None, 1, 3, 64]
SERVERS, POINTS = 300, 100

LINE = re.compile(r"compact lookupN: (\d+) keys, (\d+) deferred, (\d+) overflowed tiles \(.* sort (\d+)\) "
                  r"ticket (\d+) grid (\d+) stagger (\d+)")


class env:
    """RP_LOOKUP_* in the process environment around a call; None removes the variable."""

    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kv}
        for k, v in self.kv.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = str(v)

    def __exit__(self, *exc):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


_STATE = {}


def state(gpu, orc):
    """(device ring, device keys, the oracle's (owners, counts) of lookupN(3)), made once."""
    if not _STATE:
        servers = [orc.c2_addr(i + 17) for i in range(SERVERS)]
        ring, oracle = gpu.HashRing({"replicaPoints": POINTS}), orc.Ring(POINTS)
        ring.addRemoveServers(servers)
        oracle.add_remove(servers)
        assert ring.checksum == oracle.checksum
        keys = orc.uuid_keys(42, 0, NMAX)
        _STATE["v"] = (ring, torch.from_numpy(keys).cuda(), oracle.lookupn_keys(keys, 3, threads=8))
    return _STATE["v"]


def launch(ring, d_keys, n, counts=True):
    """One lookupN(3) queued on the current stream, not waited for: (rows, counts) on the device."""
    d_o = torch.full((n * 3,), -2, dtype=torch.int32, device="cuda")
    d_c = torch.full((n,), 77, dtype=torch.uint8, device="cuda") if counts else None
    ring.lookupn_dev(d_keys.data_ptr(), n, 3, d_o.data_ptr(), d_c.data_ptr() if counts else None)
    return d_o, d_c


def host(res, n):
    torch.cuda.synchronize()
    d_o, d_c = res
    return d_o.cpu().numpy().view(np.uint32).reshape(n, 3), (d_c.cpu().numpy() if d_c is not None else None)


def lookupn(ring, d_keys, n, counts=True):
    return host(launch(ring, d_keys, n, counts), n)


def debug_line(capfd):
    m = LINE.search(capfd.readouterr().err)
    assert m, "no RP_LOOKUP_DEBUG line"
    keys, deferred, over, sort, ticket, grid, stagger = (int(x) for x in m.groups())
    return {"keys": keys, "deferred": deferred, "over": over, "sort": sort, "ticket": ticket, "grid": grid,
            "stagger": stagger}


def ticket_env(grid, stagger, **more):
    return env(RP_LOOKUP_TICKET=1, RP_LOOKUP_TICKET_GRID=grid, RP_LOOKUP_STAGGER=stagger, RP_LOOKUP_GRID=None,
               RP_LOOKUP_SORT=None, **more)


def strided_env(**more):
    return env(RP_LOOKUP_TICKET=0, RP_LOOKUP_TICKET_GRID=None, RP_LOOKUP_STAGGER=None, RP_LOOKUP_GRID=None,
               RP_LOOKUP_SORT=None, **more)


@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("n", KEY_COUNTS)
def test_ticket_vs_oracle_and_strided(gpu, orc, n, grid, capfd):
    ring, d_keys, (want, wcnt) = state(gpu, orc)
    tiles = n // TILE
    for stagger in (0, 4):
        for counts in (True, False):
            capfd.readouterr()
            with ticket_env(grid, stagger, RP_LOOKUP_DEBUG=1):
                got, gcnt = lookupn(ring, d_keys, n, counts)
            tk = debug_line(capfd)
            with strided_env(RP_LOOKUP_DEBUG=1):
                ref, rcnt = lookupn(ring, d_keys, n, counts)
            st = debug_line(capfd)
            # the sorted kernel took the tiles in both calls, in the form asked for
            assert tk["sort"] == st["sort"] == 256
            assert tk["ticket"] == 1 and st["ticket"] == 0
            assert tk["stagger"] == stagger
            if grid is not None:
                assert tk["grid"] == grid  # the forced grid is not capped at the tile count
            else:
                assert 1 <= tk["grid"] <= tiles  # what is resident, capped at the tile count
            assert np.array_equal(got, want[:n]), (stagger, counts)
            assert np.array_equal(got, ref), (stagger, counts)
            if counts:
                assert np.array_equal(gcnt, wcnt[:n]), stagger
                assert np.array_equal(gcnt, rcnt), stagger
            assert tk["keys"] == st["keys"] >= tiles * TILE
            assert tk["deferred"] == st["deferred"]
            assert tk["over"] == st["over"] == 0


@pytest.mark.parametrize("grid", GRIDS)
def test_counter_is_put_back_between_launches(gpu, orc, grid):
    """Three launches queued back to back on one ring and stream, nothing waited for in between."""
    ring, d_keys, (want, wcnt) = state(gpu, orc)
    n = TILE * 33
    with ticket_env(grid, 0):
        queued = [launch(ring, d_keys, n) for _ in range(3)]
    for res in queued:
        got, gcnt = host(res, n)
        assert np.array_equal(got, want[:n])
        assert np.array_equal(gcnt, wcnt[:n])


@pytest.mark.parametrize("grid", GRIDS)
def test_many_tiles_then_one_tile(gpu, orc, grid):
    ring, d_keys, (want, wcnt) = state(gpu, orc)
    with ticket_env(grid, 0):
        big = launch(ring, d_keys, TILE * 33)
        small = launch(ring, d_keys, TILE)
    for res, n in ((big, TILE * 33), (small, TILE)):
        got, gcnt = host(res, n)
        assert np.array_equal(got, want[:n]), n
        assert np.array_equal(gcnt, wcnt[:n]), n


@pytest.mark.parametrize("grid", GRIDS)
def test_ticket_call_then_strided_call_then_ticket_call(gpu, orc, grid):
    ring, d_keys, (want, wcnt) = state(gpu, orc)
    n = TILE * 5 + 77
    with ticket_env(grid, 4):
        first = launch(ring, d_keys, n)
    with strided_env():
        second = launch(ring, d_keys, n)
    with ticket_env(grid, 0):
        third = launch(ring, d_keys, n)
    for res in (first, second, third):
        got, gcnt = host(res, n)
        assert np.array_equal(got, want[:n])
        assert np.array_equal(gcnt, wcnt[:n])


def test_an_explicit_grid_keeps_the_strided_kernel(gpu, orc, capfd):
    """RP_LOOKUP_GRID means what it meant: the strided kernel at that grid, whatever RP_LOOKUP_TICKET."""
    ring, d_keys, (want, _) = state(gpu, orc)
    n = TILE * 5 + 77
    capfd.readouterr()
    with env(RP_LOOKUP_TICKET=1, RP_LOOKUP_GRID=2, RP_LOOKUP_DEBUG=1, RP_LOOKUP_TICKET_GRID=None,
             RP_LOOKUP_STAGGER=None, RP_LOOKUP_SORT=None):
        got, _ = lookupn(ring, d_keys, n)
    line = debug_line(capfd)
    assert line["sort"] == 256 and line["ticket"] == 0
    assert np.array_equal(got, want[:n])
