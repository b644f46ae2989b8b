"""CPU tests of the key-free routing-agreement entry points (no device calls): the header declares
them in their place, librpamd.so exports them, SIGNATURES binds them in order with the header's
argument counts, the Python wrappers exist, a null handle is RP_EINVAL with a message naming it,
and the gfx950 code objects of k_share_reduce / k_share_carry / k_share_apply keep what DESIGN
§4.2g states (no scratch memory, launch bound equal to the launch size)."""
import os
import re

import pytest

from test_ring_load_capi import LLVM, REPO, _kernels

RING = ["rp_ring_route_share_dev", "rp_ring_route_share"]
SIM = ["rp_sim_routing_share"]


def _header():
    with open(os.path.join(REPO, "include", "ringpop_amd.h")) as f:
        return re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)


def test_header_declares_and_library_exports(rpa):
    src = _header()
    L = rpa.lib()
    for s in RING + SIM:
        assert re.search(r"\bint\s+%s\s*\(" % s, src), s
        assert hasattr(L, s) and s in rpa.SIGNATURES, s
    # the ring level: after rp_ring_route_views, before the membership section
    assert src.index("rp_ring_route_views(") < min(src.index(s + "(") for s in RING)
    assert max(src.index(s + "(") for s in RING) < src.index("rp_members_create")
    assert src.index(RING[0] + "(") < src.index(RING[1] + "(")
    # the simulator level: after rp_sim_routing_hashes, before rp_sim_census
    assert src.index("rp_sim_routing_hashes(") < src.index(SIM[0] + "(") < src.index("rp_sim_census(")
    order = list(rpa.SIGNATURES)
    assert order.index("rp_ring_route_views") < order.index(RING[0]) < order.index(RING[1]) \
        < order.index("rp_members_create")
    assert order.index("rp_sim_routing_hashes") < order.index(SIM[0]) < order.index("rp_sim_census")
    assert L.rp_version() >= (1 << 16) | 5  # the minor version these entry points came with


def test_signatures_match_the_header(rpa):
    """The bound argument counts equal the header's parameter counts."""
    src = _header()
    for s in RING + SIM:
        params = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % s, src).group(1)
        assert len(params.split(",")) == len(rpa.SIGNATURES[s][1]), s
    assert len(rpa.SIGNATURES[RING[0]][1]) == len(rpa.SIGNATURES[RING[1]][1]) + 1  # the stream


def test_python_wrappers_exist(rpa):
    for m in ("route_share_dev", "route_share_ids", "routeShare"):
        assert callable(getattr(rpa.HashRing, m)), m
    assert callable(rpa.GossipSim.routingShare)
    assert callable(rpa.SimShard.routing_share)
    assert callable(rpa.ShardedGossipSim.routingShare)


def test_null_handles_are_einval_with_a_message(rpa):
    L = rpa.lib()
    ring_calls = [
        lambda: L.rp_ring_route_share_dev(None, None, 0, 1, 0, None, 0, None, None, 0, None, None, None, 0, None),
        lambda: L.rp_ring_route_share(None, None, 0, 1, 0, None, 0, None, None, 0, None, None, None, 0),
    ]
    for i, call in enumerate(ring_calls):
        assert call() == -1, i
        err = L.rp_last_error()
        assert b"null" in err and b"handle" in err and b"ring" in err, (i, err)
    assert L.rp_sim_routing_share(None, None, None, None, None, None, 0) == -1
    err = L.rp_last_error()
    assert b"null" in err and b"handle" in err and b"sim" in err, err


def test_share_kernel_resources(rpa):
    if not os.path.exists(os.path.join(LLVM, "llvm-objdump")):
        pytest.skip("no ROCm LLVM tools")
    ks = _kernels(rpa.LIB_PATH)
    with open(os.path.join(REPO, "ringpop-node_amd", "csrc", "rp_ring.hip")) as f:
        src = f.read()
    threads = int(re.search(r"kShareThreads = (\d+);", src).group(1))
    carry_threads = int(re.search(r"kShareCarryThreads = (\d+);", src).group(1))
    want = {"k_share_reduce": (1, threads), "k_share_carry": (1, carry_threads),
            "k_share_apply": (2, threads)}  # apply: with and without pos_wrong
    for name, (count, bound) in want.items():
        found = {n: k for n, k in ks.items() if name in n}
        assert len(found) == count, (name, sorted(found))
        for n, k in found.items():
            assert k.get("private_segment_fixed_size", 0) == 0, n  # no scratch memory
            assert k["max_flat_workgroup_size"] == bound, n  # the launch size
