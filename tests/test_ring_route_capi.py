"""CPU tests of the routing-agreement entry points (no device calls): the header declares them in
their place, librpamd.so exports them, SIGNATURES binds them in order with the header's argument
counts, the Python wrappers exist, a null handle is RP_EINVAL with a message naming it, and the
gfx950 code objects of k_route_pack / k_route keep what DESIGN §4.2f states (no scratch memory,
launch bound equal to the launch size)."""
import os
import re

import pytest

from test_ring_load_capi import LLVM, REPO, _kernels

RING = ["rp_ring_route_views_dev", "rp_ring_route_views"]
SIM = ["rp_sim_ring_members", "rp_sim_routing", "rp_sim_routing_hashes"]


def _header():
    with open(os.path.join(REPO, "include", "ringpop_amd.h")) as f:
        return re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)


def test_header_declares_and_library_exports(rpa):
    src = _header()
    L = rpa.lib()
    for s in RING + SIM:
        assert re.search(r"\bint\s+%s\s*\(" % s, src), s
        assert hasattr(L, s) and s in rpa.SIGNATURES, s
    # the ring level: after the hand-off section, before the membership section
    assert src.index("rp_ring_handoff_hashes(") < min(src.index(s + "(") for s in RING)
    assert max(src.index(s + "(") for s in RING) < src.index("rp_members_create")
    # the simulator level: in the scenarios section
    assert src.index("rp_sim_create_scenario(") < min(src.index(s + "(") for s in SIM)
    order = list(rpa.SIGNATURES)
    assert order.index("rp_ring_handoff_hashes") < min(order.index(s) for s in RING)
    assert max(order.index(s) for s in RING) < order.index("rp_members_create")
    assert order.index(RING[0]) < order.index(RING[1])
    assert order.index("rp_sim_create_scenario") < min(order.index(s) for s in SIM)
    assert [order.index(s) for s in SIM] == sorted(order.index(s) for s in SIM)
    assert L.rp_version() >= (1 << 16) | 4  # the minor version these entry points came with


def test_signatures_match_the_header(rpa):
    """The bound argument counts equal the header's parameter counts."""
    src = _header()
    for s in RING + SIM:
        params = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % s, src).group(1)
        assert len(params.split(",")) == len(rpa.SIGNATURES[s][1]), s
    assert len(rpa.SIGNATURES[RING[0]][1]) == len(rpa.SIGNATURES[RING[1]][1]) + 1  # the stream


def test_python_wrappers_exist(rpa):
    for m in ("route_views_dev", "route_view_ids", "route_view_hashes", "routeViews"):
        assert callable(getattr(rpa.HashRing, m)), m
    for cls in (rpa.GossipSim, rpa.SimShard, rpa.ShardedGossipSim):
        for m in ("ring_members", "routing"):
            assert callable(getattr(cls, m)), (cls.__name__, m)


def test_null_handles_are_einval_with_a_message(rpa):
    L = rpa.lib()
    ring_calls = [
        lambda: L.rp_ring_route_views_dev(None, None, None, 36, None, 0, None, 0, 1, 0, None, 0, None, None, 0, None,
                                          None, None, None, None, None),
        lambda: L.rp_ring_route_views(None, None, None, 36, None, 0, None, 0, 1, 0, None, 0, None, None, 0, None,
                                      None, None, None, None),
    ]
    for i, call in enumerate(ring_calls):
        assert call() == -1, i
        err = L.rp_last_error()
        assert b"null" in err and b"handle" in err and b"ring" in err, (i, err)
    sim_calls = [
        lambda: L.rp_sim_ring_members(None, 0, None),
        lambda: L.rp_sim_routing(None, None, None, None, 36, 0, None, None, None, None, None),
        lambda: L.rp_sim_routing_hashes(None, None, None, 0, None, None, None, None, None),
    ]
    for i, call in enumerate(sim_calls):
        assert call() == -1, i
        err = L.rp_last_error()
        assert b"null" in err and b"handle" in err and b"sim" in err, (i, err)


def test_route_kernel_resources(rpa):
    if not os.path.exists(os.path.join(LLVM, "llvm-objdump")):
        pytest.skip("no ROCm LLVM tools")
    ks = _kernels(rpa.LIB_PATH)
    with open(os.path.join(REPO, "ringpop-node_amd", "csrc", "rp_ring.hip")) as f:
        src = f.read()
    threads = int(re.search(r"kRouteThreads = (\d+);", src).group(1))
    pack_threads = int(re.search(r"kRoutePackThreads = (\d+);", src).group(1))
    walk = {n: k for n, k in ks.items() if "k_route" in n and "k_route_pack" not in n}
    assert len(walk) == 4, sorted(walk)  # streamed and generic keys, with and without the owners output
    for n, k in walk.items():
        assert k.get("private_segment_fixed_size", 0) == 0, n  # no scratch memory
        assert k["max_flat_workgroup_size"] == threads, n  # the launch size
    pack = {n: k for n, k in ks.items() if "k_route_pack" in n}
    assert len(pack) == 1, sorted(pack)
    for n, k in pack.items():
        assert k.get("private_segment_fixed_size", 0) == 0, n
        assert k["max_flat_workgroup_size"] == pack_threads, n
