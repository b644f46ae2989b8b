"""CPU tests of rp_sim_ring_checksums (no device calls): the header declares it next to
rp_sim_ring_members, librpamd.so exports it, SIGNATURES binds it there with the header's argument
count, the Python wrappers exist on every simulator class, and a null handle is RP_EINVAL with a
message naming it."""
import os
import re

from test_ring_load_capi import REPO

NAME = "rp_sim_ring_checksums"


def _header():
    with open(os.path.join(REPO, "include", "ringpop_amd.h")) as f:
        return re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)


def test_header_declares_and_library_exports(rpa):
    src = _header()
    L = rpa.lib()
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % NAME, src)
    assert m and hasattr(L, NAME) and NAME in rpa.SIGNATURES
    assert len(m.group(1).split(",")) == len(rpa.SIGNATURES[NAME][1]) == 2
    assert src.index("rp_sim_ring_members(") < src.index(NAME + "(") < src.index("rp_sim_routing(")
    order = list(rpa.SIGNATURES)
    assert order.index(NAME) == order.index("rp_sim_ring_members") + 1
    assert L.rp_version() >= (1 << 16) | 8  # the minor version this entry point came with


def test_python_wrappers_exist(rpa):
    for cls in (rpa.GossipSim, rpa.SimShard, rpa.ShardedGossipSim):
        assert callable(getattr(cls, "ring_checksums")), cls.__name__


def test_null_handle_is_einval_with_a_message(rpa):
    L = rpa.lib()
    assert L.rp_sim_ring_checksums(None, None) == -1
    err = L.rp_last_error()
    assert b"null" in err and b"handle" in err and b"sim" in err, err
