"""CPU tests of the hand-off entry points (no device calls): the header declares them in their
place, librpamd.so exports them, SIGNATURES binds them, the Python wrappers exist, a null handle is
RP_EINVAL with a message naming it, and the gfx950 code objects of the k_handoff instantiations
keep what DESIGN §4.2e states (no scratch memory, launch bound equal to the launch size)."""
import os
import re

import pytest

from test_ring_load_capi import LLVM, REPO, _kernels

NEW = ["rp_ring_handoff_dev", "rp_ring_handoff", "rp_ring_handoff_hashes"]


def test_header_declares_and_library_exports(rpa):
    with open(os.path.join(REPO, "include", "ringpop_amd.h")) as f:
        src = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    L = rpa.lib()
    for s in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % s, src), s
        assert hasattr(L, s) and s in rpa.SIGNATURES, s
    # after the snapshot dump, before the membership section
    assert src.index("rp_ring_snap_dump") < src.index("rp_ring_handoff_dev")
    assert max(src.index(s + "(") for s in NEW) < src.index("rp_members_create")
    order = list(rpa.SIGNATURES)
    assert order.index("rp_ring_snap_dump") < min(order.index(s) for s in NEW)
    assert max(order.index(s) for s in NEW) < order.index("rp_members_create")
    assert L.rp_version() >= (1 << 16) | 3  # the minor version these entry points came with


def test_signatures_match_the_header(rpa):
    """The bound argument counts equal the header's parameter counts."""
    with open(os.path.join(REPO, "include", "ringpop_amd.h")) as f:
        src = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    for s in NEW:
        params = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % s, src).group(1)
        assert len(params.split(",")) == len(rpa.SIGNATURES[s][1]), s


def test_python_wrappers_exist(rpa):
    for m in ("handoff_ids", "handoffPlan", "handoff_dev"):
        assert callable(getattr(rpa.HashRing, m)), m


def test_null_handles_are_einval_with_a_message(rpa):
    L = rpa.lib()
    calls = [
        lambda: L.rp_ring_handoff_dev(None, None, None, None, 36, 0, 3, 0xFFFFFFFF, 0, None, None, None, None, None,
                                      None, None, None),
        lambda: L.rp_ring_handoff(None, None, None, None, 36, 0, 3, 0xFFFFFFFF, 0, None, None, None, None, None,
                                  None, None),
        lambda: L.rp_ring_handoff_hashes(None, None, None, 0, 3, 0xFFFFFFFF, 0, None, None, None, None, None, None,
                                         None),
    ]
    for i, call in enumerate(calls):
        assert call() == -1, i
        err = L.rp_last_error()
        assert b"null" in err and b"handle" in err and b"ring" in err, (i, err)


def test_handoff_kernel_resources(rpa):
    if not os.path.exists(os.path.join(LLVM, "llvm-objdump")):
        pytest.skip("no ROCm LLVM tools")
    ks = _kernels(rpa.LIB_PATH)
    with open(os.path.join(REPO, "ringpop-node_amd", "csrc", "rp_ring.hip")) as f:
        src = f.read()
    threads = int(re.search(r"kLkThreads = (\d+);", src).group(1))
    mine = {n: k for n, k in ks.items() if "k_handoff" in n and "k_handoff_" not in n}
    assert len(mine) == 6, sorted(mine)  # rows of 1, up to 4 and up to 8 owners; streamed and generic keys
    for n, k in mine.items():
        assert k.get("private_segment_fixed_size", 0) == 0, n  # no scratch memory
        assert k["max_flat_workgroup_size"] == threads, n  # the launch size
    for name in ("k_handoff_heads", "k_handoff_emit"):
        assert sum(name in n for n in ks) == 1, name
