"""CPU tests of the moved-ranges entry points (no device calls): the header declares them in their
place, librpamd.so exports them, SIGNATURES binds them, the Python wrappers exist, a null handle is
RP_EINVAL with a message naming it, and the gfx950 code objects of the four k_ranges_* kernels
keep what DESIGN §4.2d states (no scratch memory, launch bounds equal to the launch size)."""
import os
import re

import pytest

from test_ring_load_capi import LLVM, REPO, _kernels

NEW = ["rp_ring_moved_ranges_dev", "rp_ring_moved_ranges", "rp_ring_snap_moved_ranges_dev",
       "rp_ring_snap_moved_ranges", "rp_ring_snap_dump"]
# kernel -> (instantiations, launch size): rows of 1, up to 4 and up to 8 owners for the two
# kernels that walk rows
KERNELS = {"k_ranges_merge": (1, 256), "k_ranges_flag": (3, 256), "k_ranges_scan": (1, 1024),
           "k_ranges_write": (3, 256)}


def test_header_declares_and_library_exports(rpa):
    with open(os.path.join(REPO, "include", "ringpop_amd.h")) as f:
        src = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    L = rpa.lib()
    for s in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % s, src), s
        assert hasattr(L, s) and s in rpa.SIGNATURES, s
    # after the owner-share block, before the membership section
    assert src.index("rp_ring_snap_owner_share") < src.index("rp_ring_moved_ranges_dev")
    assert src.index("rp_ring_snap_dump") < src.index("rp_members_create")
    order = list(rpa.SIGNATURES)
    assert order.index("rp_ring_snap_owner_share") < min(order.index(s) for s in NEW)
    assert max(order.index(s) for s in NEW) < order.index("rp_members_create")
    assert L.rp_version() >= (1 << 16) | 2  # the minor version these entry points came with


def test_python_wrappers_exist(rpa):
    for m in ("moved_range_ids", "movedRanges", "movedShare", "moved_ranges_dev"):
        assert callable(getattr(rpa.HashRing, m)), m
    for m in ("moved_range_ids", "moved_ranges_dev", "dump"):
        assert callable(getattr(rpa.RingSnapshot, m)), m


def test_null_handles_are_einval_with_a_message(rpa):
    L = rpa.lib()
    calls = [
        (lambda: L.rp_ring_moved_ranges_dev(None, None, 3, 0, None, None, None, None, None, None, None), b"ring"),
        (lambda: L.rp_ring_moved_ranges(None, None, 3, 0, None, None, None, None, None, None), b"ring"),
        (lambda: L.rp_ring_snap_moved_ranges_dev(None, None, 3, 0, None, None, None, None, None, None, None),
         b"snapshot"),
        (lambda: L.rp_ring_snap_moved_ranges(None, None, 3, 0, None, None, None, None, None, None), b"snapshot"),
        (lambda: L.rp_ring_snap_dump(None, None, None, 0), b"snapshot"),
    ]
    for i, (call, which) in enumerate(calls):
        assert call() == -1, i
        err = L.rp_last_error()
        assert b"null" in err and b"handle" in err and which in err, (i, err)


def test_ranges_kernel_resources(rpa):
    if not os.path.exists(os.path.join(LLVM, "llvm-objdump")):
        pytest.skip("no ROCm LLVM tools")
    ks = _kernels(rpa.LIB_PATH)
    with open(os.path.join(REPO, "ringpop-node_amd", "csrc", "rp_ring.hip")) as f:
        src = f.read()
    assert int(re.search(r"kRngThreads = (\d+);", src).group(1)) == 256
    assert int(re.search(r"kRngScanThreads = (\d+);", src).group(1)) == 1024
    for name, (count, threads) in KERNELS.items():
        mine = {n: k for n, k in ks.items() if name in n}
        assert len(mine) == count, (name, sorted(mine))
        for n, k in mine.items():
            assert k.get("private_segment_fixed_size", 0) == 0, n  # no scratch memory
            assert k["max_flat_workgroup_size"] == threads, n  # the launch size
            assert k.get("group_segment_fixed_size", 0) <= 128, n  # a few counters, no LDS staging
