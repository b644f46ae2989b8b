"""CPU tests of the owner-load / hash-space-share entry points (no device calls): the header
declares them, librpamd.so exports them, the Python wrappers exist, a null handle is RP_EINVAL
with a message, and the gfx950 code object of k_owner_load keeps the resources DESIGN §4.2c
states (no scratch, registers and LDS for two 1,024-thread workgroups a CU)."""
import os
import re
import shutil
import subprocess
import tempfile

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/lib/llvm/bin"
LDS_PER_CU = 160 * 1024
SIMDS = 4
NEW = ["rp_ring_id_bound", "rp_ring_owner_load_dev", "rp_ring_owner_load", "rp_ring_owner_load_hashes",
       "rp_ring_snap_owner_load_dev", "rp_ring_owner_share", "rp_ring_snap_owner_share"]
# two workgroups a CU by registers (windows of at most 80 KB of dynamic LDS run two a
# CU, larger ones one); the launch size is the launch bound
PER_CU = 2
THREADS = 1024


def test_header_declares_and_library_exports(rpa):
    with open(os.path.join(REPO, "include", "ringpop_amd.h")) as f:
        src = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    L = rpa.lib()
    for s in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % s, src), s
        assert hasattr(L, s) and s in rpa.SIGNATURES, s
    # after the moved-keys block, before the membership section
    assert src.index("rp_ring_moved_hashes") < src.index("rp_ring_id_bound") < src.index("rp_members_create")
    assert rpa.lib().rp_version() >= (1 << 16) | 1  # the minor version these entry points came with


def test_python_wrappers_exist(rpa):
    for m in ("id_bound", "owner_load_ids", "owner_load_hashes", "owner_load_dev", "ownerLoad", "owner_share_ids",
              "ownerShare"):
        assert callable(getattr(rpa.HashRing, m)), m
    for m in ("id_bound", "owner_load_dev", "owner_share_ids"):
        assert callable(getattr(rpa.RingSnapshot, m)), m


def test_null_handles_are_einval_with_a_message(rpa):
    L = rpa.lib()
    calls = [
        lambda: L.rp_ring_id_bound(None, None),
        lambda: L.rp_ring_owner_load_dev(None, None, None, 36, 0, 3, 0, 0, None, None),
        lambda: L.rp_ring_owner_load(None, None, None, 36, 0, 3, 0, None),
        lambda: L.rp_ring_owner_load_hashes(None, None, 0, 3, 0, None),
        lambda: L.rp_ring_snap_owner_load_dev(None, None, None, 36, 0, 3, 0, 0, None, None),
        lambda: L.rp_ring_owner_share(None, 0, None),
        lambda: L.rp_ring_snap_owner_share(None, 0, None),
    ]
    for i, call in enumerate(calls):
        assert call() == -1, i
        assert b"null" in L.rp_last_error() and b"handle" in L.rp_last_error(), i


def _kernels(lib):
    """{mangled name: {field: int}} from the gfx950 code objects' metadata notes (as
    tests/test_kernel_resources.py reads them)."""
    tmp = tempfile.mkdtemp()
    try:
        so = os.path.join(tmp, "lib.so")
        shutil.copy(lib, so)  # llvm-objdump --offloading writes the bundles beside its input
        subprocess.run([os.path.join(LLVM, "llvm-objdump"), "--offloading", so], check=True,
                       capture_output=True, cwd=tmp)
        out = {}
        for f in sorted(os.listdir(tmp)):
            if not f.endswith("gfx950"):
                continue
            notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", os.path.join(tmp, f)],
                                   check=True, capture_output=True, text=True).stdout
            cur = None
            for line in notes.splitlines():
                m = re.match(r"^(  - |    )\.(\w+):\s+(\S+)", line)
                if not m:
                    continue
                if m.group(1) == "  - ":
                    cur = {}
                if cur is None:
                    continue
                key, val = m.group(2), m.group(3)
                if key == "name":
                    out[val] = cur
                elif val.isdigit():
                    cur[key] = int(val)
        return out
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def test_owner_load_kernel_resources(rpa):
    if not os.path.exists(os.path.join(LLVM, "llvm-objdump")):
        pytest.skip("no ROCm LLVM tools")
    ks = {n: k for n, k in _kernels(rpa.LIB_PATH).items() if "k_owner_load" in n}
    assert len(ks) == 5, sorted(ks)  # row widths 1-4 and the any-width form
    for n, k in ks.items():
        assert k.get("private_segment_fixed_size", 0) == 0, n  # no scratch
        assert k["max_flat_workgroup_size"] == THREADS, n
        assert k.get("group_segment_fixed_size", 0) == 0, n  # all LDS is the dynamic bin window
        regs = k.get("vgpr_count", 0) + k.get("agpr_count", 0)
        alloc = max(8, (regs + 7) // 8 * 8)
        waves_simd = min(8, 512 // alloc)
        per_simd = (THREADS // 64 + SIMDS - 1) // SIMDS
        assert waves_simd // per_simd >= PER_CU, (n, regs)
    # the windows: the default fills 128 KB (one workgroup a CU), half windows leave room for two
    with open(os.path.join(REPO, "ringpop-node_amd", "csrc", "rp_ring.hip")) as f:
        src = f.read()
    bins = int(re.search(r"kLoadBins = (\d+);", src).group(1))
    bins2 = int(re.search(r"kLoadBins2 = (\d+);", src).group(1))
    assert bins * 4 <= LDS_PER_CU and bins >= 30_000  # the C2 shape (10,000 servers x 3) in one window
    assert bins2 * 4 * PER_CU <= LDS_PER_CU
