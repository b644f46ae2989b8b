"""Membership.update's dispatch rule on a CPU: csrc/rp_members_plan.h (the knob reader
members_knobs(), the fold plan fold_plan(), the checksum pool ck_pool() and string_mode()) compiled
with the host compiler into tests/members_plan_driver.cpp and run as a child process, against the
table below. The table is the rule as Members::update_dev and checksum_dev applied it before the
plan existed (use_bucket_fold, fuse_fold, string_mode, the drain condition, the pool resize),
written out by hand. Its size rows (2^29 changes, 8M ids) are taken by no GPU test. No GPU, nothing
loaded into Python.

Two rows differ from that code on purpose: RP_MEMBERS_FUSE=2 no longer drains a deferred string
(the drain test read the variable by another rule than the fold did), and RP_MEMBERS_SORTED_FOLD is
a per-batch input like the others (it was fixed when the handle was created)."""
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M22, M19, M29 = 1 << 22, 1 << 19, 1 << 29
CAP8M = 8 << 20


def row(name, want, k=2000, cap=3000, names=3000, damp=0, ranged=0, id_lo=0, id_hi=0, pw_on=0, pw_same=0,
        need=200_000, **env):
    return name, (k, cap, names, damp, ranged, id_lo, id_hi, pw_on, pw_same, need), env, want


def knob(**kw):
    """RP_ names are long: F=..., B=..., S=... stand for the RP_MEMBERS_ fold knobs."""
    full = {"S": "RP_MEMBERS_SORTED_FOLD", "B": "RP_MEMBERS_BUCKET_FOLD", "F": "RP_MEMBERS_FUSE",
            "SB": "RP_MEMBERS_SIDE_BUILD", "CK": "RP_MEMBERS_CK_BYTES", "GS": "RP_MEMBERS_GROUP_SLOTS",
            "REC8": "RP_BK_REC8", "DIRECT": "RP_BK_DIRECT", "SGRID": "RP_BK_SGRID", "PROF": "RP_BK_PROF_PRINT"}
    return {full[k]: v for k, v in kw.items()}


BUCKET_LARGE = dict(path="bucket", nb=1024, b_lo=0, b_hi=1024, ntiles=128, sgrid=0, rec8=1, direct=1, gather=0,
                    fuse=0, bits=0, nparts=1024, drain=0)
RANGED = dict(k=2000, cap=20_000, names=20_000, ranged=1)  # 5 buckets

ROWS = [
    # the size rule: from 2^19 changes the bucket path, up to 2^29 - 1 (the batch index shares a word with the status)
    row("size-below", dict(path="grouped", nb=1024, nparts=2048, ntiles=0, fuse=0, bits=0, drain=0), k=M19 - 1, cap=M22,
        names=M22),
    row("size-at", BUCKET_LARGE, k=M19, cap=M22, names=M22),
    row("index-below", dict(path="bucket", ntiles=131072, nparts=1024), k=M29 - 1, cap=M22, names=M22),
    row("index-at", dict(path="grouped", nparts=2097152), k=M29, cap=M22, names=M22),
    row("index-at-forced", dict(path="grouped"), k=M29, cap=M22, names=M22, **knob(B="1")),
    # the table: at most 2,048 buckets of 4,096 ids
    row("table-8m", dict(path="bucket", nb=2048, b_hi=2048, nparts=2048), k=M19, cap=CAP8M, names=CAP8M),
    row("table-8m-1", dict(path="grouped", nb=2049, nparts=2048), k=M19, cap=CAP8M + 1, names=CAP8M),
    row("table-8m-1-forced", dict(path="grouped"), k=M19, cap=CAP8M + 1, names=CAP8M, **knob(B="1")),
    row("small-default", dict(path="grouped", nb=1, nparts=8, fuse=0, drain=0, bits=0)),
    row("one-change", dict(path="grouped", nparts=1), k=1),
    row("empty-batch", dict(path="empty", nparts=0, drain=0), k=0),
    # damp scoring and the sorted fold keep a batch off the bucket path whatever the knob says
    row("damp-forced", dict(path="grouped", nparts=8), damp=1, **knob(B="1")),
    row("damp-large", dict(path="grouped"), k=M19, cap=M22, names=M22, damp=1),
    row("sorted-forced", dict(path="sorted", bits=16, nparts=0, fuse=0), **knob(S="1", B="1")),
    row("sorted-large", dict(path="sorted", bits=24), k=M19, cap=M22, names=M22, **knob(S="1")),
    row("sorted-damp", dict(path="sorted"), damp=1, **knob(S="1")),
    # ranged: whole buckets through the bucket path at any size
    row("ranged-whole", dict(path="bucket", nb=5, b_lo=1, b_hi=3, ntiles=1, direct=1, gather=0, nparts=5, drain=0),
        id_lo=4096, id_hi=12288, **RANGED),
    row("ranged-to-cap", dict(path="bucket", b_lo=2, b_hi=5), id_lo=8192, id_hi=20_001, **RANGED),
    row("ranged-all", dict(path="bucket", b_lo=0, b_hi=5), id_lo=0, id_hi=0xFFFFFFFF, **RANGED),
    row("ranged-past", dict(path="empty", b_lo=5, b_hi=5), id_lo=24576, id_hi=28672, **RANGED),
    row("ranged-nothing", dict(path="empty", b_lo=1, b_hi=1), id_lo=4096, id_hi=4096, **RANGED),
    row("ranged-bucket-off", dict(path="bucket"), id_lo=0, id_hi=4096, **RANGED, **knob(B="0")),
    row("ranged-no-changes", dict(path="empty", drain=0), id_lo=0, id_hi=4096, **dict(RANGED, k=0)),
    row("ranged-damp", dict(path="grouped"), id_lo=0, id_hi=4096, damp=1, **RANGED),  # refused
    row("ranged-damp-no-changes", dict(path="grouped"), id_lo=0, id_hi=4096, damp=1, **dict(RANGED, k=0)),  # refused
    row("ranged-sorted", dict(path="sorted"), id_lo=0, id_hi=4096, **RANGED, **knob(S="1")),  # refused
    row("ranged-too-many", dict(path="grouped"), id_lo=0, id_hi=4096, **dict(RANGED, cap=CAP8M + 1)),  # refused
    row("ranged-index", dict(path="grouped"), id_lo=0, id_hi=4096, **dict(RANGED, k=M29)),  # refused
    # a pending deferred string: only the grouped fold's launch on its own stream carries it
    row("drain-other-stream", dict(path="grouped", drain=1), pw_on=1, pw_same=0),
    row("drain-same-stream", dict(path="grouped", drain=0), pw_on=1, pw_same=1),
    row("drain-bucket", dict(path="bucket", drain=1), pw_on=1, pw_same=1, **knob(B="1")),
    row("drain-bucket-large", dict(path="bucket", drain=1), k=M19, cap=M22, names=M22, pw_on=1, pw_same=1),
    row("drain-sorted", dict(path="sorted", drain=1), pw_on=1, pw_same=1, **knob(S="1")),
    row("drain-fuse", dict(path="grouped", fuse=1, drain=1), pw_on=1, pw_same=1, **knob(F="1")),
    row("drain-fuse-2", dict(path="grouped", fuse=0, drain=0), pw_on=1, pw_same=1, **knob(F="2")),  # was drain=1
    row("drain-none-pending", dict(path="grouped", fuse=1, drain=0), pw_on=0, pw_same=1, **knob(F="1")),
    row("drain-none-pending-bucket", dict(path="bucket", drain=0), pw_on=0, pw_same=0, **knob(B="1")),
    row("drain-empty-batch", dict(path="empty", drain=0), k=0, pw_on=1, pw_same=0),
    row("drain-ranged", dict(path="bucket", drain=1), id_lo=0, id_hi=4096, pw_on=1, pw_same=1, **RANGED),
    row("drain-ranged-past", dict(path="empty", drain=1), id_lo=24576, id_hi=28672, pw_on=1, pw_same=1, **RANGED),
    # the scatter's grid
    row("sgrid-0", dict(path="bucket", ntiles=128, sgrid=0), k=M19, cap=M22, names=M22, **knob(SGRID="0")),
    row("sgrid-48", dict(sgrid=48), k=M19, cap=M22, names=M22, **knob(SGRID="48")),
    row("sgrid-abc", dict(sgrid=0), k=M19, cap=M22, names=M22, **knob(SGRID="abc")),
    row("sgrid-48x", dict(sgrid=0), k=M19, cap=M22, names=M22, **knob(SGRID="48x")),
    row("sgrid-empty", dict(sgrid=0), k=M19, cap=M22, names=M22, **knob(SGRID="")),
    row("sgrid-127", dict(sgrid=127), k=M19, cap=M22, names=M22, **knob(SGRID="127")),
    row("sgrid-ntiles", dict(sgrid=0), k=M19, cap=M22, names=M22, **knob(SGRID="128")),
    row("sgrid-above", dict(sgrid=0), k=M19, cap=M22, names=M22, **knob(SGRID="200")),
    row("sgrid-one-tile", dict(ntiles=1, sgrid=0), **knob(B="1", SGRID="1")),
    row("sgrid-grouped", dict(path="grouped", sgrid=0), **knob(SGRID="48")),
    # record width and who writes the applied flags
    row("rec8-0", dict(rec8=0, direct=1), **knob(B="1", REC8="0")),
    row("rec8-00", dict(rec8=1), **knob(B="1", REC8="00")),
    row("rec8-empty", dict(rec8=1), **knob(B="1", REC8="")),
    row("rec8-1", dict(rec8=1), **knob(B="1", REC8="1")),
    row("direct-0", dict(direct=0, gather=1, rec8=1), **knob(B="1", DIRECT="0")),
    row("direct-00", dict(direct=1, gather=0), **knob(B="1", DIRECT="00")),
    row("direct-empty", dict(direct=1, gather=0), **knob(B="1", DIRECT="")),
    row("direct-0-ranged", dict(path="bucket", direct=1, gather=0), id_lo=0, id_hi=4096, **RANGED, **knob(DIRECT="0")),
    row("direct-0-grouped", dict(path="grouped", direct=0, gather=0), **knob(DIRECT="0")),
    # parse rules
    row("bucket-empty", dict(path="grouped"), **knob(B="")),
    row("bucket-empty-large", dict(path="bucket"), k=M19, cap=M22, names=M22, **knob(B="")),
    row("bucket-0", dict(path="grouped"), **knob(B="0")),
    row("bucket-0-large", dict(path="grouped"), k=M19, cap=M22, names=M22, **knob(B="0")),
    row("bucket-1", dict(path="bucket", nb=1, ntiles=1, nparts=1), **knob(B="1")),
    row("bucket-yes", dict(path="bucket"), **knob(B="yes")),
    row("bucket-01", dict(path="grouped"), **knob(B="01")),
    row("sorted-1", dict(path="sorted"), **knob(S="1")),
    row("sorted-0", dict(path="grouped"), **knob(S="0")),
    row("sorted-empty", dict(path="grouped"), **knob(S="")),
    row("sorted-yes", dict(path="sorted"), **knob(S="yes")),
    row("sorted-01", dict(path="grouped"), **knob(S="01")),
    row("fuse-1", dict(fuse=1), **knob(F="1")),
    row("fuse-2", dict(fuse=0), **knob(F="2")),
    row("fuse-0", dict(fuse=0), **knob(F="0")),
    row("fuse-10", dict(fuse=1), **knob(F="10")),
    row("fuse-empty", dict(fuse=0), **knob(F="")),
    row("fuse-bucket", dict(path="bucket", fuse=0), **knob(F="1", B="1")),
    row("fuse-sorted", dict(path="sorted", fuse=0), **knob(F="1", S="1")),
    row("side-unset", dict(mode_ov=2, mode_plain=0)),
    row("side-0", dict(mode_ov=0, mode_plain=0), **knob(SB="0")),
    row("side-1", dict(mode_ov=1, mode_plain=0), **knob(SB="1")),
    row("side-2", dict(mode_ov=2, mode_plain=0), **knob(SB="2")),
    row("side-01", dict(mode_ov=0, mode_plain=0), **knob(SB="01")),
    row("side-x", dict(mode_ov=2, mode_plain=0), **knob(SB="x")),
    row("side-empty", dict(mode_ov=2, mode_plain=0), **knob(SB="")),
    row("prof-unset", dict(prof=0)),
    row("prof-empty", dict(prof=1), **knob(PROF="")),
    row("prof-0", dict(prof=1), **knob(PROF="0")),
    # the checksum pool: slots of `need` bytes in the budget, at most 1,024; groups of at most half of them, at most 4
    row("pool-c3", dict(nslots=1024, group_slots=512, ngroups=2), need=4_700_000),  # 6 GiB / 4.7 MB = 1,370
    row("pool-default-fits", dict(nslots=1024, group_slots=512, ngroups=2)),
    row("pool-three", dict(nslots=3, group_slots=1, ngroups=3), **knob(CK="600000")),
    row("pool-two", dict(nslots=2, group_slots=1, ngroups=2), **knob(CK="599999")),
    row("pool-below-need", dict(nslots=1, group_slots=1, ngroups=1), **knob(CK="100000")),
    row("pool-100", dict(nslots=100, group_slots=50, ngroups=2), **knob(CK="20000000")),
    row("pool-groups-64", dict(nslots=1024, group_slots=64, ngroups=4), need=4_700_000, **knob(GS="64")),
    row("pool-groups-300", dict(nslots=1024, group_slots=300, ngroups=3), **knob(GS="300")),
    row("pool-groups-600", dict(nslots=1024, group_slots=512, ngroups=2), **knob(GS="600")),
    row("pool-groups-0", dict(nslots=1024, group_slots=512, ngroups=2), **knob(GS="0")),
    row("pool-bytes-abc", dict(nslots=1024, group_slots=512, ngroups=2), **knob(CK="abc")),
    row("pool-bytes-empty", dict(nslots=1024, group_slots=512, ngroups=2), **knob(CK="")),
    # the radix sort's key bits: whole bytes that hold every id
    row("bits-1", dict(path="sorted", bits=8), names=1, **knob(S="1")),
    row("bits-255", dict(bits=8), names=255, **knob(S="1")),
    row("bits-256", dict(bits=8), names=256, **knob(S="1")),
    row("bits-257", dict(bits=16), names=257, **knob(S="1")),
    row("bits-65536", dict(bits=16), names=65536, **knob(S="1")),
    row("bits-65537", dict(bits=24), names=65537, **knob(S="1")),
    row("bits-2-24", dict(bits=24), names=1 << 24, **knob(S="1")),
    row("bits-2-24-1", dict(bits=32), names=(1 << 24) + 1, **knob(S="1")),
]


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("members_plan") / "members_plan_driver")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I",
                           os.path.join(REPO, "ringpop-node_amd", "csrc"),
                           os.path.join(REPO, "tests", "members_plan_driver.cpp"), "-o", exe])
    text = "".join("%s %s\n" % (" ".join(map(str, nums)), " ".join("%s=%s" % kv for kv in env.items()))
                   for _, nums, env, _ in ROWS)
    out = subprocess.run([exe], input=text, capture_output=True, text=True, check=True, timeout=60).stdout
    got = [dict(f.split("=", 1) for f in line.split()) for line in out.splitlines()]
    assert len(got) == len(ROWS)
    return {r[0]: g for r, g in zip(ROWS, got)}


def test_row_ids_are_unique():
    assert len({r[0] for r in ROWS}) == len(ROWS)


@pytest.mark.parametrize("r", ROWS, ids=[r[0] for r in ROWS])
def test_members_plan_row(lines, r):
    name, nums, _, want = r
    got = lines[name]
    assert {k: got[k] for k in want} == {k: str(v) for k, v in want.items()}, got
    # what only one path has is left at zero on the others
    if got["path"] != "bucket":
        assert [got[f] for f in ("ntiles", "sgrid", "rec8", "direct", "gather")] == ["0"] * 5, got
    if got["path"] != "grouped":
        assert got["fuse"] == "0", got
    if got["path"] != "sorted":
        assert got["bits"] == "0", got
    assert int(got["gather"]) + int(got["direct"]) == (got["path"] == "bucket"), got
    assert int(got["drain"]) <= nums[7], got  # nothing to drain unless a string is pending
    assert int(got["nslots"]) >= int(got["group_slots"]) * int(got["ngroups"]) or got["nslots"] == "1", got
