"""The gossip simulator's checksum-refresh rule on a CPU: csrc/rp_sim_plan.h (the knob reader
sim_knobs() and the plan ck_plan_begin / ck_plan_finish, d1_ck_kernel, early_ck_kernel) compiled
with the host compiler into tests/sim_plan_driver.cpp and run as a child process, against the
table below. The table is the rule as the code before the plan existed applied it, written out by
hand; its automatic rows (more 64-view groups than CUs, the kernel by the dirty count) are taken by
no GPU test, which would need more than 16,384 local nodes. No GPU, nothing loaded into Python.

The rule's description speaks of sixteen variables and of knobs in conv_local(); the code before
had twelve (the driver's kKnobs) and conv_local() reads none but through the refresh it starts.
Otherwise the two agree on every row."""
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CUS = 256
BIG = 100_000  # 1,563 groups of 64: the lane path by size

# (id, NL, G, nd, knobs, expected fields of the driver's line). nd None: the plan must not ask for
# the count (the driver then passes 0 whatever stands here).
PLAN = [
    ("default-small", 900, 1, None, {}, dict(kernel="pc<7>", twins=0, list=0, sort=0, key=1, pass1=1)),
    ("default-sharded", 900, 3, 500, {}, dict(kernel="pc<7>", twins=0, list=1, sort=1, radix=1, key=1, pass1=1)),
    ("auto-lanes", BIG, 1, 99_000, {}, dict(kernel="lanes", twins=1, list=1, sort=1, radix=1, key=1, pass1=0)),
    ("auto-pc32", BIG, 1, 40_000, {}, dict(kernel="pc<3,2>", twins=1, list=1, sort=0, radix=0, pass1=1)),
    ("pc32-edge-below", BIG, 1, 49_152, {}, dict(kernel="pc<3,2>")),  # 768 groups = 3 x 256
    ("pc32-edge-above", BIG, 1, 49_153, {}, dict(kernel="lanes")),
    ("per-cu-2", BIG, 1, 40_000, {"RP_SIM_PC32_PER_CU": "2"}, dict(kernel="lanes", sort=1)),  # 625 > 512
    ("per-cu-empty", BIG, 1, 49_152, {"RP_SIM_PC32_PER_CU": ""}, dict(kernel="pc<3,2>")),
    ("auto-sharded-pc32", BIG, 3, 40_000, {}, dict(kernel="pc<3,2>", sort=1, radix=1, key=1, pass1=1)),
    ("size-edge-below", 64 * CUS, 1, None, {}, dict(kernel="pc<7>", twins=0, list=0)),
    ("size-edge-above", 64 * CUS + 1, 1, 64 * CUS + 1, {}, dict(kernel="pc<3,2>", twins=1, list=1)),  # 257 <= 768
    ("twins-off-large", BIG, 1, None, {"RP_SIM_TWINS": "0"},
     dict(kernel="lanes", twins=0, list=0, sort=0, pass1=0)),
    ("lanes", 900, 1, 700, {"RP_SIM_CK": "lanes"},
     dict(kernel="lanes", twins=1, list=1, sort=1, radix=1, key=1, pass1=0)),
    ("lanes-one-dirty", 900, 1, 1, {"RP_SIM_CK": "lanes"}, dict(kernel="lanes", sort=1, radix=0)),
    ("lanes-two-dirty", 900, 1, 2, {"RP_SIM_CK": "lanes"}, dict(kernel="lanes", sort=1, radix=1)),
    ("lanes-sort1", 900, 1, 700, {"RP_SIM_CK": "lanes", "RP_SIM_CK_SORT": "1"},
     dict(kernel="lanes", sort=1, key=0, pass1=1)),
    ("lanes-sort0", 900, 1, None, {"RP_SIM_CK": "lanes", "RP_SIM_CK_SORT": "0"},
     dict(kernel="lanes", twins=1, list=1, sort=0, pass1=0)),
    ("lanes-twins0", 900, 1, None, {"RP_SIM_CK": "lanes", "RP_SIM_TWINS": "0"},
     dict(kernel="lanes", twins=0, list=0, sort=0)),
    ("lanes-pass1", 900, 1, 700, {"RP_SIM_CK": "lanes", "RP_SIM_PASS1": "1"}, dict(kernel="lanes", pass1=1)),
    ("pc", 900, 1, None, {"RP_SIM_CK": "pc"}, dict(kernel="pc<7>", twins=0, list=0, sort=0, pass1=1)),
    ("pc-large", BIG, 1, None, {"RP_SIM_CK": "pc"}, dict(kernel="pc<7>", twins=0, list=0, sort=0, pass1=1)),
    ("pc3", 900, 1, None, {"RP_SIM_CK": "pc3"}, dict(kernel="pc<3>", twins=0, pass1=1)),
    ("pc32", 900, 1, None, {"RP_SIM_CK": "pc32"}, dict(kernel="pc<3,2>", twins=0, list=0, sort=0)),
    ("pc32-twins-sortpc", 900, 1, 700, {"RP_SIM_CK": "pc32", "RP_SIM_TWINS": "1", "RP_SIM_CK_SORT_PC": "1"},
     dict(kernel="pc<3,2>", twins=1, list=1, sort=1, key=1, pass1=1)),
    ("unknown", 900, 1, None, {"RP_SIM_CK": "foo"}, dict(kernel="pc<7>", twins=0, list=0)),
    ("ck-empty", 900, 1, None, {"RP_SIM_CK": ""}, dict(kernel="pc<7>", twins=0, list=0)),
    ("pair", 900, 1, None, {"RP_SIM_CK": "pair"}, dict(kernel="pair<6,2,32>", twins=0, sort=0, pass1=0)),
    ("pair-pass1", 900, 1, None, {"RP_SIM_CK": "pair", "RP_SIM_PASS1": "1"},
     dict(kernel="pair<6,2,32>", sort=0, pass1=0)),
    ("pair-sortpc-twins", 900, 3, None, {"RP_SIM_CK": "pair", "RP_SIM_CK_SORT_PC": "1", "RP_SIM_TWINS": "1"},
     dict(kernel="pair<6,2,32>", twins=1, list=1, sort=0, pass1=0)),
    ("pc-sortpc", 900, 1, 700, {"RP_SIM_CK": "pc", "RP_SIM_CK_SORT_PC": "1"},
     dict(kernel="pc<7>", twins=0, list=1, sort=1, key=1)),
    ("pc-sortpc-sort1", 900, 1, None, {"RP_SIM_CK": "pc", "RP_SIM_CK_SORT_PC": "1", "RP_SIM_CK_SORT": "1"},
     dict(kernel="pc<7>", list=0, sort=0)),  # the producer/consumer paths sort by vdt only
    ("sharded-sortpc0", 900, 3, None, {"RP_SIM_CK_SORT_PC": "0"}, dict(kernel="pc<7>", list=0, sort=0)),
    ("sharded-sortpc-yes", 900, 3, None, {"RP_SIM_CK_SORT_PC": "yes"}, dict(list=0, sort=0)),  # on only for '1'
    ("pc-twins", 900, 1, None, {"RP_SIM_CK": "pc", "RP_SIM_TWINS": "1"},
     dict(kernel="pc<7>", twins=1, list=1, sort=0)),
    ("pc-pass1-off", 900, 1, None, {"RP_SIM_CK": "pc", "RP_SIM_PASS1": "0"}, dict(kernel="pc<7>", pass1=0)),
    ("empty-strings", 900, 1, None, {"RP_SIM_TWINS": "", "RP_SIM_CK_SORT": ""},
     dict(kernel="pc<7>", twins=0, list=0, sort=0, key=1, pass1=1)),
    ("empty-strings-sharded", 900, 3, 500, {"RP_SIM_TWINS": "", "RP_SIM_CK_SORT": "", "RP_SIM_PASS1": ""},
     dict(kernel="pc<7>", twins=0, list=1, sort=1, key=1, pass1=1)),
    ("twins-yes", 900, 1, None, {"RP_SIM_TWINS": "yes"}, dict(twins=1, list=1)),  # anything but a leading '0'
    ("verify", 900, 1, None, {"RP_SIM_TWIN_VERIFY": "1"}, dict(verify=1, twins=0)),
    ("verify-0", 900, 1, None, {"RP_SIM_TWIN_VERIFY": "0"}, dict(verify=0)),
    ("verify-empty", 900, 1, None, {"RP_SIM_TWIN_VERIFY": ""}, dict(verify=0)),
    ("ablate", 900, 1, None, {"RP_SIM_CK_ABLATE": "2"}, dict(ablate=2, kernel="pc<7>")),
    ("ablate-unset", 900, 1, None, {}, dict(ablate=0, verify=0)),
]

D1 = [
    ("d1-default", {}, "pair<6,2,8>"),
    ("d1-vpg16", {"RP_SIM_D1_VPG": "16"}, "pair<6,2,16>"),
    ("d1-vpg4", {"RP_SIM_D1_VPG": "4"}, "pair<6,2,8>"),
    ("d1-vpg-empty", {"RP_SIM_D1_VPG": ""}, "pair<6,2,8>"),
    ("d1-pc", {"RP_SIM_D1_CK": "pc"}, "pc<7>"),
    ("d1-blockck", {"RP_SIM_D1_CK": "blockck"}, "none"),
    ("d1-blockck-flag", {"RP_SIM_D1_BLOCKCK": "1"}, "none"),
    ("d1-blockck-flag-empty", {"RP_SIM_D1_BLOCKCK": ""}, "none"),  # set at all
    ("d1-pc-beats-flag", {"RP_SIM_D1_CK": "pc", "RP_SIM_D1_BLOCKCK": "1"}, "pc<7>"),
    ("d1-other", {"RP_SIM_D1_CK": "pair"}, "pair<6,2,8>"),
]

EARLY = [("early-1", {"RP_SIM_EARLY": "1"}, 1), ("early-0", {"RP_SIM_EARLY": "0"}, 0),
         ("early-empty", {"RP_SIM_EARLY": ""}, 0), ("early-yes", {"RP_SIM_EARLY": "yes"}, 0),
         ("early-unset", {}, 0)]

ROWS = PLAN + [(i, 900, 1, None, env, dict(d1=want, kernel="pc<7>")) for i, env, want in D1] \
    + [(i, 900, 1, None, env, dict(early=want, early_kernel="pc<7>")) for i, env, want in EARLY] \
    + [("early-kernel-large", BIG, 1, None, {"RP_SIM_TWINS": "0"}, dict(early_kernel="lanes")),
       ("early-kernel-edge", 64 * CUS, 1, None, {}, dict(early_kernel="pc<7>"))]


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("sim_plan") / "sim_plan_driver")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I",
                           os.path.join(REPO, "ringpop-node_amd", "csrc"),
                           os.path.join(REPO, "tests", "sim_plan_driver.cpp"), "-o", exe])
    text = "".join("%d %d %d %d %s\n" % (NL, G, CUS, nd or 0, " ".join("%s=%s" % kv for kv in env.items()))
                   for _, NL, G, nd, env, _ in ROWS)
    out = subprocess.run([exe], input=text, capture_output=True, text=True, check=True, timeout=60).stdout
    got = [dict(f.split("=", 1) for f in line.split()) for line in out.splitlines()]
    assert len(got) == len(ROWS)
    return {row[0]: g for row, g in zip(ROWS, got)}


def test_row_ids_are_unique():
    assert len({r[0] for r in ROWS}) == len(ROWS)


@pytest.mark.parametrize("row", ROWS, ids=[r[0] for r in ROWS])
def test_sim_plan_row(lines, row):
    name, _, _, nd, _, want = row
    got = lines[name]
    assert int(got["nd_read"]) == (nd is not None), got  # the host wait: exactly where the rule uses the count
    assert {k: got[k] for k in want} == {k: str(v) for k, v in want.items()}, got
    assert int(got["sort"]) <= int(got["list"]) and int(got["radix"]) <= int(got["sort"]), got
    assert int(got["twins"]) <= int(got["list"]), got
