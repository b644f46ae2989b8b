"""The damp-scoring oracle (oracle/orc_damp.c) and the sequential damp model (tests/damp_model.py)
against the reference's own run (tests/golden/damp_golden.json and damp_hot_golden.json:
lib/membership/{index,member}.js in node, make_damp_golden.py).
CPU only. Bit-exact: every Math.pow(Math.E, y) the engine evaluated, and every member's
dampScore / lastUpdateDampScore / lastUpdateTimestamp after every op, plus the order of
'suppressLimitExceeded' events."""
import math
import struct

import numpy as np
import pytest

import golden_util as gu
from damp_model import DampModel

STATUSES = ["alive", "suspect", "faulty", "leave"]


def bits(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


@pytest.fixture(scope="module")
def golden():
    # damp_hot_golden.json: the hot-address case (one address past 1,024 changes in a batch)
    return {"cases": gu.load("damp_golden.json")["cases"] + gu.load("damp_hot_golden.json")["cases"]}


def test_pow_matches_engine_bit_for_bit(orc, golden):
    n = bad = 0
    for c in golden["cases"]:
        for o in c["out"]:
            for y, r in o["pow"]:
                n += 1
                bad += bits(orc.js_pow(math.e, y)) != bits(r)
    assert n > 5000 and bad == 0, (n, bad)


def test_js_round_half_up(orc):
    for x, want in [(0.49999999999999994, 0.0), (0.5, 1.0), (1.5, 2.0), (2.5, 3.0), (-2.5, -2.0), (-0.5, -0.0),
                    (125.49999999999999, 125.0), (125.5, 126.0), (4503599627370495.5, 4503599627370496.0)]:
        assert orc.js_round(x) == want, x


def replay(orc, case):
    """The reference's damp bookkeeping from the applied lists (tests/damp_model.py, the model the
    GPU tests compare the device with), with the oracle's arithmetic."""
    model = DampModel(orc, case["config"], local=case["local"])
    snaps, events = [], []
    for op, o in zip(case["ops"], case["out"]):
        now = op["now"]
        ev = []
        if op["type"] == "update":
            addrs = [c[0] for c in op["changes"]]
            app = np.zeros(len(addrs), np.uint8)
            app[o["applied"]] = 1
            _, flag = model.update(addrs, app, now)
            ev = [addrs[i] for i in np.flatnonzero(flag)]
        elif op["type"] == "set":
            assert not model.state
            model.set([m[0] for m in o["members"]])
        elif op["type"] == "decay":
            model.decay(now)
        snaps.append(model.snapshot())
        events.append(ev)
    return snaps, events


def test_oracle_replays_reference_damp_state(orc, golden):
    checked = 0
    for c in golden["cases"]:
        snaps, events = replay(orc, c)
        for k, (o, snap, ev) in enumerate(zip(c["out"], snaps, events)):
            want = {m[0]: (m[1], m[2], m[3] or 0) for m in o["members"]}
            assert snap == want, (c["name"], k)
            assert ev == o["suppressed"], (c["name"], k)
            checked += len(want)
    assert checked > 20000


def test_golden_covers_the_branches(golden):
    names = {c["name"] for c in golden["cases"]}
    assert {"flap", "half-life", "bootstrap", "disabled", "fractional", "min-floor"} <= names
    flap = next(c for c in golden["cases"] if c["name"] == "flap")
    assert sum(len(o["suppressed"]) for o in flap["out"]) > 0
    # x.5 products: a decay of an odd score by exactly a half-life sits on Math.round's tie
    hl = next(c for c in golden["cases"] if c["name"] == "half-life")
    assert any(m[1] == 126 for o in hl["out"] for m in o["members"]) or \
        any(m[1] == 125 for o in hl["out"] for m in o["members"])
