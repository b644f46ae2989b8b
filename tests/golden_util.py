"""Helpers to replay tests/golden/*.json fixtures (data produced by the reference JS)."""
import json
import os

import pyoracle

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load(name):
    with open(os.path.join(GOLDEN, name)) as f:
        return json.load(f)


_SIM = {}


def load_sim(name):
    """A simulator fixture (sim_golden.json, sim_tiny_golden.json) with every case in the schema
    of sim_golden.json: rows stored as runs ([[count, row], ...]: checksumRuns, maxPiggybackRuns)
    are expanded to one row per round. Parsed once per process; callers do not modify it."""
    if name not in _SIM:
        fixture = load(name)
        for c in fixture["cases"]:
            for key, packed in (("checksums", "checksumRuns"), ("maxPiggyback", "maxPiggybackRuns")):
                if packed in c:
                    c[key] = [row for count, row in c.pop(packed) for _ in range(count)]
            if "checksums" in c or "ringRuns" not in c:  # (a ring case may name its source fixture instead)
                assert len(c["checksums"]) == len(c["maxPiggyback"]) == c["rounds"]
        _SIM[name] = fixture
    return _SIM[name]


_RING = {}


def load_sim_ring():
    """sim_ring_golden.json by case name, every case in the schema of its source fixture (a tiny or
    net case takes its inputs and checksums from sim_tiny_golden.json / sim_net_golden.json, a flap
    case holds its own), plus rings = uint8[rounds][n][n]: rings[r][v][i] = 1 when the reference
    ring of node v held node i after round r. Parsed once per process; callers do not modify it."""
    if not _RING:
        import numpy as np

        import sim_net_cases
        src = {"tiny": {c["name"]: c for c in load_sim("sim_tiny_golden.json")["cases"]}, "net": sim_net_cases.load()}
        for f in load_sim("sim_ring_golden.json")["cases"]:
            c = dict(src[f["source"]][f["name"]], source=f["source"]) if f["source"] in src else dict(f)
            assert (c["n"], c["rounds"]) == (f["n"], f["rounds"]), f["name"]
            rows = [row for count, row in f["ringRuns"] for _ in range(count)]
            assert len(rows) == c["rounds"] and all(len(row) == c["n"] for row in rows), f["name"]
            bits = np.array([[[int(m, 16) >> i & 1 for i in range(c["n"])] for m in row] for row in rows],
                            dtype=np.uint8)
            assert all(int(m, 16) >> c["n"] == 0 for row in rows for m in row), f["name"]
            c.pop("ringRuns", None)
            c["rings"] = bits
            _RING[c["name"]] = c
    return _RING


def hash_func(case):
    """The hashFunc the generator injected (tests/golden/ref_ring.js makeHash)."""
    kind = case["hashKind"]
    if kind == "farmhash":
        return None
    if kind == "port":
        return lambda s: int(s[s.rfind(":") + 1:])
    mod = case["hashMod"]
    return lambda s: int(s[1:]) if s.startswith("#") else pyoracle.hash32(s) % mod


def keys_of(batch):
    keys = batch["keys"]
    if isinstance(keys, dict):
        seed, k0, n = keys["uuid"]
        return [k.tobytes().decode() for k in pyoracle.uuid_keys(seed, k0, n)]
    return keys
