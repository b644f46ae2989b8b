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
            assert len(c["checksums"]) == len(c["maxPiggyback"]) == c["rounds"]
        _SIM[name] = fixture
    return _SIM[name]


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
