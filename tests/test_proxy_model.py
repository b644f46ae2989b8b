"""Pins tests/proxy_model.py without a device. ring_checksum against the reference's own
computeChecksum values (the `checksum` the reference ring reported after every batch of the
farmhash cases of tests/golden/ring_golden.json, over the servers it then held), against the CPU
oracle ring built from the same set, and on hand-made sets."""
import numpy as np
import pytest

import golden_util as gu
import proxy_model as pm

FARMHASH_CASES = [c for c in gu.load("ring_golden.json")["cases"] if c["hashKind"] == "farmhash"]


@pytest.mark.parametrize("case", FARMHASH_CASES, ids=[c["name"] for c in FARMHASH_CASES])
def test_ring_checksum_equals_the_reference_ring(orc, case):
    """After every batch: the model over (all names ever seen, a row marking the servers the
    reference ring holds), in an order that is not the sorted one, equals the reference's checksum
    and the oracle ring's after add_remove(add=that set)."""
    pool = sorted({s for b in case["batches"] for s in b["servers"]}, reverse=True)
    assert pool and pool != sorted(pool) or len(pool) == 1
    for i, b in enumerate(case["batches"]):
        held = set(b["servers"])
        row = np.array([s in held for s in pool], dtype=np.uint8)
        got = pm.ring_checksum(pool, row)
        assert got == b["checksum"], (case["name"], i)
        ring = orc.Ring(case["replicaPoints"])
        ring.add_remove(add=sorted(held))
        assert got == ring.checksum, (case["name"], i)


def test_ring_checksum_by_hand(orc):
    """The string is the held names sorted as bytes and joined by ';', with no trailing separator;
    nobody held hashes the empty string."""
    names = ["10.0.0.2:3000", "10.0.0.10:3000", "10.0.0.1:3001", "10.0.0.1:3000"]
    assert pm.ring_checksum(names, [1, 1, 1, 1]) == orc.hash32("10.0.0.10:3000;10.0.0.1:3000;10.0.0.1:3001;10.0.0.2:3000")
    assert pm.ring_checksum(names, [1, 0, 0, 1]) == orc.hash32("10.0.0.1:3000;10.0.0.2:3000")
    assert pm.ring_checksum(names, [0, 0, 1, 0]) == orc.hash32("10.0.0.1:3001")
    assert pm.ring_checksum(names, [0, 0, 0, 0]) == orc.hash32("") == pm.EMPTY_RING
    rows = np.array([[1, 1, 1, 1], [1, 0, 0, 1], [1, 1, 1, 1], [0, 0, 0, 0]], dtype=np.uint8)
    got = pm.ring_checksums(names, rows)
    assert got.dtype == np.uint32 and got.tolist() == [pm.ring_checksum(names, r) for r in rows]
    assert got[0] == got[2] != got[1] and got[3] == pm.EMPTY_RING
