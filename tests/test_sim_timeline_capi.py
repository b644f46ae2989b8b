"""CPU checks of the timeline entry points: the symbols and the minor version they came with, the
record's layout in the Python package, the null-handle refusals made before a device is touched,
and timeline_reduce / rounds_to_convergence on made-up shard parts."""
import ctypes

import numpy as np
import pytest


def test_symbols_version_and_record_layout(rpa):
    L = rpa.lib()
    assert L.rp_version() >= (1 << 16) | 7  # the minor version these entry points came with
    assert L.rp_sim_timeline_enable and L.rp_sim_timeline_read
    rec = rpa._TL_REC
    assert rec.itemsize == 128 and rpa.SIM_NEVER == 0xFFFFFFFF
    assert [rec.fields[k][1] for k in ("round", "observers", "ck_min", "ck_max", "pairs", "in_ring", "unmet",
                                       "false_faulty", "stats", "tail")] == [0, 8, 12, 16, 24, 56, 64, 72, 80, 112]


def test_null_handle_is_refused(rpa):
    L = rpa.lib()
    n, first = ctypes.c_uint32(5), ctypes.c_uint64()
    assert L.rp_sim_timeline_enable(None, 4) == -1 and b"null sim handle" in L.rp_last_error()
    assert L.rp_sim_timeline_read(None, None, 0, ctypes.byref(n), ctypes.byref(first), None) == -1
    assert n.value == 5


def _part(rounds, observers, lo, hi, unmet, first_seen):
    k = len(rounds)
    p = {"round": np.array(rounds, dtype=np.uint64), "observers": np.array(observers, dtype=np.uint32),
         "ck_min": np.array(lo, dtype=np.uint32), "ck_max": np.array(hi, dtype=np.uint32),
         "pairs": np.outer(np.array(observers, dtype=np.uint64), np.array([3, 0, 1, 0], dtype=np.uint64)),
         "in_ring": np.array(observers, dtype=np.uint64) * np.uint64(3), "unmet": np.array(unmet, dtype=np.uint64),
         "false_faulty": np.zeros(k, dtype=np.uint64), "stats": np.ones((k, 4), dtype=np.uint64),
         "first_seen": np.array(first_seen, dtype=np.uint32)}
    return p


def test_timeline_reduce_and_rounds_to_convergence(rpa):
    never = rpa.SIM_NEVER
    a = _part([4, 5, 6], [2, 2, 2], [9, 7, 7], [9, 7, 7], [1, 1, 0], [[never, 5, never], [4, never, never]])
    b = _part([4, 5, 6], [1, 1, 0], [9, 8, never], [9, 8, 0], [0, 0, 0], [[3, never, never], [never, never, never]])
    r = rpa.timeline_reduce([a, b])
    assert r["round"].tolist() == [4, 5, 6] and r["observers"].tolist() == [3, 3, 2] and r["observers"].dtype == np.uint32
    assert r["ck_min"].tolist() == [9, 7, 7] and r["ck_max"].tolist() == [9, 8, 7]
    assert r["pairs"].tolist() == [[9, 0, 3, 0], [9, 0, 3, 0], [6, 0, 2, 0]] and r["pairs"].dtype == np.uint64
    assert r["unmet"].tolist() == [1, 1, 0] and r["stats"].tolist() == [[2] * 4] * 3
    assert r["first_seen"].tolist() == [[3, 5, never], [4, never, never]] and r["first_seen"].dtype == np.uint32
    # round 4: one checksum but a want unmet; round 5: two checksums; round 6: converged (the shard
    # with no observer left its range empty)
    assert r["converged"].tolist() == [False, False, True]
    assert rpa.rounds_to_convergence(r) == 6
    r["converged"][:] = False
    assert rpa.rounds_to_convergence(r) is None
    nobody = rpa.timeline_reduce([_part([0], [0], [never], [0], [0], [[never] * 3])])
    assert nobody["converged"].tolist() == [True] and rpa.rounds_to_convergence(nobody) == 0
    late = _part([5, 6, 7], [1, 1, 1], [9, 9, 9], [9, 9, 9], [0, 0, 0], [[never] * 3] * 2)
    with pytest.raises(ValueError, match="different rounds"):
        rpa.timeline_reduce([a, late])
    with pytest.raises(ValueError, match="different rounds"):
        rpa.timeline_reduce([a, {k: v[:2] if k != "first_seen" else v for k, v in b.items()}])
