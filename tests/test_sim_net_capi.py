"""CPU checks of the partition entry points: the symbols and the minor version they came with, the
event packing of the Python package, the validation rp_sim_create_scenario makes before it touches a
device, and side_summary_reduce on made-up shard parts."""
import numpy as np
import pytest


def test_symbols_and_version(rpa):
    L = rpa.lib()
    assert L.rp_version() >= (1 << 16) | 6  # the minor version these entry points came with
    assert L.rp_sim_sides and L.rp_sim_side_summary
    assert rpa.SIM_EVENT == {"kill": 0, "revive": 1, "leave": 2, "join": 3, "side": 4, "heal": 5}


def test_events_take_triples_and_an_argument(rpa):
    ev, n = rpa._events([(3, "kill", 1), [4, "side", 2, 7], (5, "heal", 0), (6, 1, 2, 9)])
    assert n == 4 and ev.dtype == np.uint32
    assert ev.tolist() == [[3, 0, 1, 0], [4, 4, 2, 7], [5, 5, 0, 0], [6, 1, 2, 9]]
    assert rpa._events([])[1] == 0


@pytest.mark.parametrize("events", [[(0, 6, 0)], [(0, "side", 1, 256)], [(0, "heal", 4)], [(0, "side", 4, 1)]],
                         ids=["kind-6", "side-256", "heal-node-n", "side-node-n"])
def test_bad_events_are_refused_before_any_device_is_used(rpa, events):
    names = ["10.0.0.%d:3000" % i for i in range(4)]
    with pytest.raises(rpa.RingpopAmdError, match="bad event"):
        rpa.GossipSim(names, np.ones(4, dtype=np.int64), np.zeros(4, dtype=np.uint8), events=events)


def test_side_summary_reduce(rpa):
    def part(nodes, lo, hi, cross):
        p = {"nodes": np.zeros(256, dtype=np.uint32), "ck_min": np.full(256, 0xFFFFFFFF, dtype=np.uint32),
             "ck_max": np.zeros(256, dtype=np.uint32), "cross_pingable": np.zeros(256, dtype=np.uint64)}
        for s in nodes:
            p["nodes"][s], p["ck_min"][s], p["ck_max"][s], p["cross_pingable"][s] = nodes[s], lo[s], hi[s], cross[s]
        return p

    empty = part({}, {}, {}, {})
    a = part({0: 2, 255: 1}, {0: 10, 255: 7}, {0: 10, 255: 7}, {0: 0, 255: 3})
    b = part({0: 1, 3: 4}, {0: 10, 3: 5}, {0: 10, 3: 6}, {0: 0, 3: 0})
    r = rpa.side_summary_reduce([empty, a, b, empty])
    assert r["nodes"][[0, 3, 255, 1]].tolist() == [3, 4, 1, 0] and r["nodes"].dtype == np.uint32
    assert r["ck_min"][[0, 3, 255, 1]].tolist() == [10, 5, 7, 0xFFFFFFFF]
    assert r["ck_max"][[0, 3, 255, 1]].tolist() == [10, 6, 7, 0]
    assert r["cross_pingable"][[0, 3, 255]].tolist() == [0, 0, 3] and r["cross_pingable"].dtype == np.uint64
    # settled: one checksum and nothing pingable across; an empty side is not
    assert r["settled"][[0, 3, 255, 1]].tolist() == [True, False, False, False]
    c = part({0: 1}, {0: 11}, {0: 11}, {0: 0})
    assert not rpa.side_summary_reduce([a, c])["settled"][0]
