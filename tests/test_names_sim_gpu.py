"""GPU tests of the gossip simulator's view checksums and ring checksums over names of 1..240
bytes (name_cases.sim_case; tests/test_name_cases.py counts, from the CPU oracle's run alone, the
deviated pieces that do not fit a piece record's 8-bit fields):

  tiny-65          pieces of 8..10 bytes, several deviated ones in one 20-byte chunk; a refuted
                   piece grows by 12 digits
  ragged-130       every name length 1..70
  host-shrink-*    base pieces of 244..262 bytes; the revived node's own piece shrinks by 12 digits
                   to at most 255 bytes while its base piece is longer, and suspect / faulty pieces
                   pass 255 bytes (so these views fall back for those already)
  host-grow-*      the same names with one-digit incarnations: only the view's piece passes 255
  host-band-65     one 240-byte node that is never down joins afresh: its own view holds its piece
                   at 250 bytes over a base piece of 262 and no piece past 255, in a run without
                   any piece past 255, so that view reaches the fallback only through the test of
                   the base length (per view in pass 1, per wave in the lane kernel)

After every round: every node's checksum against the oracle simulator's; every live node's
checksum against the oracle hash of the string rebuilt in Python from the device's own view rows
(independent of the oracle simulator); every node's ring checksum, twin classes on and off,
against tests/proxy_model.py over the oracle's ring rows. On every chain kernel, with and without
the twin pass, on the three D1 checksum kernels, and once in three shards. Exact."""
import numpy as np
import pytest

import name_cases as nc
import proxy_model as pm

pytestmark = pytest.mark.gpu


def _sim(gpu, case, shards=None):
    args = (case["names"], case["inc0"], np.array(case["dead"], dtype=np.uint8))
    kw = dict(seed=case["seed"], suspicion_rounds=nc.SIM_SUSP, now0=case["now0"], events=case["events"])
    return gpu.ShardedGossipSim(*args, shards, **kw) if shards else gpu.GossipSim(*args, **kw)


def _ring_checksums(sim, monkeypatch):
    monkeypatch.delenv("RP_SIM_RCK_TWINS", raising=False)
    on = sim.ring_checksums()
    monkeypatch.setenv("RP_SIM_RCK_TWINS", "0")
    off = sim.ring_checksums()
    monkeypatch.delenv("RP_SIM_RCK_TWINS", raising=False)
    return on, off


def _run(gpu, orc, case_name, monkeypatch, rings=False, views=True, shards=None):
    run = nc.sim_oracle_run(orc, case_name)
    case = run["case"]
    names, n = case["names"], len(case["names"])
    sim = _sim(gpu, case, shards)
    cache = {}
    for r in range(case["rounds"]):
        sim.step()
        got = sim.checksums()
        if views:
            for v in range(n):
                if run["up"][r][v]:
                    st, inc = sim.view(v)
                    assert int(got[v]) == orc.hash32(nc.view_string(names, run["order"], st, inc)), (case_name, r, v)
        assert got.tolist() == run["ck"][r].tolist(), (case_name, r)
        if rings:
            want = pm.ring_checksums(names, run["ring"][r], cache)
            on, off = _ring_checksums(sim, monkeypatch)
            assert np.array_equal(on, want), (case_name, r, "twins on")
            assert np.array_equal(off, want), (case_name, r, "twins off")
    sim.close()


@pytest.mark.parametrize("case_name", nc.SIM_CASES)
def test_names_sim_default_path(gpu, orc, monkeypatch, case_name):
    """The default refresh: view checksums, the strings rebuilt from the device's view rows, and
    the ring checksums with the twin classes on and off."""
    _run(gpu, orc, case_name, monkeypatch, rings=True)


CHAIN_CASES = ["tiny-65", "ragged-130", "host-shrink-65", "host-grow-65", "host-band-65"]


@pytest.mark.parametrize("twins", ["0", "1"])
@pytest.mark.parametrize("ck", ["lanes", "pc", "pc3", "pc32", "pair"])
@pytest.mark.parametrize("case_name", CHAIN_CASES)
def test_names_sim_chain_kernels(gpu, orc, monkeypatch, case_name, ck, twins):
    """Every refresh chain kernel (RP_SIM_CK), without and with the twin pass (its fingerprints
    verified): the pieces past a record's fields must take each kernel's general fallback."""
    monkeypatch.setenv("RP_SIM_CK", ck)
    monkeypatch.setenv("RP_SIM_TWINS", twins)
    if twins == "1":
        monkeypatch.setenv("RP_SIM_TWIN_VERIFY", "1")
    _run(gpu, orc, case_name, monkeypatch)


@pytest.mark.parametrize("pass1", ["0", "1"])
@pytest.mark.parametrize("ck", ["lanes", "pc32"])
@pytest.mark.parametrize("case_name", ["host-shrink-65", "host-grow-65", "host-band-65"])
def test_names_sim_both_pass1_forms(gpu, orc, monkeypatch, case_name, ck, pass1):
    """The per-lane and the per-segment pass 1 (RP_SIM_PASS1) both send an oversize piece to the
    fallback."""
    monkeypatch.setenv("RP_SIM_CK", ck)
    monkeypatch.setenv("RP_SIM_PASS1", pass1)
    _run(gpu, orc, case_name, monkeypatch, views=False)


@pytest.mark.parametrize("d1ck", [None, "pc", "blockck"])
@pytest.mark.parametrize("case_name", ["tiny-65", "host-shrink-130", "host-grow-130", "host-band-65"])
def test_names_sim_d1_checksum_kernels(gpu, orc, monkeypatch, case_name, d1ck):
    """The D1 senders' checksum kernels (RP_SIM_D1_CK): the default, the producer / consumer
    kernel and the block chain."""
    if d1ck:
        monkeypatch.setenv("RP_SIM_D1_CK", d1ck)
    _run(gpu, orc, case_name, monkeypatch, views=False)


@pytest.mark.parametrize("case_name", ["host-shrink-130", "host-band-65"])
def test_names_sim_sharded(gpu, orc, monkeypatch, case_name):
    """Three shards of the 130-node shrinking case and of the band case (its join crosses shards):
    checksums only."""
    _run(gpu, orc, case_name, monkeypatch, views=False, shards=3)
