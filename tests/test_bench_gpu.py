"""bench.py's launch contract on the GPU box: `python bench.py --gpus 2` (no torchrun) starts two
rank processes itself, the C5-path simulator is sharded over them (DistGossipSim: message
exchange by all-to-all-v; gloo here because both ranks share the box's one GPU — the driver's
8-GPU node runs the same code over RCCL), and rank 0 prints ONE JSON line reporting n_gpus = 2
with every rank's keys counted."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(gpus, extra, env_extra=None):
    env = dict(os.environ, **(env_extra or {}))
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", str(gpus)] + extra,
                       env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


SMALL = ["--full", "--steps", "2", "--warmup", "1", "--batch-log2", "18", "--no-merge", "--no-wire", "--no-cpu",
         "--sim-n", "0", "--sim5-n", "3000"]


def test_bench_two_ranks_spawned(gpu):
    out = _bench(2, SMALL, {"RP_BENCH_BACKEND": "gloo"})
    assert out["n_gpus"] == 2
    assert out["config"]["total_keys"] == 2 * 2 * (1 << 18)
    assert out["sim_c5"]["n_gpus"] == 2 and out["sim_c5"]["converged"]
    assert out["sim_c5"]["exchange_bytes_per_round_rank0"] > 0
    for k in ("metric", "value", "unit", "roofline", "ms_per_step", "scaling"):
        assert k in out


def test_bench_one_gpu_schema(gpu):
    out = _bench(1, SMALL)
    assert out["n_gpus"] == 1 and out["roofline"]["frac"] > 0
    assert out["sim_c5"]["round_ms"]["max"] >= out["sim_c5"]["round_ms"]["p50"]
    assert out["sim_c5"]["traffic"]["records"] > 0


def test_bench_four_ranks_spawned_with_merge(gpu):
    """`bench.py --gpus 4`: four ranks (gloo; they share the box's GPU), the C5-path simulator
    sharded four ways, the C3 merge as four replicas with batch-strided checksums
    (DistMembership) and the fold partitioned by member id (PartMembership); rank 0 reports
    n_gpus = 4 for each."""
    small = [x for x in SMALL if x != "--no-merge"] + ["--part-log2", "16"]
    out = _bench(4, small, {"RP_BENCH_BACKEND": "gloo"})
    assert out["n_gpus"] == 4
    assert out["config"]["total_keys"] == 4 * 2 * (1 << 18)
    assert out["sim_c5"]["n_gpus"] == 4 and out["sim_c5"]["converged"]
    assert out["merge"]["n_gpus"] == 4 and out["merge"]["updates_per_s"] > 0
    assert isinstance(out["merge"]["checksum"], int)
    # the id-partitioned fold (PartMembership) at 2^16 members / updates, four ways
    fp = out["merge"]["fold_large_partitioned"]
    assert fp["n_gpus"] == 4 and fp["members"] == 1 << 16 and fp["ms_per_batch"] > 0
    # the exchange's host and device time per round, shown with -rP
    print("sim_c5 exchange:", json.dumps({k: v for k, v in out["sim_c5"].items()
                                          if k.startswith("exchange") or k in ("rounds", "round_ms")}))


def test_bench_plain_run_is_lean_and_dumps_outputs(gpu, orc, tmp_path):
    """Without --full the line holds the headline figure alone (no leg beside the timed steps),
    --steps sets the timed steps, and --dump-outputs writes the last timed step's owners: with
    --steps 3 that step read key buffer 2 (keys 2 * 2^18 ...), checked here against the oracle
    by server name."""
    import numpy as np

    n, servers = 1 << 18, 500
    out = _bench(1, ["--steps", "3", "--warmup", "1", "--batch-log2", "18", "--servers", str(servers),
                     "--dump-outputs", str(tmp_path / "dump")])
    assert out["steps"] == 3 and out["config"]["total_keys"] == 3 * n
    assert out["ms_per_step"] > 0 and out["value"] == pytest.approx(n / (out["ms_per_step"] * 1e-3))
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "roofline"):
        assert k in out
    for k in ("merge", "sim", "sim_c5", "wire", "api_latency", "cpu_baseline"):
        assert k not in out
    assert sorted(p.name for p in (tmp_path / "dump").iterdir()) == ["owners.npy", "owners_index.npy"]
    got = np.load(tmp_path / "dump" / "owners.npy")
    idx = np.load(tmp_path / "dump" / "owners_index.npy")
    assert got.dtype == np.float64 and got.shape == (n, 3)
    assert idx.dtype == np.float64 and np.array_equal(idx, np.arange(n))
    names = [orc.c2_addr(i) for i in range(servers)]
    ring = gpu.HashRing(device=0)
    ring.addRemoveServers(names)
    oracle = orc.Ring(100)
    oracle.add_remove(names)
    want, _ = oracle.lookupn_keys(orc.uuid_keys(42, 2 * n, n), 3)
    gname = np.array([ring.name(i) for i in range(servers)])
    wname = np.array([oracle.name(i) for i in range(servers)])
    assert np.array_equal(gname[got.astype(np.int64)], wname[np.asarray(want).astype(np.int64)])


def test_bench_dump_sample_is_fixed():
    """The sample --dump-outputs keeps of a full-size step: both ends, 2^20 drawn keys, the same
    on every call, under 64 MB as float64 owners plus indices."""
    import importlib.util

    import numpy as np
    spec = importlib.util.spec_from_file_location("rp_bench", os.path.join(REPO, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    n = 1 << 26
    a, b = bench.dump_sample_index(n), bench.dump_sample_index(n)
    assert np.array_equal(a, b) and a[0] == 0 and a[-1] == n - 1 and a.min() >= 0 and a.max() < n
    assert np.array_equal(a[:4096], np.arange(4096)) and np.all(np.diff(a) >= 0)
    assert len(a) * (3 + 1) * 8 <= 64 << 20
    assert np.array_equal(bench.dump_sample_index(1000), np.arange(1000))
