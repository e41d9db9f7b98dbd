"""bench.py's multi-GPU launch path on the CPU: `--gpus 2` without WORLD_SIZE starts
two rank processes itself (one per GPU on a GPU node; here gloo + the engine's CPU
build), cost-balanced shards of one universe, the snapshot broadcast and the
two-phase CSR all-gather. The gathered results must cover the same universe as a
one-rank run over all of its bindings."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# --full: the oracle parity check of the results is part of the full run only
ARGS = ["--full", "--config", "6", "--steps", "2", "--warmup", "1", "--check", "40", "--e2e-reps", "0", "--no-cpu",
        "--inflight", "2", "--lib", "karmada_amd/libkp_cpusim.so"]


def run(extra, env_extra=None, args=ARGS):
    env = dict(os.environ, KP_DIST_BACKEND="gloo", KP_CPUSIM_THREADS="2")
    env.pop("WORLD_SIZE", None)
    env.update(env_extra or {})
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args + extra, cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=300)
    return p


def line(p):
    assert p.returncode == 0, p.stderr[-2000:]
    return json.loads([x for x in p.stdout.splitlines() if x.startswith("{")][-1])


def test_bench_two_ranks_gloo():
    two = line(run(["--gpus", "2", "--bindings", "250"]))
    one = line(run(["--gpus", "1", "--bindings", "500"]))
    assert two["n_gpus"] == 2 and len(two["per_rank_ms"]) == 2
    assert two["config"]["bindings_total"] == 500 == one["config"]["bindings_total"]
    assert two["parity_bad"] == 0 and two["parity_checked"] == 80 and two["parity_lanes"] == 3
    # the all-gathered CSR covers the whole universe: same totals as one rank over all of it
    assert two["result_targets"] == one["result_targets"]
    assert two["scheduled_ok"] == one["scheduled_ok"]


def test_bench_four_ranks_gloo_config5_whole_csr():
    """Four rank processes over config 5's mix (SEL_ALL StaticWeight, Dynamic/Aggregated
    and spread constraints, interleaved), cost-balanced shards (dist.shard_range_weighted):
    every binding of the gathered CSR is re-checked against the oracle (--check covers each
    rank's whole shard), and the totals equal one rank over the same universe."""
    common = ["--config", "5", "--clusters", "300", "--check", "400", "--inflight", "1"]
    four = line(run(common + ["--gpus", "4", "--bindings", "100"], {"KP_CPUSIM_THREADS": "1"}))
    one = line(run(common + ["--gpus", "1", "--bindings", "400"]))
    assert four["n_gpus"] == 4 and len(four["per_rank_ms"]) == 4
    assert four["config"]["bindings_total"] == 400 == one["config"]["bindings_total"]
    # the shards are cut by cost, not by count, yet cover the universe: every binding checked once
    assert four["parity_checked"] == 400 and four["parity_bad"] == 0
    assert one["parity_checked"] == 400 and one["parity_bad"] == 0
    assert four["result_targets"] == one["result_targets"]
    assert four["scheduled_ok"] == one["scheduled_ok"]


def test_bench_plain_run_is_lean_and_dumps_its_outputs(tmp_path):
    """Without --full the bench times its steps and prints the headline line only; the
    arrays --dump-outputs writes are the same from run to run (same arguments, same
    inputs) and the same a --full run writes."""
    import numpy as np
    plain = [a for a in ARGS if a != "--full"]
    sizes = ["--gpus", "1", "--bindings", "250", "--steps", "3"]
    a = line(run(sizes + ["--dump-outputs", str(tmp_path / "a")], args=plain))
    b = line(run(sizes + ["--dump-outputs", str(tmp_path / "b")]))
    assert a["full"] is False and b["full"] is True
    assert a["steps"] == 3 and a["timed_window"]["timed_completions"] == 3
    assert a["ms_per_step"] > 0 and abs(a["value"] * a["ms_per_step"] * 1e-3 / 250 - 1) < 1e-2
    for k in ("metric", "unit", "higher_is_better", "dtype"):
        assert a[k] == b[k]
    for k in ("parity_checked", "kernels", "roofline", "stages_ms", "serial_value", "end_to_end_value",
              "cpu_baseline"):
        assert k not in a, k
    assert b["parity_checked"] == 40 and b["parity_bad"] == 0
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == sorted(x + ".npy" for x in a["dump_outputs"]["arrays"]) == sorted(os.listdir(tmp_path / "b"))
    for name in names:
        x, y = np.load(tmp_path / "a" / name), np.load(tmp_path / "b" / name)
        assert x.dtype in (np.float32, np.float64) and np.array_equal(x, y), name
    offs = np.load(tmp_path / "a" / "offsets.npy")
    assert len(offs) == 251 and offs[-1] == a["result_targets"] == len(np.load(tmp_path / "a" / "replicas.npy"))
    assert int((np.load(tmp_path / "a" / "status.npy") == 0).sum()) == a["scheduled_ok"]


def test_dump_outputs_sample_is_fixed_and_consistent(tmp_path, monkeypatch):
    """A result larger than the dump budget is written as a fixed sample of its bindings:
    within the budget, the same bindings every time, each with exactly its own targets."""
    import numpy as np
    sys.path.insert(0, ROOT)
    import bench
    from karmada_amd.dist import Csr
    rng = np.random.default_rng(7)
    n = 1000
    counts = rng.integers(0, 40, n)
    offs = np.concatenate(([0], np.cumsum(counts))).astype(np.int64)
    t = int(offs[-1])
    csr = Csr(rng.integers(0, 3, n).astype(np.int32), rng.integers(0, 9, n).astype(np.int32),
              rng.integers(0, 1 << 40, n).astype(np.int64), offs,
              rng.integers(0, 5000, t).astype(np.int32), rng.integers(1, 1 << 26, t).astype(np.int32))
    monkeypatch.setattr(bench, "DUMP_BUDGET", 40000)
    info = bench.dump_outputs(str(tmp_path / "a"), csr)
    bench.dump_outputs(str(tmp_path / "b"), csr, ".rank1")
    got = {k: np.load(tmp_path / "a" / f"{k}.npy") for k in info["arrays"]}
    for k, v in got.items():
        assert np.array_equal(v, np.load(tmp_path / "b" / f"{k}.rank1.npy")), k
    assert sum(v.nbytes for v in got.values()) == info["bytes"] <= 40000
    idx = got["binding_index"].astype(np.int64)
    assert 0 < len(idx) == info["bindings"] < n == info["of"] and np.all(np.diff(idx) > 0)
    assert got["err_arg"].dtype == np.float64 and got["replicas"].dtype == np.float64  # values past 2^24
    assert got["cluster_idx"].dtype == np.float32
    assert np.array_equal(got["err_arg"], csr.err_arg[idx]) and np.array_equal(got["status"], csr.status[idx])
    o = got["offsets"].astype(np.int64)
    # each kept binding with exactly its own targets, in cluster order (the engine's order
    # within a binding varies from run to run and means nothing)
    for j, i in enumerate(idx):
        want = sorted(zip(csr.cluster_idx[offs[i]:offs[i + 1]], csr.replicas[offs[i]:offs[i + 1]]))
        assert list(zip(got["cluster_idx"][o[j]:o[j + 1]], got["replicas"][o[j]:o[j + 1]])) == want
    # the same result with every binding's targets in another order: the same files
    perm = np.concatenate([offs[i] + rng.permutation(counts[i]) for i in range(n)]).astype(np.int64)
    other = Csr(csr.status, csr.err_code, csr.err_arg, offs, csr.cluster_idx[perm], csr.replicas[perm])
    bench.dump_outputs(str(tmp_path / "c"), other)
    for k, v in got.items():
        assert np.array_equal(v, np.load(tmp_path / "c" / f"{k}.npy")), k


def test_bench_gpus_must_match_world_size():
    p = run(["--gpus", "2", "--bindings", "50"], {"WORLD_SIZE": "1", "RANK": "0", "LOCAL_RANK": "0"})
    assert p.returncode != 0 and "WORLD_SIZE" in (p.stderr + p.stdout)
