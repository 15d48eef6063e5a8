"""bench.py --gpus N: one command starts N ranks (the reference's benchmark starts one
worker per GPU itself, benchmarks/python_e2e/main.py:72-79).

CPU: the dispatch logic (child launch when WORLD_SIZE is unset, the WORLD_SIZE /
--gpus consistency check, the torch.distributed.run command line).
GPU: a real 4-rank run from one command on the single test GPU over the
torch.distributed callbacks (RCCL refuses two ranks per GPU), small scales, with the
--full legs; a plain one-GPU run (headline only) and its --dump-outputs files.
"""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    sys.path.insert(0, ROOT)
    import bench
    return bench


def test_gpus_n_starts_child_launcher(monkeypatch):
    bench = _bench()
    seen = {}

    def fake(n, argv):
        seen["n"], seen["argv"] = n, list(argv)
        return 7

    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.setattr(bench, "launch_ranks", fake)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "4", "--steps", "3"])
    with pytest.raises(SystemExit) as e:
        bench.main()
    assert e.value.code == 7
    assert seen == {"n": 4, "argv": ["--gpus", "4", "--steps", "3"]}


def test_world_size_must_match_gpus(monkeypatch):
    bench = _bench()
    monkeypatch.setenv("WORLD_SIZE", "2")
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "4"])
    with pytest.raises(SystemExit) as e:
        bench.main()
    assert "WORLD_SIZE=2" in str(e.value.code)


def test_launch_command_line():
    bench = _bench()
    cmd = bench.launch_command(8, ["--gpus", "8", "--steps", "2"], 29555)
    assert cmd[:3] == [sys.executable, "-m", "torch.distributed.run"]
    assert "--nproc-per-node=8" in cmd and "--nnodes=1" in cmd
    i = cmd.index("--master-addr")
    assert cmd[i + 1] == "127.0.0.1" and cmd[cmd.index("--master-port") + 1] == "29555"
    assert cmd[-4:] == ["--gpus", "8", "--steps", "2"]
    assert cmd[cmd.index("--master-port") + 2].endswith("bench.py")


@pytest.mark.gpu
def test_bench_gpus4_one_command_rehearsal():
    env = dict(os.environ)
    env.pop("WORLD_SIZE", None)
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "4", "--comm", "torch", "--scale", "17",
           "--bfs-scale", "15", "--bfs-roots", "2", "--louvain-scale", "12", "--full", "--no-secondary",
           "--no-traffic", "--no-cpu-baseline", "--steps", "2", "--warmup", "1"]
    r = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=240)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    lines = [x for x in r.stdout.decode().splitlines() if x.startswith("{")]
    assert len(lines) == 1, r.stdout.decode()[-2000:]
    out = json.loads(lines[0])
    assert out["n_gpus"] == 4
    assert out["config"]["parallelism"].startswith("mg4: 2D ")
    assert out["value"] > 0
    assert out["bfs"]["n_gpus"] == 4 and out["bfs"]["mteps_harmonic_mean"] > 0
    assert out["louvain"]["n_gpus"] == 4 and out["louvain"]["modularity"] > 0


@pytest.mark.gpu
def test_bench_plain_run_is_lean_and_dumps_outputs(tmp_path):
    """A plain run times the headline only (none of the --full legs on the line) and
    --dump-outputs writes the last timed step's (vertices, pageranks): every id of the
    RMAT-10 id space, float64 ids and float32 ranks that sum to 1."""
    import numpy as np
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--scale", "10", "--steps", "3",
           "--warmup", "1", "--dump-outputs", str(tmp_path / "out")]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    lines = [x for x in r.stdout.decode().splitlines() if x.startswith("{")]
    assert len(lines) == 1, r.stdout.decode()[-2000:]
    out = json.loads(lines[0])
    assert out["steps"] == 3 and len(out["config"]) and out["ms_per_step"] > 0 and out["value"] > 0
    assert out["unit"] == "edges/s" and out["dtype"] == "f32" and out["higher_is_better"] is True
    for leg in ("cpu_baseline", "bfs", "sssp", "louvain", "louvain_rmat26", "pagerank_rmat22", "pagerank_rmat26"):
        assert leg not in out, leg
    assert "copy_ceiling_gbs" not in out["roofline"] and out["roofline"]["traffic"] is None
    v = np.load(tmp_path / "out" / "vertices.npy")
    x = np.load(tmp_path / "out" / "pagerank.npy")
    assert v.dtype == np.float64 and x.dtype == np.float32
    assert np.array_equal(v, np.arange(1 << 10)) and x.shape == v.shape
    assert np.count_nonzero(x) == out["config"]["vertices"]
    # ranks sum to 1 up to fp32 rounding of ~1000 terms (6e-8 each, relative) and the 1e-6 stopping rule
    assert abs(float(x.astype(np.float64).sum()) - 1.0) < 1e-4


@pytest.mark.gpu
def test_dump_outputs_sample_is_fixed_and_indexed_by_vertex(tmp_path, monkeypatch):
    """Above DUMP_SAMPLE ids the dump is a seeded sample: the same ids on every call,
    each with the rank of that external id (0 for an id the graph does not hold),
    whatever order the result lists the vertices in."""
    import argparse
    import numpy as np
    import torch
    bench = _bench()
    monkeypatch.setattr(bench, "DUMP_SAMPLE", 100)
    args = argparse.Namespace(scale=10, world=1, rank=0)
    rng = np.random.default_rng(5)
    held = np.sort(rng.choice(1 << 10, size=700, replace=False))
    rank_of = np.zeros(1 << 10, np.float32)
    rank_of[held] = rng.random(700, dtype=np.float32) + 0.5
    dumps = []
    for k, order in enumerate((held, held[::-1].copy())):
        res = (torch.as_tensor(order.astype(np.int32), device="cuda"), torch.as_tensor(rank_of[order], device="cuda"))
        bench.dump_outputs(args, res, str(tmp_path / str(k)))
        dumps.append((np.load(tmp_path / str(k) / "vertices.npy"), np.load(tmp_path / str(k) / "pagerank.npy")))
    (v0, x0), (v1, x1) = dumps
    assert v0.dtype == np.float64 and x0.dtype == np.float32 and v0.shape == x0.shape == (100,)
    assert np.all(np.diff(v0) > 0) and v0[0] >= 0 and v0[-1] < 1 << 10
    assert np.array_equal(v0, v1) and np.array_equal(x0, x1)
    assert np.array_equal(x0, rank_of[v0.astype(np.int64)])
