"""bench.py contract: runs end-to-end (CPU, tiny config) and prints one
valid JSON line with the required fields."""
import json
import os
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from conftest import free_port

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_json_contract():
    out = subprocess.run(
        [sys.executable, "bench.py", "--model", "vgg16", "--batch-size", "2",
         "--steps", "2", "--warmup", "1", "--density", "0.05",
         "--full", "--dense-baseline-steps", "1"],
        cwd=REPO, capture_output=True, text=True, timeout=300,
    )
    assert out.returncode == 0, out.stderr[-2000:]
    line = out.stdout.strip().splitlines()[-1]
    d = json.loads(line)
    for field in ("metric", "value", "unit", "n_gpus", "steps", "warmup",
                  "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
                  "dtype", "data", "config"):
        assert field in d, field
    assert d["n_gpus"] == 1 and d["steps"] == 2 and d["data"] == "synthetic"
    assert d["value"] > 0
    assert d["config"]["compressor"] == "oktopk"
    assert d["config"]["speedup_vs_dense"] is not None


def test_bench_world2_torchrun():
    """The driver's multi-GPU invocation shape: torch.distributed.run with
    --nproc-per-node 2 (gloo on CPU here; RCCL on the GPU box).  Rank 0
    prints the one JSON line; value aggregates over the world."""
    env = dict(os.environ, OKTOPK_BACKEND="gloo")
    out = subprocess.run(
        [sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
         "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
         "--master-port", str(free_port()), "bench.py", "--gpus", "2", "--model",
         "vgg16", "--batch-size", "2", "--steps", "2", "--warmup", "1",
         "--density", "0.05", "--full", "--dense-baseline-steps", "1"],
        cwd=REPO, capture_output=True, text=True, timeout=600,
    )
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.strip().splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2
    assert d["config"]["parallelism"] == "dp2"
    assert d["config"]["global_batch"] == 4


def test_bench_dense_compressor_json():
    """--compressor dense: no dense arm, speedup null, allreduce phase only."""
    out = subprocess.run(
        [sys.executable, "bench.py", "--model", "vgg16", "--batch-size", "2",
         "--steps", "2", "--warmup", "1", "--compressor", "dense"],
        cwd=REPO, capture_output=True, text=True, timeout=300,
    )
    assert out.returncode == 0, out.stderr[-2000:]
    d = json.loads(out.stdout.strip().splitlines()[-1])
    assert d["config"]["compressor"] == "dense"
    assert d["config"]["speedup_vs_dense"] is None
    assert d["config"]["dense_ms_per_step"] is None


def _plain_run(dump_dir):
    # pinned to the CPU fp32 path even where a GPU is present: the run-to-run
    # tolerance below is argued for that path
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES="")
    out = subprocess.run(
        [sys.executable, "bench.py", "--gpus", "1", "--model", "mnistnet",
         "--batch-size", "4", "--steps", "3", "--warmup", "1", "--density",
         "0.05", "--dump-outputs", dump_dir],
        cwd=REPO, env=env, capture_output=True, text=True, timeout=300,
    )
    assert out.returncode == 0, out.stderr[-2000:]
    return json.loads(out.stdout.strip().splitlines()[-1])


def test_bench_plain_run_is_lean_and_dumps_outputs(tmp_path):
    """Without --full there is no dense arm; --dump-outputs writes the last
    timed step's loss/params/grads as float32 .npy, and a second run with the
    same arguments starts from the same inputs, so it writes the same."""
    import numpy as np

    a_dir, b_dir = str(tmp_path / "a"), str(tmp_path / "b")
    d = _plain_run(a_dir)
    assert d["steps"] == 3 and d["ms_per_step"] > 0 and d["dtype"] == "fp32"
    assert d["config"]["speedup_vs_dense"] is None
    assert d["config"]["dense_ms_per_step"] is None
    _plain_run(b_dir)
    assert sorted(os.listdir(a_dir)) == ["grads.npy", "loss.npy", "params.npy"]
    total = 0
    for name in os.listdir(a_dir):
        a = np.load(os.path.join(a_dir, name))
        b = np.load(os.path.join(b_dir, name))
        assert a.dtype == np.float32 and a.size > 0
        assert np.isfinite(a).all()
        # CPU fp32, same seed, same thread count: identical up to rounding
        np.testing.assert_allclose(a, b, rtol=1e-5, atol=1e-6, err_msg=name)
        total += a.nbytes
    assert total <= 64 * 1000 * 1000


def test_bench_dump_sampling_is_fixed_and_bounded(monkeypatch):
    """Above DUMP_MAX_ELEMS the dump is a seeded sample: bounded in size, the
    same positions on every call, drawn from the concatenated tensors."""
    import numpy as np
    import torch

    sys.path.insert(0, REPO)
    import bench

    monkeypatch.setattr(bench, "DUMP_MAX_ELEMS", 1000)
    small = [torch.arange(6.0).reshape(2, 3), torch.arange(6.0, 10.0)]
    np.testing.assert_array_equal(bench._sample_flat(small), np.arange(10.0))
    big = [torch.arange(0, 4000, dtype=torch.bfloat16).float().reshape(40, 100),
           torch.arange(4000.0, 10000.0)]
    s1, s2 = bench._sample_flat(big), bench._sample_flat(big)
    assert s1.dtype == np.float32 and s1.shape == (1000,)
    np.testing.assert_array_equal(s1, s2)
    assert (np.diff(s1) >= 0).all() and s1.max() > 4000 > s1.min()
