"""bench.py driver contract: one JSON line from rank 0 with the required
fields, under both plain and torchrun invocation."""

import json
import os
import socket
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

REQUIRED = {"metric", "value", "unit", "n_gpus", "steps", "warmup",
            "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
            "dtype", "data", "config"}


def _extract_json(stdout):
    lines = [ln for ln in stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, "exactly one JSON line expected: {!r}".format(lines)
    return json.loads(lines[0])


@pytest.mark.timeout(420)
def test_bench_json_contract():
    out = subprocess.run(
        [sys.executable, "bench.py", "--steps", "2", "--warmup", "1",
         "--batch", "4", "--model", "resnet56_cifar"],
        capture_output=True, text=True, cwd=REPO, timeout=360)
    assert out.returncode == 0, out.stderr[-1500:]
    r = _extract_json(out.stdout)
    assert REQUIRED <= set(r.keys())
    assert r["n_gpus"] == 1 and r["steps"] == 2 and r["warmup"] == 1
    assert r["higher_is_better"] is True and r["scaling"] == "weak"
    assert r["unit"] == "images/sec" and r["value"] > 0
    assert r["dtype"] == "bf16" and "synthetic" in r["data"]
    assert r["config"]["global_batch"] == 4
    assert r["config"]["parallelism"] == "dp1"


@pytest.mark.timeout(500)
def test_bench_torchrun_world2_aggregates():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    out = subprocess.run(
        [sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
         "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
         "--master-port", str(port), "bench.py", "--gpus", "2",
         "--steps", "2", "--warmup", "1", "--batch", "4",
         "--model", "mnist_mlp"],
        capture_output=True, text=True, cwd=REPO, timeout=420)
    assert out.returncode == 0, out.stderr[-1500:]
    r = _extract_json(out.stdout)
    assert r["n_gpus"] == 2
    assert r["config"]["global_batch"] == 8       # whole-job aggregate
    assert r["config"]["parallelism"] == "dp2"


@pytest.mark.timeout(300)
def test_bench_dump_outputs_reproducible(tmp_path):
    """--dump-outputs writes the last timed step's arrays as float .npy, and
    two runs with the same arguments start from identical inputs (seeded init
    and data), so on CPU their outputs agree. --full is accepted alongside."""
    import numpy as np
    # hide any GPU: the comparison below relies on CPU arithmetic
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES="")
    dumps = []
    for tag, extra in (("a", []), ("b", ["--full"])):
        d = tmp_path / tag
        out = subprocess.run(
            [sys.executable, "bench.py", "--gpus", "1", "--steps", "3",
             "--warmup", "1", "--batch", "4", "--model", "mnist_mlp",
             "--dump-outputs", str(d)] + extra,
            capture_output=True, text=True, cwd=REPO, env=env, timeout=240)
        assert out.returncode == 0, out.stderr[-1500:]
        r = _extract_json(out.stdout)
        assert r["steps"] == 3 and r["ms_per_step"] > 0
        dumps.append({p.stem: np.load(p) for p in sorted(d.glob("*.npy"))})
    a, b = dumps
    assert {"loss", "logits", "params"} <= set(a) and set(a) == set(b)
    assert a["logits"].shape == (4, 10) and a["loss"].shape == (1,)
    assert sum(v.nbytes for v in a.values()) <= 64 << 20
    for name in a:
        assert a[name].dtype in (np.float32, np.float64)
        assert np.isfinite(a[name]).all()
        # fp32 CPU arithmetic on identical inputs; allow last-bit reduction
        # order differences only
        np.testing.assert_allclose(a[name], b[name], rtol=1e-5, atol=1e-6,
                                   err_msg=name)


@pytest.mark.timeout(300)
def test_bench_no_launcher_does_not_hang():
    """`--gpus 8` without torchrun must run single-process (no peer wait)."""
    out = subprocess.run(
        [sys.executable, "bench.py", "--gpus", "8", "--steps", "1",
         "--warmup", "0", "--batch", "2", "--model", "mnist_mlp"],
        capture_output=True, text=True, cwd=REPO, timeout=240)
    assert out.returncode == 0, out.stderr[-1500:]
    assert _extract_json(out.stdout)["n_gpus"] == 1
