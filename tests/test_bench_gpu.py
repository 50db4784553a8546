"""bench.py end to end on the GPU, each run in a fresh interpreter exactly as the driver starts it
(round 2 began with a bench that failed at its first launch while every other GPU test passed: the
library was loaded before torch and two HIP runtimes were mapped). Short runs; the line must carry the
driver's keys and the measurement blocks, and every rate must be positive and below the HBM peak."""
import json
import os
import socket
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
        "vs_baseline", "dtype", "data", "config", "roofline")


def _line(cmd, env=None, timeout=240):
    p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=timeout,
                       env=dict(os.environ, **(env or {})))
    assert p.returncode == 0, p.stdout[-1500:] + p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, f"stdout must be exactly one JSON line, got {len(lines)}: {p.stdout[-800:]}"
    d = json.loads(lines[0])
    for k in KEYS:
        assert k in d, k
    assert 0 < d["value"] and 0 < d["roofline"]["achieved"] < d["roofline"]["peak"]
    return d


def test_bench_default_line_short():
    d = _line([sys.executable, "bench.py", "--steps", "3", "--warmup", "1", "--no-cpu", "--no-h2d", "--no-extra",
               "--full"])
    assert d["n_gpus"] == 1 and d["steps"] == 3 and d["config"]["k_inputs"] == 2
    assert d["exact"] is True and len(d["roofline"]["per_set_us"]) == 3


def _load_dump(directory):
    import numpy as np
    arrays = {p.name: np.load(p) for p in sorted(directory.iterdir())}
    assert list(arrays) == ["dst0.npy"]  # C2 has one output buffer
    a = arrays["dst0.npy"]
    assert a.dtype == np.float32 and 0 < a.nbytes <= 64 * 1000 * 1000 and np.isfinite(a).all()
    return a


def test_bench_plain_line_and_dumped_outputs(tmp_path):
    """The plain line (no --full) carries the headline and nothing measured after the timed steps;
    --dump-outputs writes the last timed step's output, the same from run to run and whatever else
    the run measures, and it is the sum of the two seeded uniform [-1, 1) inputs."""
    import numpy as np
    d = _line([sys.executable, "bench.py", "--gpus", "1", "--steps", "4", "--warmup", "1", "--dump-outputs",
               str(tmp_path / "plain")])
    assert d["steps"] == 4 and d["warmup"] == 1 and d["full"] is False
    for k in ("exact", "extra_configs", "c1_ring", "cpu_baseline", "h2d_inclusive"):
        assert k not in d, k
    assert d["value"] == pytest.approx(3 * (256 << 20) / (d["ms_per_step"] / 1e3) / 1e9, rel=1e-3)
    a = _load_dump(tmp_path / "plain")
    assert d["dumped_outputs"] == {"dst0.npy": a.size}
    assert np.abs(a).max() < 2.0 and 0.60 < a.std() < 1.0 and abs(a.mean()) < 0.01  # std of the sum: sqrt(2/3)
    f = _line([sys.executable, "bench.py", "--gpus", "1", "--steps", "4", "--warmup", "1", "--dump-outputs",
               str(tmp_path / "full"), "--full", "--no-cpu", "--no-h2d", "--no-extra"])
    assert f["exact"] is True
    assert np.array_equal(a, _load_dump(tmp_path / "full"))


def test_bench_extra_configs_and_c1():
    d = _line([sys.executable, "bench.py", "--steps", "3", "--warmup", "1", "--no-cpu", "--no-h2d", "--full"])
    assert set(d["extra_configs"]) == {"c3_f16", "c3_bf16", "c4_i32_min", "c4_i32_max", "c4_i32_prod", "c4_i8_min",
                                       "c4_i8_max", "c4_i8_prod"}
    for v in d["extra_configs"].values():
        assert 0 < v["frac"] < 1
    assert "error" not in d["c1_ring"], d["c1_ring"]
    assert all(d["c1_ring"][k]["exact"] for k in ("device", "device_ll", "device_ll128", "host_staged", "cpu_oracle"))
    assert d["c1_ring"]["device"]["step_wait"] == "word"  # both emulated ranks on the one GPU
    assert "resident_ring" not in d and "device_resident" not in d["c1_ring"]  # extras: not in the default line


def test_bench_fanout_rehearsal():
    d = _line([sys.executable, "bench.py", "--gpus", "2", "--steps", "3", "--warmup", "1", "--no-xgmi", "--full"],
              env={"NEXR_BENCH_FOLD": "1"})
    assert d["n_gpus"] == 2 and "c5" in d
    assert d["phase_s"]["total"] < d["phase_s"]["cap_s"]


def test_bench_torchrun_two_ranks():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    d = _line([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr",
               "127.0.0.1", "--master-port", str(port), "bench.py", "--gpus", "2", "--steps", "3", "--warmup", "1",
               "--no-xgmi", "--full"])
    assert d["n_gpus"] == 2 and len(d["per_gpu"]["wall_gbs"]) == 2 and "c5" in d
