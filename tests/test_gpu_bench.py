"""bench.py end to end on the GPU at a small config: the one JSON line the
driver reads (its keys, units and roofline object), at N = 1 and at N = 2
(torchrun, gloo ranks sharing the one GPU: the N > 1 step schedule, the
adaptive exchange and the max-over-ranks timing; the 2..8-GPU RCCL runs are
the driver's)."""
import json
import os
import socket
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ["--config", "small", "--samples", str(1 << 22), "--steps", "2", "--warmup", "1", "--pmc", "off"]

pytestmark = pytest.mark.gpu


def _json_line(out):
    lines = [l for l in out.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out[-2000:]
    return json.loads(lines[0])


def _check_contract(d, n, schedule="blocks"):
    assert d["metric"] == "M edge-updates/sec (d=64, neg=5)" and d["unit"] == "M edge-updates/s"
    assert d["n_gpus"] == n and d["steps"] == 2 and d["warmup"] == 1
    assert d["value"] > 0 and d["ms_per_step"] > 0 and d["higher_is_better"] is True
    assert d["scaling"] == "weak" and d["dtype"] == "f32" and d["vs_baseline"] is None
    par = "replicas%d" % n if n == 1 else "%s%d" % (schedule, n)
    assert d["config"]["parallelism"] == par and "workload" in d["config"]
    assert d["setup"]["max_setup_s"] > 0 and len(d["setup"]["ranks"]) == n
    r = d["roofline"]
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
        assert k in r
    assert r["bound"] == "hbm" and r["unit"] == "GB/s" and r["peak"] == 8000.0
    assert abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-3
    assert d["skipped_samples"] == 0
    assert d["config"]["scatter"] == "hybrid" and d["config"]["scatter_asked"] == "hybrid"


def test_bench_json_line_n1():
    """--full (here without its CPU baseline and live PMC legs): the copy
    bandwidth and the whole-table finite check run too."""
    p = subprocess.run([sys.executable, "bench.py", "--full", "--no-cpu-baseline"] + SMALL, cwd=ROOT,
                       capture_output=True, text=True, timeout=240)
    assert p.returncode == 0, p.stderr[-2000:]
    d = _json_line(p.stdout)
    _check_contract(d, 1)
    assert d["cpu_baseline"] is None and d["config"]["sync"] == "none"
    mp = d["roofline"]["measured_peak"]
    assert mp["copy_GBs"] > 0 and mp["frac"] > 0


def test_bench_plain_run_dumps_outputs(tmp_path):
    """A plain run (no --full) measures nothing of its own beyond the steps
    -- no CPU baseline, no copy bandwidth, the committed traffic or none --
    and --dump-outputs writes the W and C tables the last step leaves when
    run once more from the seeded tables: the small config has 100000 rows,
    so the seeded sample of bench.DUMP_ROWS rows, float32, finite, trained
    (C starts at zero), under 64 MB in all."""
    import numpy as np
    out = tmp_path / "dump"
    p = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--dump-outputs", str(out)] + SMALL[:-2],
                       cwd=ROOT, capture_output=True, text=True, timeout=240)
    assert p.returncode == 0, p.stderr[-2000:]
    d = _json_line(p.stdout)
    _check_contract(d, 1)
    assert d["cpu_baseline"] is None and d["roofline"]["measured_peak"] is None
    assert "pmc:" not in p.stderr      # no live rocprofv3 child runs
    assert sorted(f.name for f in out.iterdir()) == ["C.npy", "W.npy", "rows.npy"]
    assert sum(f.stat().st_size for f in out.iterdir()) <= 64 << 20
    rows = np.load(out / "rows.npy")
    n = min(65536, d["config"]["vertices"])
    assert rows.dtype == np.float64 and rows.shape == (n,)
    assert (np.diff(rows) > 0).all() and rows[0] >= 0 and rows[-1] < d["config"]["vertices"]
    for name in ("W", "C"):
        t = np.load(out / (name + ".npy"))
        assert t.dtype == np.float32 and t.shape == (n, 64) and np.isfinite(t).all()
        assert np.count_nonzero(np.abs(t).sum(1)) > n // 2


@pytest.mark.parametrize("schedule", ["blocks", "replicas"])
def test_bench_json_line_n2_gloo_ranks(schedule):
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    p = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                        "--master-addr", "127.0.0.1", "--master-port", str(port), "bench.py", "--gpus", "2", "--full",
                        "--dist-backend", "gloo", "--schedule", schedule] + SMALL, cwd=ROOT, capture_output=True, text=True, timeout=300,
                       env=env)
    assert p.returncode == 0, p.stderr[-2000:]
    d = _json_line(p.stdout)
    _check_contract(d, 2, schedule)
    if schedule == "blocks":
        assert d["config"]["sync"].startswith("blocks")
    else:
        assert d["config"]["sync"].startswith("adaptive") and "1/2 step" in d["config"]["sync"]


def test_bench_gpus_flag_starts_the_ranks():
    """`python bench.py --gpus 2` (no launcher) starts 2 ranks itself: the
    line says n_gpus 2 and the block schedule's parallelism (VERDICT r5
    item 2; gloo ranks sharing the one GPU here)."""
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    p = subprocess.run([sys.executable, "bench.py", "--gpus", "2", "--full", "--dist-backend", "gloo"] + SMALL, cwd=ROOT,
                       capture_output=True, text=True, timeout=300, env=env)
    assert p.returncode == 0, p.stderr[-2000:]
    d = _json_line(p.stdout)
    _check_contract(d, 2, "blocks")
    assert d["config"]["parallelism"] == "blocks2"
