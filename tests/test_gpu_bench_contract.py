"""bench.py's output contract: exactly one JSON line on stdout with the agreed keys (a small grid so
that the test takes seconds; the default run is the full 0.25 degree configuration).  A plain run
carries the headline figure only; the other legs ride the line with --full."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


@pytest.mark.gpu
def test_bench_prints_one_json_line_with_the_contract_keys():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--full",
                          "--cells", "20000", "--cpu-cells", "16", "--parity-cells", "16", "--other-cells", "6000"],
                         capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, out.stdout[-2000:]
    d = json.loads(lines[0])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline", "other_configs"):
        assert k in d, k
    # SURVEY 8(d) "report both f32 and f64" + the other BASELINE configs ride the same line
    oc = d["other_configs"]
    # (round 4: six of them -- float64 legs of configs[1] and of the configs[4] share too -- each with its own parity sample;
    # round 5: five more on configs[2]'s shape -- values at 0.01 K with sea-ice plateaus (scattered, packs), AR(1)
    # anomalies, int16 codes read in place)
    assert len(oc) == 11 and all("error" not in o for o in oc), oc
    assert sum(o["dtype"].startswith("f64") for o in oc) == 3
    assert sum("0.01 K" in o["workload"] or "AR(1)" in o["workload"] for o in oc) == 3
    # ... and the int16-packed legs (codes read in place, float32 and float64 decode)
    assert sum(o["dtype"].startswith("i16") for o in oc) == 2
    assert all(o["parity_cells"] >= 16 for o in oc)
    assert all(o["parity_ok"] and o["roofline_frac"] > 0 and o["ms_per_step"] > 0 for o in oc), oc
    assert d["n_gpus"] == 1 and d["steps"] == 2 and d["warmup"] == 1
    assert d["unit"] == "cells/s" and d["higher_is_better"] is True and d["scaling"] == "weak"
    assert d["vs_baseline"] is None and d["data"] == "synthetic"
    assert "workload" in d["config"] and "model" not in d["config"]
    r = d["roofline"]
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
        assert k in r, k
    assert r["bound"] == "hbm" and r["unit"] == "GB/s" and r["peak"] == 8000.0
    # the resource that actually binds the kernel rides next to the HBM fraction (null only without rocprofv3)
    assert "binding" in r
    if r["binding"] is not None:
        b = r["binding"]
        assert 0.0 < b["frac_of_issue_peak"] <= 1.0 and b["insts_per_wave_row"]["valu"] > 100
    assert abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-12
    c = d["cpu_baseline"]
    for k in ("value", "unit", "cores", "kind", "sample"):
        assert k in c, k
    assert c["kind"] in ("port", "reference") and c["cores"] >= 1 and c["value"] > 0
    assert d["parity"]["ok"] is True
    assert d["value"] > 0 and abs(d["value"] - 20000 * 2 / (d["ms_per_step"] * 2e-3)) / d["value"] < 1e-6


def _plain_run(outdir, *extra):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                          "--cells", "20000", "--dump-outputs", str(outdir)] + list(extra),
                         capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, out.stdout[-2000:]
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_times_the_path_alone_and_dumps_what_it_computed(tmp_path):
    """No --full: the headline figure and nothing else; --dump-outputs writes thresh / seas of the last timed step for a
    fixed sample of cells, the same from run to run, and the same through the gather path (--force-dist)"""
    d = _plain_run(tmp_path / "a")
    assert d["metric"] == "grid-cells/sec for threshold() on 40yr daily SST" and d["unit"] == "cells/s"
    assert d["higher_is_better"] is True and d["dtype"] == "f32 in / f64 out"
    assert d["steps"] == 3 and d["warmup"] == 1 and d["ms_per_step"] > 0
    assert abs(d["value"] - 20000 / (d["ms_per_step"] * 1e-3)) / d["value"] < 1e-6
    for k in ("cpu_baseline", "other_configs", "parity"):
        assert k not in d, k
    assert d["roofline"]["traffic"] is None and d["roofline"]["binding"] is None and d["roofline"]["avg_launch_ms"] > 0
    a = {n: np.load(tmp_path / "a" / f"{n}.npy") for n in ("thresh", "seas")}
    assert sorted(os.listdir(tmp_path / "a")) == ["seas.npy", "thresh.npy"]
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")) <= 64_000_000
    for v in a.values():
        assert v.dtype == np.float64 and v.shape == (366, 8192) and np.isfinite(v).all()
    assert (a["thresh"] > a["seas"]).mean() > 0.99          # the 90th percentile lies above the mean
    _plain_run(tmp_path / "b")
    _plain_run(tmp_path / "c", "--force-dist")
    for sub in ("b", "c"):
        for n in ("thresh", "seas"):
            np.testing.assert_array_equal(np.load(tmp_path / sub / f"{n}.npy"), a[n])


@pytest.mark.gpu
def test_bench_gather_path_with_one_rank():
    """--force-dist: the RCCL communicator (C ABI), the per-slab gather on a second stream and the
    multi_gpu block of the JSON line, with the one rank a 1-GPU box has"""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--full",
                          "--cells", "20000", "--no-cpu", "--no-pmc", "--parity-cells", "16", "--force-dist"],
                         capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, out.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["ranks"] == 1 and d["config"]["slabs"] == 4 and "xmhw_gather_blocks" in d["config"]["gather"]
    assert d["multi_gpu"]["step_ms"] > 0 and d["parity"]["ok"] is True
    # the N-rank == 1-rank check really compares columns (first columns of the first slab, last of the last)
    assert d["multi_gpu"]["compared_columns"] == 64 and d["multi_gpu"]["n_rank_equals_1_rank_bitwise"] is True


@pytest.mark.gpu
def test_bench_starts_its_own_ranks():
    """`python bench.py --gpus 2` with no launcher environment: the parent spawns the two workers
    (strong scaling of configs[3]); needs two GPUs"""
    sys.path.insert(0, ROOT)
    from xmhw_amd._lib import hip
    n = hip().device_count()
    if n < 2:
        pytest.skip(f"needs 2 GPUs, this box has {n}")
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1", "--full",
                          "--cells", "40000", "--parity-cells", "16"], capture_output=True, text=True, timeout=900, env=env)
    assert out.returncode == 0, out.stderr[-3000:]
    d = json.loads([l for l in out.stdout.splitlines() if l.strip()][0])
    assert d["n_gpus"] == 2 and d["ranks"] == 2 and d["scaling"] == "strong"
    assert d["multi_gpu"]["n_rank_equals_1_rank_bitwise"] is True and d["parity"]["ok"] is True
    assert d["multi_gpu"]["compared_columns"] == 2 * 2 * 32
    assert d["multi_gpu"]["single_rank_ms_same_workload"] > 0 and d["multi_gpu"]["speedup_vs_single_rank"] > 0
