"""bench.py's output contract, checked without a GPU (missing #4):
 * the ONE JSON line with every BASELINE row present stays under the driver's 8 KB window, and each row keeps
   workload / value / ms_per_step / dtype / frac / kernel_ms / config.workload / cpu_baseline.value / cold;
 * `--gpus N` that disagrees with WORLD_SIZE is refused instead of printing a 1-GPU line;
 * `--gpus N` without a launcher starts N ranks itself (RANK / LOCAL_RANK / WORLD_SIZE / MASTER_* for each)."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _fake_row(name, bench):
    return {"workload": name, "label": "x" * 120, "value": 12345.678901234, "unit": "M samples/s", "dtype": "f32", "ms_per_step": 1.3680123456,
            "steps": 20, "warmup": 5, "preroll_steps": 44, "scaling": "weak",
            "config": {"workload": "RationalQuadraticSpline K=16 fwd+inv+logabsdetjac (BASELINE configs[2])", "dim": 32, "batch_per_gpu": 4194304},
            "roofline": {"bound": "hbm", "achieved": 6358.123456789, "peak": bench.HBM_PEAK_GBS, "unit": "GB/s", "frac": 0.79476543210, "traffic": 8598323200.0,
                         "traffic_source": "y" * 150, "kernel": "planar_reg2_kernel (forward + inverse launch)", "kernel_ms": 1.35134567,
                         "kernel_launches_per_step": 2.0, "stream_region_ms_per_step": 1.3612345, "algorithmic_bytes_per_launch": 8589934592,
                         "frac_of_measured_copy_ceiling_6290": 1.0108},
            "sum_logabsdetjac": -744261117.123, "cold": {"value": 11111.123456, "ms_per_step": 1.51234567, "kernel_ms": 1.4987654},
            "cpu_baseline": {"value": 12.3456789, "unit": "M samples/s", "cores": 1, "kind": "port", "sample": "z" * 200}, "us_per_call": 17.6123}


def test_the_line_fits_the_drivers_window_with_every_row():
    import bench

    a = argparse.Namespace(steps=20, warmup=5, scaling="weak", collective="torch", no_cache_params=False)
    names = ["c1", "c3", "c3_uncached", "c4", "c5a", "c5b", "c2_f64", "c4_f64"]
    head = _fake_row("c2", bench)
    cpu = dict(head["cpu_baseline"], variants={"fused_single_pass_1_core": {"value": 210.123456, "cores": 1}, "fused_single_pass_threads": {"value": 5210.123456, "cores": 64}})
    graph = [{"workload": w, "log2_batch_per_gpu": lb, "label": "q" * 100, "steps": 50, "eager_ms_per_step": 0.0176123, "graph_ms_per_step": 0.0140123,
              "speedup": 1.2567, "M_samples_per_s_graph": 1234.5, "sum_logabsdetjac_eager": 1.0, "sum_logabsdetjac_graph": 1.0} for w, lb in (("c1", None), ("c2", 20), ("c2", 16))]
    strong = [_fake_row("c2", bench), _fake_row("c4", bench)]
    line = bench.build_line(a, 8, head, [_fake_row(n, bench) for n in names], graph, strong, cpu)
    line["detail"] = "gpurun_out/bench_detail.json"
    text = json.dumps(line, separators=(",", ":"))
    assert len(text.encode()) < 7000, len(text.encode())        # the driver keeps an 8 KB tail
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline", "cold"):
        assert k in line, k
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
        assert k in line["roofline"], k
    assert [r["workload"] for r in line["rows"]] == names
    for r in line["rows"]:
        for k in ("workload", "value", "ms_per_step", "dtype", "frac", "kernel_ms", "cold"):
            assert k in r, (r["workload"], k)
        assert r["config"]["workload"] and r["cpu_baseline"]["value"] is not None


def test_gpus_flag_that_disagrees_with_the_launcher_is_refused():
    env = dict(os.environ, WORLD_SIZE="1", RANK="0", LOCAL_RANK="0")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "8"], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 2 and p.stdout.strip() == "" and "WORLD_SIZE=1" in p.stderr


def test_gpus_n_without_a_launcher_starts_n_ranks(tmp_path, monkeypatch):
    """spawn_ranks: every rank gets its RANK / LOCAL_RANK / WORLD_SIZE / MASTER_*, rank 0's stdout is relayed, a failing rank fails the run."""
    import bench

    seen = []

    class FakeP:
        def __init__(self, argv, env=None, stdout=None):
            seen.append((argv, {k: env[k] for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}, stdout))
            self.rank = int(env["RANK"])

        def communicate(self):
            return (b'{"n_gpus": 4}\n', None)

        def wait(self):
            return 0

    monkeypatch.setattr(subprocess, "Popen", FakeP)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "4", "--steps", "3"])
    out = []
    monkeypatch.setattr(sys.stdout, "write", lambda t: out.append(t))
    bench.spawn_ranks(argparse.Namespace(gpus=4))
    assert [e["RANK"] for _, e, _ in seen] == ["0", "1", "2", "3"] and all(e["WORLD_SIZE"] == "4" and e["MASTER_ADDR"] == "127.0.0.1" for _, e, _ in seen)
    assert len({e["MASTER_PORT"] for _, e, _ in seen}) == 1 and [e["LOCAL_RANK"] for _, e, _ in seen] == ["0", "1", "2", "3"]
    assert all(argv[2:] == ["--gpus", "4", "--steps", "3"] for argv, _, _ in seen)
    assert "".join(out) == '{"n_gpus": 4}\n'


def test_a_plain_line_carries_the_headline_only(monkeypatch):
    """A plain run (no --full) times the headline alone: the line keeps the contract's fields and says null for what it did not measure."""
    import bench

    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"])
    a = bench.parse()
    assert not a.full and a.dump_outputs is None and a.steps == 7
    head = {k: v for k, v in _fake_row("c2", bench).items() if k not in ("roofline", "cold", "cpu_baseline")}
    line = bench.build_line(a, 1, head, [], [], [], None)
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert line[k] is not None, k
    assert line["ms_per_step"] == head["ms_per_step"] and line["steps"] == 7
    assert line["roofline"] is None and line["cpu_baseline"] is None and line["cold"] is None and "rows" not in line


def test_dump_outputs_writes_a_seeded_sample_of_the_same_columns(tmp_path):
    """--dump-outputs: float32 / float64 arrays, at most 64 MB together; a batch too large for that keeps the same seeded columns in
    every array, from run to run."""
    import numpy as np
    import torch

    import bench

    n = 1 << 20
    col = torch.arange(n, dtype=torch.float32)
    outs = {"y": col.double()[None, :] * 100 + torch.arange(16, dtype=torch.float64)[:, None], "logabsdetjac": col.clone(),
            "logabsdetjac_sum": torch.tensor([3.5], dtype=torch.float64), "absent": None}
    for d in ("a", "b"):
        bench.dump_outputs(outs, str(tmp_path / d))
    files = sorted(p.name for p in (tmp_path / "a").iterdir())
    assert files == ["logabsdetjac.npy", "logabsdetjac_sum.npy", "y.npy"]
    assert sum((tmp_path / "a" / f).stat().st_size for f in files) <= 64 << 20
    y, l, s = (np.load(tmp_path / "a" / f) for f in ("y.npy", "logabsdetjac.npy", "logabsdetjac_sum.npy"))
    assert y.dtype == np.float64 and l.dtype == np.float32 and s.dtype == np.float64 and s.tolist() == [3.5]
    assert y.shape[0] == 16 and 1 < y.shape[1] < n and l.shape == (y.shape[1],)
    assert np.array_equal(y[0] / 100, l) and np.all(np.diff(l) > 0)                  # the same sorted columns in both arrays
    np.testing.assert_array_equal(y[5], l.astype(np.float64) * 100 + 5)
    for f in files:
        assert np.array_equal(np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f))
    small = {"y": torch.ones(4, 8, dtype=torch.float64)}                              # under the budget: written whole
    bench.dump_outputs(small, str(tmp_path / "c"))
    assert np.load(tmp_path / "c" / "y.npy").shape == (4, 8)


def test_the_kernel_pass_never_overfills_a_kernel_time_region():
    """The library records at most 1024 launches per bjx_kernel_time_begin/_end region: `--full --steps K` with K x launches per step
    above that cuts the kernel pass into regions of whole steps that together are exactly K steps."""
    import bench

    for steps, per_step in ((20, 3.0), (1093, 1.0), (3000, 3.0), (5000, 2.5), (7, 2000.0), (1, 1.0), (0, 3.0)):
        chunks = bench.kernel_chunks(steps, per_step)
        assert sum(chunks) == steps and all(c > 0 for c in chunks), (steps, per_step, chunks)
        if per_step <= bench.KERNEL_TIME_MAX_LAUNCHES:
            assert all(c * per_step <= bench.KERNEL_TIME_MAX_LAUNCHES for c in chunks), (steps, per_step, chunks)
    assert bench.kernel_chunks(20, 3.0) == [20] and len(bench.kernel_chunks(3000, 3.0)) == 9
    header = open(os.path.join(ROOT, "include", "bjx.h")).read()
    assert f"(at most {bench.KERNEL_TIME_MAX_LAUNCHES} per region)" in header
