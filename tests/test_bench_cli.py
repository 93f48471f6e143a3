"""bench.py's command line at N=1 on CPU (the stub attack engine of the gloo tests): what a plain
run does and prints, what `--full` adds, and `--dump-outputs`."""
import json
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STUB = ["--device", "cpu", "--engine-factory", "bench_stub:make_engine", "--batch", "2",
        "--size", "16"]


@pytest.fixture
def run_bench(monkeypatch, capsys):
    for p in (ROOT, os.path.join(ROOT, "tests")):
        monkeypatch.syspath_prepend(p)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    import bench

    def run(*argv):
        monkeypatch.setattr(sys, "argv", ["bench.py", *STUB, *argv])
        bench.main()
        lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
        assert len(lines) == 1, lines
        return json.loads(lines[0])
    return run


def _stub_output():
    """bench_stub.StubEngine.run on run_leg's rank-0 inputs (seed 1000, batch 2, 16²)."""
    g = torch.Generator().manual_seed(1000)
    x0 = torch.rand(2, 3, 16, 16, generator=g) * 2 - 1
    t = torch.rand(2, 3, 16, 16, generator=g) * 2 - 1
    return torch.clamp(x0 + 2 * (8 / 255) * torch.sign(t - x0), -1.0, 1.0)


def test_plain_run_prints_the_headline_only(run_bench):
    out = run_bench("--gpus", "1", "--steps", "3", "--warmup", "1")
    for k in ("roofline", "low_precision", "cpu_baseline"):
        assert k not in out
    assert out["steps"] == 3 and out["warmup"] == 1 and out["n_gpus"] == 1
    assert out["unit"] == "attacked images/s" and out["higher_is_better"] is True
    assert out["dtype"] == "f32" and "PGD-20" in out["metric"]
    # the stub sleeps 0.05 s per step: ms_per_step is the time of ONE of the 3 timed steps
    assert 50 <= out["ms_per_step"] < 150
    assert out["value"] == pytest.approx(2 / (out["ms_per_step"] / 1e3))


def test_full_adds_the_low_precision_leg(run_bench):
    out = run_bench("--steps", "1", "--warmup", "1", "--full", "--no-cpu-baseline")
    lp = out["low_precision"]
    assert lp["dtype"] == "f16" and lp["steps"] == 2 and lp["output_in_eps_ball_and_finite"]
    assert "cpu_baseline" not in out
    assert out["dtype"] == "f32"  # the headline is still the fp32 leg


def test_dump_outputs_is_the_last_steps_output_and_repeats(run_bench, tmp_path):
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    run_bench("--steps", "2", "--warmup", "1", "--dump-outputs", a)
    run_bench("--steps", "2", "--warmup", "1", "--dump-outputs", b)
    assert os.listdir(a) == ["adv.npy"]
    got = np.load(os.path.join(a, "adv.npy"))
    assert got.dtype == np.float32 and got.shape == (2, 3, 16, 16)
    assert np.array_equal(got, _stub_output().numpy())
    assert np.array_equal(got, np.load(os.path.join(b, "adv.npy")))


def test_dump_outputs_samples_a_large_output(run_bench, tmp_path, monkeypatch):
    import bench
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 4 * 100)
    big = torch.arange(2 * 3 * 16 * 16, dtype=torch.float16).reshape(2, 3, 16, 16)
    bench.dump_outputs(str(tmp_path), big)
    first = np.load(str(tmp_path / "adv.npy"))
    bench.dump_outputs(str(tmp_path), big)
    assert first.dtype == np.float32 and first.shape == (100,)
    assert np.array_equal(first, np.load(str(tmp_path / "adv.npy")))  # the same sample every time
    # distinct elements of the output, in ascending flat-index order
    assert (np.diff(first) > 0).all() and first.max() < big.numel()
