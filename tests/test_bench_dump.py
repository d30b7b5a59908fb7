"""CPU: bench.py's `--dump-outputs` writer (dump_outputs) on a small plain-torch module, and the `--steps` / `--warmup` check.
tests/test_hip_ddp.py runs the whole bench with `--dump-outputs` on a GPU."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn

from mp_util import run_bounded

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture
def bench(monkeypatch):
    monkeypatch.delenv("HSA_ENABLE_IPC_MODE_LEGACY", raising=False)     # (bench.py sets it at import: undone after the test)
    import bench as b
    return b


def _dump(bench, path):
    torch.manual_seed(0)
    model = nn.Sequential(nn.Linear(16, 300), nn.Linear(300, 3))
    out = {"b_loss": torch.tensor(0.5), "a_logits": torch.randn(7, 50), "big_logits": torch.randn(3, 2000).to(torch.bfloat16),
           "labels": torch.arange(7), "text": ["x"] * 7}
    info = bench.dump_outputs(str(path), torch.tensor(1.25), out, model)
    return info, out, model


def test_dump_outputs_writes_float_arrays_of_fixed_seeded_samples(bench, monkeypatch, tmp_path):
    monkeypatch.setattr(bench, "DUMP_SAMPLE", 1000)
    info, out, model = _dump(bench, tmp_path / "a")
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == ["a_logits.npy", "b_loss.npy", "big_logits_sample.npy", "labels.npy", "loss.npy", "param_norms.npy",
                     "param_sample.npy"], names
    assert info["arrays"] == len(names)
    got = {n[:-4]: np.load(tmp_path / "a" / n) for n in names}
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    assert got["loss"].dtype == np.float64 and got["loss"].tolist() == [1.25]
    assert np.array_equal(got["a_logits"], out["a_logits"].reshape(-1).numpy())
    assert np.array_equal(got["labels"], np.arange(7, dtype=np.float32))
    big = out["big_logits"].float().reshape(-1)
    pos = bench._seeded_positions("big_logits", big.numel(), 1000)
    assert got["big_logits_sample"].shape == (1000,) and np.array_equal(got["big_logits_sample"], big[pos].numpy())
    params = list(model.parameters())
    assert np.allclose(got["param_norms"], [p.detach().double().norm().item() for p in params], rtol=1e-12)
    assert got["param_sample"].shape == (sum(min(bench.DUMP_PARAM_SAMPLE, p.numel()) for p in params),)
    assert info["bytes"] == sum(a.nbytes for a in got.values())

    _dump(bench, tmp_path / "b")                          # same inputs -> the same files
    for n in names:
        assert np.array_equal(np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n)), n


def test_dump_outputs_refuses_more_than_64_mb(bench, monkeypatch, tmp_path):
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 1000)
    with pytest.raises(AssertionError, match="dump-outputs"):
        _dump(bench, tmp_path / "a")
    assert not os.path.exists(tmp_path / "a")             # nothing half written


@pytest.mark.parametrize("args", [["--steps", "0"], ["--warmup", "-1"]])
def test_bench_rejects_a_run_without_timed_steps(args):
    res = run_bounded([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1"] + args, 120, cwd=ROOT)
    assert res.returncode == 2 and "--steps must be >= 1" in res.stderr, res.stderr[-500:]
    assert not [l for l in res.stdout.splitlines() if l.startswith("{")]
