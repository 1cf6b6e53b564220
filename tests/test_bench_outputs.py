"""bench.py's plain run and --dump-outputs: a plain run prints the headline line only (what takes runs of its own
sits behind --full), --steps is the number of timed steps, and --dump-outputs writes the last timed step's
results as float32 .npy files within the size budget, reproducibly."""
import json
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

FULL_ONLY = ("roofline", "roofline_by_family", "roofline_critical_path", "cpu_baseline", "f32_sensitivity",
             "vocab_1024_sensitivity", "encoder_fm_router_sensitivity", "xl_shape_sensitivity", "xl_fp8_sensitivity")


def _fake_engine(n):
    g = torch.Generator().manual_seed(3)
    st = types.SimpleNamespace(data=torch.randn(n, generator=g), grad=torch.randn(n, generator=g).double())
    return types.SimpleNamespace(losses=torch.arange(5.0), student=st)


def test_dump_outputs_whole_arrays(tmp_path):
    eng = _fake_engine(1000)
    bench.dump_outputs(str(tmp_path / "out"), eng)
    got = {n: np.load(tmp_path / "out" / f"{n}.npy") for n in ("losses", "student_params", "student_grad")}
    assert sorted(os.listdir(tmp_path / "out")) == ["losses.npy", "student_grad.npy", "student_params.npy"]
    assert all(a.dtype == np.float32 for a in got.values())
    np.testing.assert_array_equal(got["losses"], np.arange(5, dtype=np.float32))
    np.testing.assert_array_equal(got["student_params"], eng.student.data.numpy())
    np.testing.assert_array_equal(got["student_grad"], eng.student.grad.float().numpy())


def test_dump_outputs_samples_within_budget(tmp_path):
    eng = _fake_engine(1000)
    budget = 3 * 4 * 100   # 100 float32 elements per array
    bench.dump_outputs(str(tmp_path / "a"), eng, max_bytes=budget)
    bench.dump_outputs(str(tmp_path / "b"), eng, max_bytes=budget)
    total = 0
    for n in ("losses", "student_params", "student_grad"):
        a, b = np.load(tmp_path / "a" / f"{n}.npy"), np.load(tmp_path / "b" / f"{n}.npy")
        np.testing.assert_array_equal(a, b)   # the same fixed sample every run
        total += a.nbytes
    assert total <= budget
    p = np.load(tmp_path / "a" / "student_params.npy")
    assert p.shape == (100,)
    full = eng.student.data.numpy()
    idx = np.sort(np.random.default_rng(0).choice(1000, size=100, replace=False))
    np.testing.assert_array_equal(p, full[idx])
    assert np.load(tmp_path / "a" / "losses.npy").shape == (5,)


def test_steps_must_be_positive(monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--steps", "0"])
    with pytest.raises(SystemExit):
        bench.parse()


def test_full_is_off_by_default(monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "3", "--warmup", "1"])
    a = bench.parse()
    assert a.full is False and a.dump_outputs is None and a.steps == 3
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "d"])
    a = bench.parse()
    assert a.full is True and a.dump_outputs == "d"


@pytest.mark.gpu
def test_plain_run_prints_headline_and_dumps(tmp_path):
    """One small plain run (B=2 x 1 s): the line holds the headline entries and none of --full's, and the dumped
    arrays are the step's: 5 finite losses equal to the line's, parameters and gradient of one length."""
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                        "--batch", "2", "--samples", "16000", "--dump-outputs", str(out)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    line = json.loads(lines[0])
    assert line["steps"] == 2 and line["unit"] == "utterances/sec" and line["higher_is_better"] is True
    assert line["dtype"] == "bf16" and line["full"] is False
    assert line["ms_per_step"] > 0
    assert line["value"] == pytest.approx(2 * 1000.0 / line["ms_per_step"], rel=1e-3)
    assert not any(k in line for k in FULL_ONLY)
    losses = np.load(out / "losses.npy")
    params, grad = np.load(out / "student_params.npy"), np.load(out / "student_grad.npy")
    assert losses.dtype == params.dtype == grad.dtype == np.float32
    assert losses.shape == (5,) and np.isfinite(losses).all()
    np.testing.assert_allclose(losses, line["losses_last_step"], rtol=0, atol=1e-5)   # the line rounds to 5 places
    assert params.shape == grad.shape and params.size > 1000
    assert np.isfinite(params).all() and np.isfinite(grad).all() and np.abs(grad).max() > 0
