"""bench.py's own contract: a plain run times exactly --steps steps and prints only the headline line; --dump-outputs
writes what the last timed step computed, the same from run to run; everything else waits for --full."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_options_are_listed():
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--help"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "--full" in r.stdout and "--dump-outputs" in r.stdout


def test_step_outputs_are_host_float_arrays():
    import bench

    class BM:
        theta = torch.nn.Parameter(torch.arange(6, dtype=torch.float32))

    class VI:
        born_machine = BM()

    BM.theta.grad = torch.ones(6, dtype=torch.float32)
    out = bench.step_outputs(VI(), (torch.tensor([2.5], dtype=torch.float64), torch.tensor(1.5), torch.rand(16, dtype=torch.float64)))
    assert sorted(out) == ["grad_norm", "loss", "q", "theta", "theta_grad"]
    assert out["loss"].dtype == np.float64 and out["q"].dtype == np.float64 and out["theta"].dtype == np.float32
    np.testing.assert_array_equal(out["theta"], np.arange(6, dtype=np.float32))
    # the host-synchronising step hands back a Python float: kept in float64
    assert bench.step_outputs(VI(), (2.5, None, torch.zeros(4, dtype=torch.float64)))["loss"].dtype == np.float64


def test_write_outputs(tmp_path):
    import bench
    bench.write_outputs({"a": np.arange(5, dtype=np.float64), "b": np.ones(3, dtype=np.float32), "c": np.arange(4)}, str(tmp_path / "d"))
    assert sorted(os.listdir(tmp_path / "d")) == ["a.npy", "b.npy", "c.npy"]
    np.testing.assert_array_equal(np.load(tmp_path / "d" / "a.npy"), np.arange(5))
    assert np.load(tmp_path / "d" / "b.npy").dtype == np.float32 and np.load(tmp_path / "d" / "c.npy").dtype == np.float64
    with pytest.raises(SystemExit):
        bench.write_outputs({"big": np.zeros((65 << 20) // 8)}, str(tmp_path / "e"))
    assert not os.path.exists(tmp_path / "e")


def _plain_run(out_dir, steps):
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "1",
                        "--workload", "n12_L4_dense", "--dump-outputs", str(out_dir)],
                       cwd=REPO, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_times_the_steps_and_dumps_the_same_outputs(tmp_path):
    steps = 3
    rec = _plain_run(tmp_path / "a", steps)
    for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert key in rec, key
    assert rec["metric"] == "ksd_gradient_steps_per_sec" and rec["unit"] == "steps/s" and rec["dtype"] == "f64"
    assert rec["steps"] == steps and rec["repeats"]["n"] == 1 and rec["repeats"]["steps_each"] == steps
    assert rec["ms_per_step"] > 0 and abs(rec["value"] * rec["ms_per_step"] - 1e3) <= 1e-2 * 1e3
    for moved in ("series", "cpu_baseline", "gate_apply", "kernels", "roofline", "extras", "phase_ms"):
        assert moved not in rec, moved                     # --full only
    a = {f[:-4]: np.load(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")}
    assert sorted(a) == ["grad_norm", "loss", "q", "theta", "theta_grad"]
    assert all(v.dtype in (np.float32, np.float64) for v in a.values())
    assert a["q"].shape == (1 << 12,) and abs(a["q"].sum() - 1.0) < 1e-12 and np.isfinite(a["loss"]).all()
    assert a["theta"].shape == (rec["config"]["params"],)
    _plain_run(tmp_path / "b", steps)                      # a second cold process: the same inputs give the same outputs
    for name, v in a.items():
        w = np.load(tmp_path / "b" / (name + ".npy"))
        np.testing.assert_allclose(w, v, rtol=1e-12 if v.dtype == np.float64 else 1e-6, atol=0, err_msg=name)
