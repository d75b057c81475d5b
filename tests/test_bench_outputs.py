"""bench.py's plain / --full split and --dump-outputs on CPU: the legs beside the headline run under --full only
(checked around the empty step of --launch-check), and the dump writes float64 .npy files within its byte limit,
a larger array as the same seeded sample every time."""
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402


def _run(args):
    e = dict(os.environ)
    e.pop("WORLD_SIZE", None)
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args], capture_output=True, text=True,
                          timeout=180, env=e, cwd=ROOT)


def test_c3_leg_needs_full():
    out = _run(["--launch-check", "--c3-leg", "on"])
    assert out.returncode == 2 and "--full" in out.stderr
    out = _run(["--launch-check", "--full", "--c3-leg", "on", "--steps", "1", "--warmup", "0"])
    assert out.returncode == 0, out.stderr[-2000:]
    assert json.loads(out.stdout.splitlines()[-1])["c3"]["ranks"] == 1


def test_two_ranks_without_full_run_no_c3_leg():
    out = _run(["--gpus", "2", "--same-device", "--launch-check", "--steps", "2", "--warmup", "0"])
    assert out.returncode == 0, out.stderr[-2000:]
    rec = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][0])
    assert rec["c3"] is None and rec["steps"] == 2 and rec["ms_per_step"] >= 0.0


def test_steps_must_be_positive():
    out = _run(["--launch-check", "--steps", "0"])
    assert out.returncode == 2 and "--steps" in out.stderr


def test_dump_outputs_small_arrays_whole(tmp_path):
    rng = np.random.default_rng(0)
    out = {"B": rng.standard_normal((2, 30)), "y_pred": rng.standard_normal((7, 2)).astype(np.float32),
           "mu": np.array([1.5, -2.0]), "msum": np.array([0.25, 4.0])}
    bench.dump_outputs(str(tmp_path / "d"), out)
    assert sorted(os.listdir(tmp_path / "d")) == ["B.npy", "msum.npy", "mu.npy", "y_pred.npy"]
    for k, v in out.items():
        a = np.load(tmp_path / "d" / (k + ".npy"))
        assert a.dtype == np.float64 and a.shape == v.shape and np.array_equal(a, v.astype(np.float64))


def test_dump_outputs_samples_beyond_the_limit(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 8 * 2 * 1000)  # 2 arrays: 1000 - 16 elements each
    big = np.arange(50000, dtype=np.float64).reshape(100, 500) * 0.5
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"B": big, "mu": np.ones(3)})
    a, b = np.load(tmp_path / "a" / "B.npy"), np.load(tmp_path / "b" / "B.npy")
    assert a.shape == (984,) and np.array_equal(a, b)  # the same elements from run to run
    assert np.all(np.diff(a) > 0) and set(a) <= set(big.reshape(-1))  # distinct elements of the array, in order
    assert np.array_equal(np.load(tmp_path / "a" / "mu.npy"), np.ones(3))
    total = sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a"))
    assert total <= bench.DUMP_LIMIT_BYTES
