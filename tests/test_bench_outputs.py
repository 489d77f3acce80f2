"""bench.py's plain run and its outputs: `--steps K` times exactly K steps, a plain run carries the headline only (everything
else runs under --full), and `--dump-outputs DIR` writes what the last timed step computed as DIR/<name>.npy -- identical
from run to run with the same arguments, so that two builds can be compared output for output."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

# what moved behind --full: none of it may appear in a plain run's line
FULL_ONLY = ("roofline", "roofline_stages", "roofline_planner", "roofline_planner_f16x3", "cpu_baseline", "utd_1_256",
             "seed_pack", "seed_pack_utd_1_256", "seed_pack_multi_gpu", "config4")


def test_write_outputs_keeps_floats_and_widens_the_rest(tmp_path):
    arrays = {"f32": torch.arange(6, dtype=torch.float32).view(3, 2), "f64": torch.tensor([0.1, 0.2], dtype=torch.float64),
              "counts": torch.tensor([2 ** 40 + 1, -3], dtype=torch.int64), "mask": torch.tensor([1, 0, 1], dtype=torch.uint8),
              "flags": torch.tensor([True, False])}
    names = bench.write_outputs(arrays, str(tmp_path / "out"))
    assert names == sorted(arrays)
    got = {n: np.load(str(tmp_path / "out" / (n + ".npy"))) for n in names}
    assert got["f32"].dtype == np.float32 and got["f32"].shape == (3, 2) and np.array_equal(got["f32"], np.arange(6).reshape(3, 2))
    assert got["f64"].dtype == np.float64 and np.array_equal(got["f64"], [0.1, 0.2])
    for n in ("counts", "mask", "flags"):                 # integers and masks: f64 holds them exactly
        assert got[n].dtype == np.float64
    assert got["counts"].tolist() == [2 ** 40 + 1, -3] and got["mask"].tolist() == [1, 0, 1] and got["flags"].tolist() == [1, 0]


def test_write_outputs_refuses_more_than_the_limit(tmp_path):
    with pytest.raises(ValueError, match="more than"):
        bench.write_outputs({"x": torch.zeros(1025, dtype=torch.float32)}, str(tmp_path / "out"), limit=4096)
    assert not os.path.exists(tmp_path / "out")           # nothing half-written
    assert bench.DUMP_LIMIT_BYTES == 64 << 20


def test_bench_options_for_the_full_run_and_the_dump():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "--full" in out.stdout and "--dump-outputs DIR" in out.stdout


def _plain_run(tmp_path, tag):
    d = tmp_path / tag
    env = dict(os.environ)
    env.pop("WORLD_SIZE", None)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "30", "--warmup", "5",
                          "--num_envs", "512", "--dump-outputs", str(d)], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    line = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(line) == 1, out.stdout[-2000:]
    arrays = {f[:-4]: np.load(str(d / f)) for f in sorted(os.listdir(d))}
    return json.loads(line[0]), arrays


@pytest.mark.gpu
def test_plain_run_times_exactly_the_steps_and_dumps_the_same_outputs_twice(tmp_path):
    r1, o1 = _plain_run(tmp_path, "a")
    r2, o2 = _plain_run(tmp_path, "b")
    for r in (r1, r2):
        assert r["steps"] == 30 and r["timed_blocks"] == 1 and r["timed_steps_total"] == 30
        assert r["unit"] == "env-steps/s" and r["higher_is_better"] is True and r["dtype"] == "f32"
        assert abs(r["ms_per_step"] - r["timed_seconds"] / 30 * 1e3) < 1e-9 * r["ms_per_step"]
        assert abs(r["value"] - 512 * 30 / r["timed_seconds"]) < 1e-6 * r["value"]
        assert not [k for k in FULL_ONLY if k in r], [k for k in FULL_ONLY if k in r]
    assert sorted(o1) == sorted(o2)
    for name in ("obs", "pos", "real_action", "recovery", "stats", "params_policy", "params_qrisk", "losses", "replay_s",
                 "constraint_replay_r"):
        assert name in o1, sorted(o1)
    assert sum(x.nbytes for x in o1.values()) <= 64 << 20
    assert all(x.dtype in (np.float32, np.float64) for x in o1.values())
    assert o1["obs"].shape == (512, 2) and np.isfinite(o1["params_policy"]).all()
    different = [n for n in o1 if not np.array_equal(o1[n], o2[n])]
    assert not different, different                       # same arguments, same inputs: the same outputs, bit for bit
