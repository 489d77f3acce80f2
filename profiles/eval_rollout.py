"""Policy evaluation at 4096 envs, Navigation 1, model-free recovery, hidden 256: the eager module path
(Experiment.get_test_rollout_vectorized as the parent commit runs it: horizon + 1 x loop.act(train=False) + env.step) against
the rrl_eval_rollout kernel path (RRL_FAST_EVAL=1), in one process.  `--env maze`: the same for Maze with the flags of
BASELINE config 3, the kernel path being rrl_eval_rollout_maze (RRL_FAST_EVAL=1 with RRL_FAST_EVAL_MAZE=1).

    python profiles/eval_rollout.py [--envs 4096] [--repeats 7] [--out profiles/eval_rollout.json]
    python profiles/eval_rollout.py --env maze --out profiles/eval_rollout_maze.json

Two measurements:
  * ONE evaluation, warm (one untimed call first), repeated: wall clock around the call with a device synchronisation on both
    sides; median, min and max per path.  The same experiment, the same weights (a few dozen training iterations first), the
    paths alternated; the switch is read per call.
  * the wall-clock share of evaluation in a run: `--eval True` against `--eval ""` with the same budget (just past 20
    episodes per env: two evaluations), on either path -- four runs, each timed around Experiment.run().
Not run by any test.  No number is claimed without the file it writes."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import arg_utils  # noqa: E402
from recovery_rl_amd.experiment import Experiment  # noqa: E402

MF = {"navigation1": ["--use_recovery", "--MF_recovery", "--gamma_safe", "0.8", "--eps_safe", "0.3"],
      "maze": ["--use_recovery", "--MF_recovery", "--gamma_safe", "0.5", "--eps_safe", "0.15", "--pos_fraction", "0.3"]}
ENV = "navigation1"


def cfg(envs, logdir, extra=()):
    return arg_utils.get_args(["--env-name", ENV, "--cuda", "--hidden_size", "256", "--num_envs", str(envs),
                               "--seed", "1", "--num_unsafe_transitions", "4000", "--logdir", logdir] + MF[ENV] + list(extra))


def set_path(path):
    for switch in ("RRL_FAST_EVAL", "RRL_FAST_EVAL_MAZE"):
        if path == "hip":
            os.environ[switch] = "1"
        else:
            os.environ.pop(switch, None)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def spread(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "samples_ms": ms}


def one_evaluation(envs, repeats, tmp):
    exp = Experiment(cfg(envs, os.path.join(tmp, "one")))
    exp.pretrain_critic_recovery()
    exp.loop.start()
    for _ in range(40):
        exp.loop.vector_step(do_update=len(exp.memory) > exp.exp_cfg.batch_size,
                             random_actions=exp.exp_cfg.start_steps > exp.loop.total_numsteps,
                             online_qrisk=exp.online_qrisk_enabled())
    out = {}
    for path in ("modules", "hip"):                       # warm both
        set_path(path)
        exp.get_test_rollout_vectorized(0)
    samples = {"modules": [], "hip": []}
    for _ in range(repeats):
        for path in ("modules", "hip"):
            set_path(path)
            samples[path].append(timed(lambda: exp.get_test_rollout_vectorized(0)))
    for path, ms in samples.items():
        out[path] = spread(ms)
    out["ratio_of_medians"] = out["modules"]["median_ms"] / out["hip"]["median_ms"]
    return out


def run_share(envs, tmp):
    budget = ["--log_every", "100", "--num_eps", "100000", "--num_steps", str(envs * 2100 - 1)]
    out = {}
    for path in ("modules", "hip"):
        set_path(path)
        for name, flag in (("eval", "True"), ("no_eval", "")):
            exp = Experiment(cfg(envs, os.path.join(tmp, path + "_" + name), budget + ["--eval", flag]))
            out["%s_%s_s" % (path, name)] = timed(exp.run) / 1e3
        out[path + "_eval_share"] = 1.0 - out[path + "_no_eval_s"] / out[path + "_eval_s"]
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--env", choices=sorted(MF), default=ENV)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eval_rollout.json"))
    a = ap.parse_args()
    ENV = a.env
    with tempfile.TemporaryDirectory() as tmp:
        result = {"env": a.env, "envs": a.envs, "device": torch.cuda.get_device_name(0), "one_evaluation": one_evaluation(a.envs, a.repeats, tmp),
                  "run_share": run_share(a.envs, tmp)}
    set_path("modules")
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result))
