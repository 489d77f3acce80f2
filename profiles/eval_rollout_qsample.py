"""Evaluation of Q-sampling recovery (--use_recovery --Q_sampling_recovery) at 4096 envs, Navigation 1, hidden 256: the module
path (Experiment.get_test_rollout_vectorized as the parent commit runs it: horizon + 1 x loop.act(train=False), which scores
n x 1000 candidate rows on every step, + env.step) against the rrl_eval_rollout_qs kernel path (RRL_FAST_EVAL=1 with
RRL_FAST_EVAL_QSAMPLE=1), in one process, in the manner of profiles/eval_rollout.py.

    python profiles/eval_rollout_qsample.py [--envs 4096] [--repeats 5] [--out profiles/eval_rollout_qsample.json]

The kernel's time follows the share of (row, step) pairs whose gate fired, so every setting reports that share (from the
kernel's own trace: flag bit 4 over the live pairs) next to its times:
  * fresh       a freshly initialised agent at the run's eps_safe (0.3);
  * pretrained  the same run after pretrain_critic_recovery and a few dozen training iterations: a gate that fires often;
  * closed      the fresh agent with eps_safe raised to 0.99: a gate that (almost) never fires -- the other end.
ONE evaluation per sample, warm (one untimed call per path first), the paths alternated, the switch read per call.  Timed
with device events around the call (the call ends with the host reading the three means, so the events span the whole
evaluation) and with the wall clock between two device synchronisations; median, min and max of the repeats per path.
--f16x3: ONLY the f16x3 leg (eval_rollout_sqrl.f16x3_leg) -- rrl_eval_rollout_qs_f16x3 against rrl_eval_rollout_qs of the same
build, alternated over three rounds, with the gate closed (eps_safe 0.99), the fresh agent at 0.3 and every row gated
(eps_safe -1); written into the "qsample" section of profiles/eval_rollout_f16x3.json.
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

QS = ["--use_recovery", "--Q_sampling_recovery", "--gamma_safe", "0.8", "--eps_safe", "0.3"]
SWITCHES = ("RRL_FAST_EVAL", "RRL_FAST_EVAL_QSAMPLE")


def cfg(envs, logdir):
    return arg_utils.get_args(["--env-name", "navigation1", "--cuda", "--hidden_size", "256", "--num_envs", str(envs),
                               "--seed", "1", "--num_unsafe_transitions", "4000", "--logdir", logdir] + QS)


def set_path(path):
    for switch in SWITCHES:
        if path == "hip":
            os.environ[switch] = "1"
        else:
            os.environ.pop(switch, None)


def set_eps(exp, eps):
    exp.exp_cfg.eps_safe = exp.loop.cfg.eps_safe = exp.agent.eps_safe = eps
    if getattr(exp, "_eval_rollout", None) is not None:
        exp._eval_rollout.eps_safe = float(eps)


def timed(fn):
    """(device ms between two events, wall ms between two synchronisations) of one call"""
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    start.record()
    fn()
    end.record()
    end.synchronize()
    wall = (time.perf_counter() - t0) * 1e3
    return start.elapsed_time(end), wall


def spread(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "samples_ms": ms}


def gated_share(exp):
    """Share of the live (row, step) pairs of one kernel evaluation whose gate fired, and the mean episode length"""
    set_path("hip")
    rollout, env = exp.eval_rollout(), exp.eval_env()
    T = env._max_episode_steps + 1
    flags = torch.zeros(T, exp.exp_cfg.num_envs, dtype=torch.uint8, device=env.device)
    rollout.launch(T, trace={"tr_flags": flags})
    live = int((flags & 1).sum())
    return {"gated_share": int(((flags >> 4) & 1).sum()) / live, "live_pairs": live, "mean_steps": live / exp.exp_cfg.num_envs}


def measure(exp, repeats):
    out = {}
    for path in ("modules", "hip"):                       # warm both
        set_path(path)
        exp.get_test_rollout_vectorized(0)
    out.update(gated_share(exp))
    samples = {"modules": ([], []), "hip": ([], [])}
    for _ in range(repeats):
        for path in ("modules", "hip"):
            set_path(path)
            assert (exp.eval_rollout() is not None) == (path == "hip")
            dev, wall = timed(lambda: exp.get_test_rollout_vectorized(0))
            samples[path][0].append(dev)
            samples[path][1].append(wall)
    for path, (dev, wall) in samples.items():
        out[path] = dict(spread(dev), wall=spread(wall))
    out["ratio_of_medians"] = out["modules"]["median_ms"] / out["hip"]["median_ms"]
    # "not slower beyond the spread of the repeats": the kernel path's slowest sample against the module path's fastest
    out["hip_max_over_modules_min"] = out["hip"]["max_ms"] / out["modules"]["min_ms"]
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eval_rollout_qsample.json"))
    ap.add_argument("--f16x3", action="store_true")
    a = ap.parse_args()
    if a.f16x3:
        from eval_rollout_sqrl import f16x3_leg, write_f16x3
        set_path("hip")
        result = {"env": "navigation1", "envs": a.envs, "candidates": 1000, "device": torch.cuda.get_device_name(0), "rounds": 3,
                  "timer": "device events around EvalRollout.launch + stats(), rrl_w2_pack calls included; both entries of one build"}
        with tempfile.TemporaryDirectory() as tmp:
            exp = Experiment(cfg(a.envs, os.path.join(tmp, "run")))
            exp.loop.start()
            for name, eps in (("gate_never_fires", 0.99), ("fresh", 0.3), ("every_row_gated", -1.0)):
                set_eps(exp, eps)
                exp._eval_rollout = None
                result[name] = dict(f16x3_leg(exp, 3, a.repeats, qsample=True), eps_safe=eps, **gated_share(exp))
                print(json.dumps({name: result[name]}), flush=True)
        write_f16x3("qsample", result)
        sys.exit(0)
    result = {"env": "navigation1", "envs": a.envs, "candidates": 1000, "device": torch.cuda.get_device_name(0),
              "timer": "device events around Experiment.get_test_rollout_vectorized; wall clock beside them"}
    with tempfile.TemporaryDirectory() as tmp:
        exp = Experiment(cfg(a.envs, os.path.join(tmp, "run")))
        exp.loop.start()
        result["fresh"] = measure(exp, a.repeats)
        print(json.dumps({"fresh": result["fresh"]}), flush=True)
        set_eps(exp, 0.99)
        result["closed"] = dict(measure(exp, a.repeats), eps_safe=0.99)
        print(json.dumps({"closed": result["closed"]}), flush=True)
        set_eps(exp, 0.3)
        exp.pretrain_critic_recovery()
        for _ in range(40):
            exp.loop.vector_step(do_update=len(exp.memory) > exp.exp_cfg.batch_size,
                                 random_actions=exp.exp_cfg.start_steps > exp.loop.total_numsteps,
                                 online_qrisk=exp.online_qrisk_enabled())
        result["pretrained"] = measure(exp, a.repeats)
    set_path("modules")
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result))
