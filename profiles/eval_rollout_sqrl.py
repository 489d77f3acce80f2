"""Evaluation of SQRL (--use_constraint_sampling, scripts/navigation1.sh's flags) at 4096 envs, Navigation 1, hidden 256: the
module path (Experiment.get_test_rollout_vectorized as the parent commit runs it: horizon + 1 x SAC._sqrl_action, which runs
the policy and the twin Q_risk on n x 100 expanded rows on every step and draws a torch.multinomial, + env.step) against the
rrl_eval_rollout_sqrl kernel path (RRL_FAST_EVAL=1 with RRL_FAST_EVAL_SQRL=1), in one process, in the manner of
profiles/eval_rollout_qsample.py.

    python profiles/eval_rollout_sqrl.py [--envs 4096] [--repeats 5] [--packed 2,4] [--out profiles/eval_rollout_sqrl.json]

The kernel scores 100 candidates for every LIVE (row, step) pair, so its time follows the episode lengths; every setting
reports the live pairs and the shares of the pick's three branches (from the kernel's own trace) next to its times:
  * fresh       a freshly initialised agent at the run's eps_safe (0.3);
  * pretrained  the same run after pretrain_critic_recovery and a few dozen training iterations.
ONE evaluation per sample, warm (one untimed call per path first), the paths alternated, the switch read per call.  Timed
with device events around the call (the call ends with the host reading the three means, so the events span the whole
evaluation) and with the wall clock between two device synchronisations; median, min and max of the repeats per path.
--packed: the launch of S evaluations side by side (rrl_eval_rollout_sqrl_packed through eval_rollouts_packed: S rollouts on
the pretrained agent's weights, each with its own eval env and seed) against the S solo launches one after another, the same
way.
--f16x3: ONLY the f16x3 leg -- rrl_eval_rollout_sqrl_f16x3 (EvalRollout(f16x3=True), its rrl_w2_pack_f16x3 call included)
against rrl_eval_rollout_sqrl of the same build, on the same eval env from the same tick, the two entries alternated over
three rounds of --repeats samples each; written into the "sqrl" section of profiles/eval_rollout_f16x3.json.
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
from recovery_rl_amd.env import make_vec_env  # noqa: E402
from recovery_rl_amd.experiment import Experiment  # noqa: E402
from recovery_rl_amd.fast_update import EvalRollout, eval_rollouts_packed  # noqa: E402

SQRL = ["--DGD_constraints", "--use_constraint_sampling", "--nu", "5000", "--update_nu", "--gamma_safe", "0.8", "--eps_safe", "0.3"]
SWITCHES = ("RRL_FAST_EVAL", "RRL_FAST_EVAL_SQRL")


def cfg(envs, logdir):
    return arg_utils.get_args(["--env-name", "navigation1", "--cuda", "--hidden_size", "256", "--num_envs", str(envs),
                               "--seed", "1", "--num_unsafe_transitions", "4000", "--logdir", logdir] + SQRL)


def set_path(path):
    for switch in SWITCHES:
        if path == "hip":
            os.environ[switch] = "1"
        else:
            os.environ.pop(switch, None)


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


def shape_of_work(exp):
    """Live (row, step) pairs of one kernel evaluation, the mean episode length and the shares of the pick's branches"""
    set_path("hip")
    rollout, env = exp.eval_rollout(), exp.eval_env()
    T, n = env._max_episode_steps + 1, exp.exp_cfg.num_envs
    flags = torch.zeros(T, n, dtype=torch.uint8, device=env.device)
    nsafe = torch.full((T, n), -1, dtype=torch.int32, device=env.device)
    rollout.launch(T, trace={"tr_flags": flags, "tr_nsafe": nsafe})
    live = (flags & 1) == 1
    pairs = int(live.sum())
    ns = nsafe[live]
    return {"live_pairs": pairs, "mean_steps": pairs / n, "none_safe_share": float((ns == 0).float().mean()),
            "all_safe_share": float((ns == rollout.SQRL_K).float().mean())}


def measure(exp, repeats):
    out = {}
    for path in ("modules", "hip"):                       # warm both
        set_path(path)
        exp.get_test_rollout_vectorized(0)
    out.update(shape_of_work(exp))
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


def f16x3_leg(exp, rounds, repeats, **form):
    """One evaluation (launch + the three means) on each of the two entries, alternated, `rounds` x `repeats` samples from the
    same tick: per entry the spread over all samples and the median of every round; `form`: EvalRollout's qsample / sqrl"""
    c, env = exp.exp_cfg, exp.eval_env()
    T = env._max_episode_steps + 1
    rollouts = {name: EvalRollout(exp.agent.fast, env, c.eps_safe, c.use_recovery, f16x3=name == "f16x3", **form)
                for name in ("f32", "f16x3")}
    tick0 = env.tick.clone()

    def one(r):
        env.tick.copy_(tick0)
        r.launch(T)
        return r.stats(0)

    stats = {name: one(r) for name, r in rollouts.items()}          # warm, and what the two evaluations report
    samples = {name: [[] for _ in range(rounds)] for name in rollouts}
    for k in range(rounds):
        for _ in range(repeats):
            for name, r in rollouts.items():
                samples[name][k].append(timed(lambda: one(r))[0])
    env.tick.copy_(tick0)
    out = {name: dict(spread([x for rnd in samples[name] for x in rnd]),
                      round_medians_ms=[statistics.median(rnd) for rnd in samples[name]], stats=stats[name]) for name in rollouts}
    out["ratio_of_medians"] = out["f32"]["median_ms"] / out["f16x3"]["median_ms"]
    out["f16x3_faster_in_rounds"] = sum(a < b for a, b in zip(out["f16x3"]["round_medians_ms"], out["f32"]["round_medians_ms"]))
    return out


def write_f16x3(section, result, path=os.path.join(ROOT, "profiles", "eval_rollout_f16x3.json")):
    """`result` as the file's `section`, beside what the other line's script wrote"""
    whole = json.load(open(path)) if os.path.exists(path) else {}
    whole[section] = result
    whole["not_measured"] = ["packed launches", "Maze", "other k"]
    with open(path, "w") as f:
        json.dump(whole, f, indent=1)


def measure_packed(exp, S, repeats):
    """S evaluations on the experiment's weights, each on an eval env of its own: one packed launch against S solo launches"""
    c = exp.exp_cfg
    envs = [make_vec_env(c.env_name, c.num_envs, device=exp.device, seed=c.seed + 7919 + 31 * s, auto_reset=False) for s in range(S)]
    rollouts = [EvalRollout(exp.agent.fast, env, c.eps_safe, False, sqrl=True) for env in envs]
    T = envs[0]._max_episode_steps + 1

    def solo():
        for r in rollouts:
            r.launch(T)

    packed, alone = [], []
    for fn in (solo, lambda: eval_rollouts_packed(rollouts, T)):
        fn()                                              # warm
    for _ in range(repeats):
        alone.append(timed(solo)[0])
        packed.append(timed(lambda: eval_rollouts_packed(rollouts, T))[0])
    return {"S": S, "packed": spread(packed), "solo_one_after_another": spread(alone),
            "ratio_of_medians": statistics.median(alone) / statistics.median(packed)}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--packed", default="2,4")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eval_rollout_sqrl.json"))
    ap.add_argument("--f16x3", action="store_true")
    a = ap.parse_args()
    os.environ["RRL_FAST_BASELINES"] = "1"                # the fused update path of the SQRL line: the flat weights the kernel reads
    if a.f16x3:
        set_path("hip")
        result = {"env": "navigation1", "envs": a.envs, "candidates": 100, "device": torch.cuda.get_device_name(0), "rounds": 3,
                  "timer": "device events around EvalRollout.launch + stats(), rrl_w2_pack calls included; both entries of one build"}
        with tempfile.TemporaryDirectory() as tmp:
            exp = Experiment(cfg(a.envs, os.path.join(tmp, "run")))
            exp.loop.start()
            result["fresh"] = dict(f16x3_leg(exp, 3, a.repeats, sqrl=True), **shape_of_work(exp))
            print(json.dumps({"fresh": result["fresh"]}), flush=True)
            exp.pretrain_critic_recovery()
            for _ in range(40):
                exp.loop.vector_step(do_update=len(exp.memory) > exp.exp_cfg.batch_size,
                                     random_actions=exp.exp_cfg.start_steps > exp.loop.total_numsteps,
                                     online_qrisk=exp.online_qrisk_enabled())
            result["pretrained_plus_40_iterations"] = dict(f16x3_leg(exp, 3, a.repeats, sqrl=True), **shape_of_work(exp))
            print(json.dumps({"pretrained": result["pretrained_plus_40_iterations"]}), flush=True)
        write_f16x3("sqrl", result)
        sys.exit(0)
    result = {"env": "navigation1", "envs": a.envs, "candidates": 100, "device": torch.cuda.get_device_name(0),
              "timer": "device events around Experiment.get_test_rollout_vectorized; wall clock beside them"}
    with tempfile.TemporaryDirectory() as tmp:
        exp = Experiment(cfg(a.envs, os.path.join(tmp, "run")))
        exp.loop.start()
        result["fresh"] = measure(exp, a.repeats)
        print(json.dumps({"fresh": result["fresh"]}), flush=True)
        exp.pretrain_critic_recovery()
        for _ in range(40):
            exp.loop.vector_step(do_update=len(exp.memory) > exp.exp_cfg.batch_size,
                                 random_actions=exp.exp_cfg.start_steps > exp.loop.total_numsteps,
                                 online_qrisk=exp.online_qrisk_enabled())
        result["pretrained"] = measure(exp, a.repeats)
        print(json.dumps({"pretrained": result["pretrained"]}), flush=True)
        result["packed"] = []
        for S in [int(s) for s in a.packed.split(",") if s]:
            result["packed"].append(measure_packed(exp, S, a.repeats))
            print(json.dumps({"packed": result["packed"][-1]}), flush=True)
    set_path("modules")
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result))
