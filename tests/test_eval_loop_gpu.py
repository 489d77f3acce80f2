"""Policy evaluation on the rollout kernel inside the experiment (RRL_FAST_EVAL=1): the solo evaluation, evaluation as an
observer of the training state, evaluation across a checkpoint, the module-code path it replaces (that path's first test),
and the evaluation of packed seeds (`run_packed`), whose `eval_stats` equal their solo runs'.  128 envs, hidden 256,
Navigation 1."""
import os
import pickle

import numpy as np
import pytest
import torch

import arg_utils
from recovery_rl_amd import checkpoint
from recovery_rl_amd.env.navigation import NavigationVecEnv
from recovery_rl_amd.experiment import Experiment, run_packed, uses_constraint_buffer

pytestmark = pytest.mark.gpu

MF = ["--use_recovery", "--MF_recovery"]
KEYS = {"label", "avg_reward", "success_rate", "violation_rate"}


def _cfg(tmp, flags=MF, extra=()):
    return arg_utils.get_args(["--env-name", "navigation1", "--cuda", "--hidden_size", "256", "--num_envs", "128", "--seed", "4",
                               "--gamma_safe", "0.8", "--eps_safe", "0.3", "--num_unsafe_transitions", "3000",
                               "--critic_safe_pretraining_steps", "30", "--log_every", "20", "--num_eps", "100000",
                               "--logdir", str(tmp)] + list(flags) + list(extra))


def make(tmp, flags=MF):
    exp = Experiment(_cfg(tmp, flags))
    if uses_constraint_buffer(exp.exp_cfg):
        exp.pretrain_critic_recovery()
    exp.loop.start()
    return exp


def iterate(exp, k):
    cfg, loop = exp.exp_cfg, exp.loop
    for _ in range(k):
        loop.vector_step(do_update=len(exp.memory) > cfg.batch_size, random_actions=cfg.start_steps > loop.total_numsteps,
                         online_qrisk=exp.online_qrisk_enabled() if uses_constraint_buffer(cfg) else False)


def _diff(a, b, path=""):
    """Paths at which two checkpoint trees differ."""
    if isinstance(a, dict):
        if set(a) != set(b):
            return [path + ": keys %s" % sorted(set(a) ^ set(b))]
        return [d for k in a for d in _diff(a[k], b[k], path + "/" + str(k))]
    if isinstance(a, (list, tuple)):
        if len(a) != len(b):
            return [path + ": length %d vs %d" % (len(a), len(b))]
        return [d for i, (x, y) in enumerate(zip(a, b)) for d in _diff(x, y, path + "/%d" % i)]
    if torch.is_tensor(a):
        return [] if a.shape == b.shape and torch.equal(a, b) else [path]
    if isinstance(a, np.ndarray):
        return [] if a.shape == b.shape and a.tobytes() == b.tobytes() else [path]
    return [] if a == b else [path + ": %r vs %r" % (a, b)]


def in_range(out, label):
    assert set(out) == KEYS and out["label"] == label
    assert np.isfinite(out["avg_reward"]) and out["avg_reward"] < 0.0           # every step costs the distance to the goal
    assert 0.0 <= out["success_rate"] <= 1.0 and 0.0 <= out["violation_rate"] <= 1.0


@pytest.mark.parametrize("flags", [MF, []], ids=["mf_recovery", "no_recovery"])
def test_solo_evaluation_is_one_launch_on_the_eval_env(monkeypatch, tmp_path, flags):
    monkeypatch.setenv("RRL_FAST_EVAL", "1")
    exp = make(tmp_path, flags)
    iterate(exp, 12)
    assert "evaluation" not in exp.vector_rules
    out = exp.get_test_rollout_vectorized(7)
    in_range(out, 7)
    assert exp.vector_rules["evaluation"] == "hip"
    env, horizon = exp.eval_env(), exp.eval_env()._max_episode_steps
    assert env.tick.tolist() == [horizon + 2, 0]
    steps = exp.eval_rollout().steps.cpu().numpy()
    assert steps.min() >= 1 and steps.max() <= horizon + 1
    # rows that neither succeeded nor violated ran all horizon + 1 steps
    done = (exp.eval_rollout().success | exp.eval_rollout().violation).bool().cpu().numpy()
    assert (steps[~done] == horizon + 1).all()
    in_range(exp.get_test_rollout_vectorized(8), 8)
    assert env.tick.tolist() == [2 * (horizon + 2), 0]
    if flags:
        exp._apply_demo_share()                              # the rebuild of vector_rules carries the key
        assert exp.vector_rules["evaluation"] == "hip"


def test_evaluation_is_an_observer(monkeypatch, tmp_path):
    """K iterations with an evaluation in the middle leave env state, both replay rings, every network's parameters and
    moments, the noise tick and the loop's action generator as K iterations without it do."""
    monkeypatch.setenv("RRL_FAST_EVAL", "1")
    a, b = make(tmp_path / "a"), make(tmp_path / "b")
    iterate(a, 6)
    a.get_test_rollout_vectorized(0)
    iterate(a, 6)
    iterate(b, 12)
    sa, sb = checkpoint.experiment_state(a), checkpoint.experiment_state(b)
    assert "eval_env" in sa and "eval_env" not in sb
    del sa["eval_env"]
    assert {"agent", "memory", "recovery_memory", "env", "loop", "rng"} <= set(sa)
    assert "noise_tick" in sa["agent"] and "loop_actions" in sa["rng"]
    d = _diff(sa, sb)
    assert not d, "\n".join(d)


def test_evaluation_continues_across_a_checkpoint(monkeypatch, tmp_path):
    monkeypatch.setenv("RRL_FAST_EVAL", "1")
    exp = make(tmp_path / "a")
    iterate(exp, 12)
    exp.get_test_rollout_vectorized(0)
    ck = checkpoint.save(exp, str(tmp_path / "ck.pt"))
    want = exp.get_test_rollout_vectorized(1)
    fresh = Experiment(_cfg(tmp_path / "b"))
    checkpoint.load(fresh, ck)
    got = fresh.get_test_rollout_vectorized(1)
    assert got == want and fresh.vector_rules["evaluation"] == "hip"


def test_module_path_without_the_switch_and_the_same_start_states(monkeypatch, tmp_path):
    monkeypatch.delenv("RRL_FAST_EVAL", raising=False)
    exp = make(tmp_path)
    iterate(exp, 12)
    out = exp.get_test_rollout_vectorized(3)
    in_range(out, 3)
    assert "evaluation" not in exp.vector_rules and exp.eval_rollout() is None
    env = exp.eval_env()
    horizon = env._max_episode_steps
    assert env.tick.tolist() == [horizon + 2, 0]               # the tick the kernel path advances by as well
    # the start states the eager path saw: the env's reset() at its seed and tick 0 ...
    twin = NavigationVecEnv("navigation1", 128, device=env.device, seed=env.seed_value, auto_reset=False)
    twin.reset()
    want = twin.pos.cpu().numpy()
    # ... and the kernel's at the same seed and tick
    monkeypatch.setenv("RRL_FAST_EVAL", "1")
    rollout = exp.eval_rollout()
    env.tick.zero_()
    tr_pos = torch.zeros(horizon + 1, 128, 2, dtype=torch.float64, device=env.device)
    rollout.launch(horizon + 1, trace={"tr_pos": tr_pos})
    assert tr_pos[0].cpu().numpy().tobytes() == want.tobytes()
    assert env.tick.tolist() == [horizon + 2, 0]
    assert exp.vector_rules["evaluation"] == "hip"
    monkeypatch.delenv("RRL_FAST_EVAL")                       # the switch is read per evaluation, not latched by the first
    assert exp.eval_rollout() is None
    in_range(exp.get_test_rollout_vectorized(4), 4)
    assert "evaluation" not in exp.vector_rules               # the rule follows the path the last evaluation took


def _stats(logdir):
    return pickle.load(open(os.path.join(logdir, "run_stats.pkl"), "rb"))


def test_packed_seeds_evaluate_as_their_solo_runs(monkeypatch, tmp_path):
    """`--seeds_per_gpu 2 --eval True` with a budget just past 10 episodes per env: every seed's eval_stats is non-empty and
    equals the list its solo run writes under the same switch; without the switch packed runs write the empty list."""
    budget = ["--eval", "True", "--log_every", "100", "--num_steps", str(128 * 1100 - 1)]
    monkeypatch.setenv("RRL_FAST_EVAL", "1")
    run_packed(_cfg(tmp_path / "packed", MF, budget + ["--seeds_per_gpu", "2"]))
    dirs = sorted(os.listdir(tmp_path / "packed"))
    got = [_stats(tmp_path / "packed" / d) for d in dirs]
    assert len(got) == 2 and all(g["eval_stats"] and g["vector_rules"]["evaluation"] == "hip" for g in got)
    assert got[0]["eval_stats"] != got[1]["eval_stats"]
    for d, g, seed in zip(dirs, got, (4, 5)):
        solo = Experiment(_cfg(tmp_path / ("solo%d" % seed), MF, budget + ["--seed", str(seed)]))
        solo.run()
        want = _stats(solo.logdir)
        assert d.endswith("_seed%d" % seed) and want["vector_rules"]["evaluation"] == "hip"
        assert len(g["eval_stats"]) == len(want["eval_stats"]) >= 1
        for a, b in zip(g["eval_stats"], want["eval_stats"]):
            assert a == b
            in_range(a, a["label"])
    monkeypatch.delenv("RRL_FAST_EVAL")
    run_packed(_cfg(tmp_path / "off", MF, budget + ["--seeds_per_gpu", "2"]))
    for d in os.listdir(tmp_path / "off"):
        off = _stats(tmp_path / "off" / d)
        assert off["eval_stats"] == [] and "evaluation" not in off["vector_rules"]
