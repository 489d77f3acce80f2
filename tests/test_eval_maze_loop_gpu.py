"""Maze evaluation on the rollout kernel inside the experiment (RRL_FAST_EVAL=1 with RRL_FAST_EVAL_MAZE=1): the solo
evaluation, evaluation as an observer of the training state, the module-code path that either switch alone keeps, and the
evaluation of packed seeds (`run_packed`), whose `eval_stats` equal their solo runs'.  128 envs, hidden 256, the flags of
BASELINE config 3."""
import os

import numpy as np
import pytest
import torch

import arg_utils
from recovery_rl_amd import checkpoint
from recovery_rl_amd.env.maze import MazeVecEnv
from recovery_rl_amd.experiment import Experiment, run_packed, uses_constraint_buffer
from test_eval_loop_gpu import KEYS, MF, _diff, _stats, iterate

pytestmark = pytest.mark.gpu


def _cfg(tmp, flags=MF, extra=()):
    return arg_utils.get_args(["--env-name", "maze", "--cuda", "--hidden_size", "256", "--num_envs", "128", "--seed", "4",
                               "--gamma_safe", "0.5", "--eps_safe", "0.15", "--pos_fraction", "0.3",
                               "--num_unsafe_transitions", "3000", "--critic_safe_pretraining_steps", "30",
                               "--log_every", "20", "--num_eps", "100000", "--logdir", str(tmp)] + list(flags) + list(extra))


def make(tmp, flags=MF):
    exp = Experiment(_cfg(tmp, flags))
    if uses_constraint_buffer(exp.exp_cfg):
        exp.pretrain_critic_recovery()
    exp.loop.start()
    return exp


def both(monkeypatch):
    monkeypatch.setenv("RRL_FAST_EVAL", "1")
    monkeypatch.setenv("RRL_FAST_EVAL_MAZE", "1")


def in_range(out, label):
    assert set(out) == KEYS and out["label"] == label
    assert np.isfinite(out["avg_reward"]) and out["avg_reward"] < 0.0           # every step costs the distance to the goal
    assert 0.0 <= out["success_rate"] <= 1.0 and 0.0 <= out["violation_rate"] <= 1.0


@pytest.mark.parametrize("flags", [MF, []], ids=["mf_recovery", "no_recovery"])
def test_solo_evaluation_is_one_launch_on_the_eval_env(monkeypatch, tmp_path, flags):
    both(monkeypatch)
    exp = make(tmp_path, flags)
    iterate(exp, 12)
    assert "evaluation" not in exp.vector_rules
    out = exp.get_test_rollout_vectorized(7)
    in_range(out, 7)
    assert exp.vector_rules["evaluation"] == "hip"
    env = exp.eval_env()
    horizon = env._max_episode_steps
    assert isinstance(env, MazeVecEnv) and horizon == env.horizon == 100
    assert env.tick.tolist() == [horizon + 2, 0]               # reset() and the reference's horizon + 1 step() calls
    rollout = exp.eval_rollout()
    steps = rollout.steps.cpu().numpy()
    assert steps.min() >= 1 and steps.max() <= horizon         # the env's own horizon ends a row: the last step is never taken
    done = (rollout.success | rollout.violation).bool().cpu().numpy()
    assert (steps[~done] == horizon).all()                     # rows with neither flag ran exactly `horizon` steps
    in_range(exp.get_test_rollout_vectorized(8), 8)
    assert env.tick.tolist() == [2 * (horizon + 2), 0]


def test_evaluation_is_an_observer(monkeypatch, tmp_path):
    """K iterations with an evaluation in the middle leave env state, both replay rings, every network's parameters and
    moments, the noise tick and the loop's action generator as K iterations without it do."""
    both(monkeypatch)
    a, b = make(tmp_path / "a"), make(tmp_path / "b")
    iterate(a, 6)
    a.get_test_rollout_vectorized(0)
    iterate(a, 6)
    iterate(b, 12)
    sa, sb = checkpoint.experiment_state(a), checkpoint.experiment_state(b)
    assert "eval_env" in sa and "eval_env" not in sb
    del sa["eval_env"]
    assert {"agent", "memory", "recovery_memory", "env", "loop", "rng"} <= set(sa)
    d = _diff(sa, sb)
    assert not d, "\n".join(d)


def test_module_path_with_one_switch_and_the_same_start_states(monkeypatch, tmp_path):
    monkeypatch.setenv("RRL_FAST_EVAL", "1")                   # alone: Maze stays module code
    monkeypatch.delenv("RRL_FAST_EVAL_MAZE", raising=False)
    exp = make(tmp_path)
    iterate(exp, 12)
    out = exp.get_test_rollout_vectorized(3)
    in_range(out, 3)
    assert "evaluation" not in exp.vector_rules and exp.eval_rollout() is None
    env = exp.eval_env()
    horizon = env._max_episode_steps
    assert env.tick.tolist() == [horizon + 2, 0]               # the tick the kernel path advances by as well
    # the start states the eager path saw: the env's reset() at its seed and tick 0 ...
    twin = MazeVecEnv("maze", 128, device=env.device, seed=env.seed_value, auto_reset=False)
    twin.reset()
    want = twin.pos.cpu().numpy()
    # ... and the kernel's at the same seed and tick
    monkeypatch.setenv("RRL_FAST_EVAL_MAZE", "1")
    rollout = exp.eval_rollout()
    env.tick.zero_()
    tr_pos = torch.zeros(horizon + 1, 128, 2, dtype=torch.float64, device=env.device)
    rollout.launch(horizon + 1, trace={"tr_pos": tr_pos})
    assert tr_pos[0].cpu().numpy().tobytes() == want.tobytes()
    assert env.tick.tolist() == [horizon + 2, 0]
    assert exp.vector_rules["evaluation"] == "hip"
    monkeypatch.delenv("RRL_FAST_EVAL")                        # the new switch alone: module code again, read per evaluation
    assert exp.eval_rollout() is None
    in_range(exp.get_test_rollout_vectorized(4), 4)
    assert "evaluation" not in exp.vector_rules


def test_packed_seeds_evaluate_as_their_solo_runs(monkeypatch, tmp_path):
    """`--seeds_per_gpu 2 --eval True` with a budget just past 10 episodes per env: every seed's eval_stats is non-empty and
    equals the list its solo run writes under the same switches; with the new switch unset packed Maze runs write the empty
    list, as before."""
    budget = ["--eval", "True", "--log_every", "100", "--num_steps", str(128 * 1100 - 1)]
    both(monkeypatch)
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
    monkeypatch.delenv("RRL_FAST_EVAL_MAZE")
    run_packed(_cfg(tmp_path / "off", MF, budget + ["--seeds_per_gpu", "2"]))
    for d in os.listdir(tmp_path / "off"):
        off = _stats(tmp_path / "off" / d)
        assert off["eval_stats"] == [] and "evaluation" not in off["vector_rules"]
