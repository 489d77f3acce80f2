"""Q-sampling recovery evaluated on the rollout kernel inside the experiment (RRL_FAST_EVAL=1 + RRL_FAST_EVAL_QSAMPLE=1), in the
manner of test_eval_loop_gpu.py: the solo evaluation, evaluation as an observer of the training state and of both generators,
the module-code path the run takes without the new switch, and the evaluation of packed seeds (`run_packed` under
RRL_PACK_QSAMPLE=1), whose `eval_stats` equal their solo runs'.  128 envs (the size the fused path's other loop tests run
at), hidden 256, Navigation 1; the packed budget is the smallest that reaches two evaluations (20 episodes per env)."""
import os
import pickle

import pytest
import torch

import arg_utils
from recovery_rl_amd import checkpoint
from recovery_rl_amd.env.navigation import NavigationVecEnv
from recovery_rl_amd.experiment import Experiment, run_packed
from test_eval_loop_gpu import _diff, in_range, iterate

pytestmark = pytest.mark.gpu

QS = ["--use_recovery", "--Q_sampling_recovery"]


def _cfg(tmp, extra=()):
    return arg_utils.get_args(["--env-name", "navigation1", "--cuda", "--hidden_size", "256", "--num_envs", "128", "--seed", "4",
                               "--gamma_safe", "0.8", "--eps_safe", "0.3", "--num_unsafe_transitions", "3000",
                               "--critic_safe_pretraining_steps", "30", "--log_every", "20", "--num_eps", "100000",
                               "--logdir", str(tmp)] + QS + list(extra))


def make(tmp):
    exp = Experiment(_cfg(tmp))
    exp.pretrain_critic_recovery()
    exp.loop.start()
    return exp


def switches(monkeypatch, qsample=True, acting=False):
    monkeypatch.setenv("RRL_FAST_EVAL", "1")
    for name, on in (("RRL_FAST_EVAL_QSAMPLE", qsample), ("RRL_FAST_QSAMPLE", acting)):
        if on:
            monkeypatch.setenv(name, "1")
        else:
            monkeypatch.delenv(name, raising=False)


def test_solo_evaluation_is_one_launch_on_the_eval_env(monkeypatch, tmp_path):
    switches(monkeypatch)
    exp = make(tmp_path)
    iterate(exp, 12)
    assert "evaluation" not in exp.vector_rules
    out = exp.get_test_rollout_vectorized(7)
    in_range(out, 7)
    assert exp.vector_rules["evaluation"] == "hip"
    rollout = exp.eval_rollout()
    assert rollout.qsample and rollout.args.k == 1000 and rollout.args.base.rW1 is None and rollout.args.base.qW1
    assert [t.tolist() for t in rollout.box] == [[-1.0, -1.0], [1.0, 1.0]]
    env, horizon = exp.eval_env(), exp.eval_env()._max_episode_steps
    assert env.tick.tolist() == [horizon + 2, 0]
    steps = rollout.steps.cpu().numpy()
    assert steps.min() >= 1 and steps.max() <= horizon + 1
    done = (rollout.success | rollout.violation).bool().cpu().numpy()
    assert (steps[~done] == horizon + 1).all()
    in_range(exp.get_test_rollout_vectorized(8), 8)
    assert env.tick.tolist() == [2 * (horizon + 2), 0]
    # the gate fires on the way (the pretrained critic at eps_safe 0.3): the launch did draw candidates
    T = horizon + 1
    flags = torch.zeros(T, 128, dtype=torch.uint8, device=env.device)
    pick = torch.full((T, 128), -1, dtype=torch.int32, device=env.device)
    rollout.launch(T, trace={"tr_flags": flags, "tr_pick": pick})
    gated = (flags >> 4) & 1 == 1
    print("gated share of live (row, step) pairs: %.3f" % (float(gated.sum()) / float((flags & 1).sum())))
    assert torch.equal(gated, pick >= 0) and int(pick.max()) < 1000


def test_evaluation_is_an_observer(monkeypatch, tmp_path):
    """K iterations with an evaluation in the middle leave env state, both replay rings, every network's parameters and
    moments, the noise tick, the loop's action generator and torch's generators as K iterations without it do -- and the
    evaluation itself leaves torch's global generators (CPU and device) where they were.  Training acts on module code here
    (RRL_FAST_QSAMPLE unset: the evaluation kernel does not depend on it), which draws its candidates from torch's global
    generator: a draw from it by the evaluation would show in everything after it.  The two runs go one after the other,
    each seeded by its own Experiment -- this line's training shares the global generator between interleaved runs."""
    switches(monkeypatch)
    a = make(tmp_path / "a")
    iterate(a, 6)
    torch.cuda.synchronize()
    before = (torch.get_rng_state().clone(), torch.cuda.get_rng_state().clone())
    a.get_test_rollout_vectorized(0)
    torch.cuda.synchronize()
    assert torch.equal(before[0], torch.get_rng_state()) and torch.equal(before[1], torch.cuda.get_rng_state())
    assert a.vector_rules["evaluation"] == "hip"
    iterate(a, 6)
    sa = checkpoint.experiment_state(a)
    b = make(tmp_path / "b")
    iterate(b, 12)
    sb = checkpoint.experiment_state(b)
    assert "eval_env" in sa and "eval_env" not in sb
    del sa["eval_env"]
    assert {"agent", "memory", "recovery_memory", "env", "loop", "rng"} <= set(sa)
    d = _diff(sa, sb)
    assert not d, "\n".join(d)


def test_module_path_without_the_new_switch_and_the_same_start_states(monkeypatch, tmp_path):
    switches(monkeypatch, qsample=False)
    exp = make(tmp_path)
    iterate(exp, 12)
    out = exp.get_test_rollout_vectorized(3)
    in_range(out, 3)
    assert "evaluation" not in exp.vector_rules and exp.eval_rollout() is None
    env = exp.eval_env()
    horizon = env._max_episode_steps
    assert env.tick.tolist() == [horizon + 2, 0]               # the tick the kernel path advances by as well
    twin = NavigationVecEnv("navigation1", 128, device=env.device, seed=env.seed_value, auto_reset=False)
    twin.reset()
    want = twin.pos.cpu().numpy()
    monkeypatch.setenv("RRL_FAST_EVAL_QSAMPLE", "1")
    rollout = exp.eval_rollout()
    assert rollout is not None and rollout.qsample
    env.tick.zero_()
    tr_pos = torch.zeros(horizon + 1, 128, 2, dtype=torch.float64, device=env.device)
    rollout.launch(horizon + 1, trace={"tr_pos": tr_pos})
    assert tr_pos[0].cpu().numpy().tobytes() == want.tobytes()
    assert env.tick.tolist() == [horizon + 2, 0]
    assert exp.vector_rules["evaluation"] == "hip"
    monkeypatch.delenv("RRL_FAST_EVAL_QSAMPLE")               # the switch is read per evaluation, not latched by the first
    assert exp.eval_rollout() is None
    in_range(exp.get_test_rollout_vectorized(4), 4)
    assert "evaluation" not in exp.vector_rules


def _stats(logdir):
    return pickle.load(open(os.path.join(logdir, "run_stats.pkl"), "rb"))


def test_packed_seeds_evaluate_as_their_solo_runs(monkeypatch, tmp_path):
    """`--seeds_per_gpu 2 --eval True` on the Q-sampling line (RRL_PACK_QSAMPLE=1, RRL_FAST_QSAMPLE=1) with a budget just past
    20 episodes per env: every seed's eval_stats holds two evaluations and equals the list its solo run writes under the same
    switches."""
    budget = ["--eval", "True", "--log_every", "100", "--num_steps", str(128 * 2200 - 1)]
    switches(monkeypatch, acting=True)
    monkeypatch.setenv("RRL_PACK_QSAMPLE", "1")
    run_packed(_cfg(tmp_path / "packed", budget + ["--seeds_per_gpu", "2"]))
    dirs = sorted(os.listdir(tmp_path / "packed"))
    got = [_stats(tmp_path / "packed" / d) for d in dirs]
    assert len(got) == 2 and all(g["eval_stats"] and g["vector_rules"]["evaluation"] == "hip" for g in got)
    assert got[0]["eval_stats"] != got[1]["eval_stats"]
    for d, g, seed in zip(dirs, got, (4, 5)):
        solo = Experiment(_cfg(tmp_path / ("solo%d" % seed), budget + ["--seed", str(seed)]))
        solo.run()
        want = _stats(solo.logdir)
        assert d.endswith("_seed%d" % seed) and want["vector_rules"]["evaluation"] == "hip"
        assert len(g["eval_stats"]) == len(want["eval_stats"]) >= 2
        for a, b in zip(g["eval_stats"], want["eval_stats"]):
            assert a == b
            in_range(a, a["label"])
