"""SQRL evaluated on the rollout kernel inside the experiment (RRL_FAST_EVAL=1 + RRL_FAST_EVAL_SQRL=1), in the manner of
test_eval_qsample_loop_gpu.py: the solo evaluation, evaluation as an observer of the training state, of the SQRL acting tick
and of every generator, the module-code path the run takes without the new switch, and the evaluation of packed seeds
(`run_packed` under RRL_PACK_SQRL=1), whose `eval_stats` equal their solo runs'.  128 envs (the size the fused path's other
loop tests run at), hidden 256, Navigation 1; the packed budget is the smallest that reaches two evaluations (20 episodes per
env)."""
import os
import pickle

import numpy as np
import pytest
import torch

import arg_utils
from recovery_rl_amd import checkpoint
from recovery_rl_amd.env.navigation import NavigationVecEnv
from recovery_rl_amd.experiment import Experiment, run_packed
from test_eval_loop_gpu import _diff, in_range, iterate

pytestmark = pytest.mark.gpu

SQRL = ["--DGD_constraints", "--use_constraint_sampling", "--nu", "5000", "--update_nu"]      # scripts/navigation1.sh


def _cfg(tmp, extra=()):
    return arg_utils.get_args(["--env-name", "navigation1", "--cuda", "--hidden_size", "256", "--num_envs", "128", "--seed", "4",
                               "--gamma_safe", "0.8", "--eps_safe", "0.3", "--num_unsafe_transitions", "3000",
                               "--critic_safe_pretraining_steps", "30", "--log_every", "20", "--num_eps", "100000",
                               "--logdir", str(tmp)] + SQRL + list(extra))


def make(tmp):
    exp = Experiment(_cfg(tmp))
    exp.pretrain_critic_recovery()
    exp.loop.start()
    return exp


def switches(monkeypatch, sqrl=True, acting=True):
    """The fused update path of the baselines (without it the SQRL line has no flat weights to read), the evaluation switches,
    and -- `acting` -- the training actions on rrl_sqrl_act, whose tick the observer test watches"""
    monkeypatch.setenv("RRL_FAST_BASELINES", "1")
    monkeypatch.setenv("RRL_FAST_EVAL", "1")
    for name, on in (("RRL_FAST_EVAL_SQRL", sqrl), ("RRL_FAST_SQRL", acting)):
        if on:
            monkeypatch.setenv(name, "1")
        else:
            monkeypatch.delenv(name, raising=False)


@pytest.mark.parametrize("acting", [True, False])
def test_solo_evaluation_is_one_launch_on_the_eval_env(monkeypatch, tmp_path, acting):
    switches(monkeypatch, acting=acting)                     # RRL_FAST_SQRL plays no part in the evaluation path
    exp = make(tmp_path)
    iterate(exp, 12)
    assert "evaluation" not in exp.vector_rules
    out = exp.get_test_rollout_vectorized(7)
    in_range(out, 7)
    assert exp.vector_rules["evaluation"] == "hip"
    rollout = exp.eval_rollout()
    assert rollout.sqrl and not rollout.qsample and rollout.args.k == 100
    assert rollout.args.base.rW1 is None and rollout.args.base.qW1 and rollout.args.base.pW3 == exp.agent.fast.policy.p["W3"].data_ptr()
    assert tuple(exp.agent.fast.policy.p["W3"].shape)[-2:] == (4, 256)         # the stacked head: mean rows, log_std rows
    assert abs(rollout.args.base.eps_safe - 0.3) < 1e-7
    env, horizon = exp.eval_env(), exp.eval_env()._max_episode_steps
    T = horizon + 1
    assert env.tick.tolist() == [horizon + 2, 0]
    steps = rollout.steps.cpu().numpy()
    assert steps.min() >= 1 and steps.max() <= T
    done = (rollout.success | rollout.violation).bool().cpu().numpy()
    assert (steps[~done] == T).all()
    # eval_stats is the fold of a traced launch from the same tick
    env.tick.zero_()
    dev = env.device
    rew = torch.zeros(T, 128, dtype=torch.float32, device=dev)
    flags = torch.zeros(T, 128, dtype=torch.uint8, device=dev)
    pick = torch.full((T, 128), -1, dtype=torch.int32, device=dev)
    nsafe = torch.full((T, 128), -1, dtype=torch.int32, device=dev)
    rollout.launch(T, trace={"tr_reward": rew, "tr_flags": flags, "tr_pick": pick, "tr_nsafe": nsafe})
    assert env.tick.tolist() == [horizon + 2, 0]
    f, r = flags.cpu().numpy(), rew.cpu().numpy()
    live = f & 1 == 1
    ret = np.zeros(128, np.float32)
    for j in range(T):
        ret = np.where(live[j], ret + r[j], ret).astype(np.float32)
    assert rollout.ret.cpu().numpy().tobytes() == ret.tobytes() and np.array_equal(rollout.steps.cpu().numpy(), live.sum(0))
    succ, viol = (live & (f >> 3 & 1 == 1)).any(0), (live & (f >> 2 & 1 == 1)).any(0)
    assert out["avg_reward"] == float(torch.tensor(ret, device=dev).mean().item())
    assert out["success_rate"] == float(torch.tensor(succ, device=dev).float().mean().item())
    assert out["violation_rate"] == float(torch.tensor(viol, device=dev).float().mean().item())
    # every live pair picked among its 100 candidates, none was gated, dead pairs were left alone
    p, ns = pick.cpu().numpy(), nsafe.cpu().numpy()
    assert ((p[live] >= 0) & (p[live] < 100)).all() and (p[~live] == -1).all() and ((f[live] >> 4) == 0).all()
    assert ((ns[live] >= 0) & (ns[live] <= 100)).all()
    print("live pairs %d, of them with no safe candidate %.3f, with all safe %.3f"
          % (live.sum(), (ns[live] == 0).mean(), (ns[live] == 100).mean()))
    in_range(exp.get_test_rollout_vectorized(8), 8)
    assert env.tick.tolist() == [2 * (horizon + 2), 0]


def test_evaluation_is_an_observer(monkeypatch, tmp_path):
    """K iterations with an evaluation in the middle leave env state, both replay rings, every network's parameters and
    moments, the noise tick, the SQRL acting tick, the loop's action generator and torch's generators as K iterations without
    it do -- and the evaluation itself leaves torch's global generators (CPU and device) where they were."""
    switches(monkeypatch)
    a = make(tmp_path / "a")
    assert a.loop.sqrl_hip
    iterate(a, 6)
    torch.cuda.synchronize()
    before = (torch.get_rng_state().clone(), torch.cuda.get_rng_state().clone())
    tick = a.loop.sqrl_actor().sqrl_tick.clone()
    a.get_test_rollout_vectorized(0)
    torch.cuda.synchronize()
    assert torch.equal(before[0], torch.get_rng_state()) and torch.equal(before[1], torch.cuda.get_rng_state())
    assert torch.equal(tick, a.loop.sqrl_actor().sqrl_tick) and int(tick[0]) > 0
    assert a.vector_rules["evaluation"] == "hip"
    iterate(a, 6)
    sa = checkpoint.experiment_state(a)
    b = make(tmp_path / "b")
    iterate(b, 12)
    sb = checkpoint.experiment_state(b)
    assert "eval_env" in sa and "eval_env" not in sb
    del sa["eval_env"]
    assert {"agent", "memory", "recovery_memory", "env", "loop", "rng"} <= set(sa) and "sqrl_tick" in sa["loop"]
    d = _diff(sa, sb)
    assert not d, "\n".join(d)


def test_module_path_without_the_new_switch_and_the_same_start_states(monkeypatch, tmp_path):
    switches(monkeypatch, sqrl=False)
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
    monkeypatch.setenv("RRL_FAST_EVAL_SQRL", "1")
    rollout = exp.eval_rollout()
    assert rollout is not None and rollout.sqrl
    env.tick.zero_()
    tr_pos = torch.zeros(horizon + 1, 128, 2, dtype=torch.float64, device=env.device)
    rollout.launch(horizon + 1, trace={"tr_pos": tr_pos})
    assert tr_pos[0].cpu().numpy().tobytes() == want.tobytes()
    assert env.tick.tolist() == [horizon + 2, 0]
    assert exp.vector_rules["evaluation"] == "hip"
    monkeypatch.delenv("RRL_FAST_EVAL_SQRL")                  # the switch is read per evaluation, not latched by the first
    assert exp.eval_rollout() is None
    in_range(exp.get_test_rollout_vectorized(4), 4)
    assert "evaluation" not in exp.vector_rules


def _stats(logdir):
    return pickle.load(open(os.path.join(logdir, "run_stats.pkl"), "rb"))


def test_packed_seeds_evaluate_as_their_solo_runs(monkeypatch, tmp_path):
    """`--seeds_per_gpu 2 --eval True` on the SQRL line (RRL_PACK_SQRL=1, RRL_FAST_SQRL=1, RRL_FAST_BASELINES=1) with a budget
    just past 20 episodes per env: every seed's eval_stats holds two evaluations and equals the list its solo run writes under
    the same switches."""
    budget = ["--eval", "True", "--log_every", "100", "--num_steps", str(128 * 2200 - 1)]
    switches(monkeypatch)
    monkeypatch.setenv("RRL_PACK_SQRL", "1")
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


def test_packed_run_without_the_new_switch_writes_empty_eval_stats(monkeypatch, tmp_path):
    """... and without RRL_FAST_EVAL_SQRL a packed SQRL run does not evaluate, as before"""
    switches(monkeypatch, sqrl=False)
    monkeypatch.setenv("RRL_PACK_SQRL", "1")
    run_packed(_cfg(tmp_path, ["--eval", "True", "--num_steps", str(128 * 40 - 1), "--seeds_per_gpu", "2"]))
    for d in sorted(os.listdir(tmp_path)):
        rs = _stats(tmp_path / d)
        assert rs["eval_stats"] == [] and "evaluation" not in rs["vector_rules"]
