"""f16x3 evaluation scoring inside the experiment (RRL_EVAL_SQRL_F16X3=1 / RRL_EVAL_QSAMPLE_F16X3=1 on top of the line's two
evaluation switches), in the manner of test_eval_sqrl_loop_gpu.py / test_eval_qsample_loop_gpu.py, whose configurations,
switches and helpers these tests use: the solo evaluation is one launch of the new entry, the run without the new switch is
the parent's, an evaluation under the switch is an observer, packed seeds evaluate as their solo runs, and a resume across
different evaluation scoring warns and continues."""
import os
import pickle

import pytest
import torch

import test_eval_qsample_loop_gpu as QL
import test_eval_sqrl_loop_gpu as SL
from recovery_rl_amd import _lib, fast_update
from recovery_rl_amd.experiment import Experiment, run_packed
from recovery_rl_amd.fast_update import EvalRollout
from test_eval_loop_gpu import in_range, iterate

pytestmark = pytest.mark.gpu

# line -> (the existing loop test module, the new switch, the f32 entry, the pack switch)
LINES = {"sqrl": (SL, "RRL_EVAL_SQRL_F16X3", "rrl_eval_rollout_sqrl", "RRL_PACK_SQRL"),
         "qsample": (QL, "RRL_EVAL_QSAMPLE_F16X3", "rrl_eval_rollout_qs", "RRL_PACK_QSAMPLE")}


def switches(monkeypatch, line, on=True, acting=False):
    """The line's own switches (its evaluation on the rollout kernel; `acting`: its training actions on the acting kernel),
    then the new one"""
    mod, new, _, _ = LINES[line]
    mod.switches(monkeypatch, acting=acting)
    if on:
        monkeypatch.setenv(new, "1")
    else:
        monkeypatch.delenv(new, raising=False)


def record_entries(monkeypatch):
    """The names of the library calls that go through _lib.check, in order"""
    calls, real = [], _lib.check
    monkeypatch.setattr(_lib, "check", lambda rc, what: (calls.append(what), real(rc, what))[1])
    return calls


def _stats(logdir):
    return pickle.load(open(os.path.join(logdir, "run_stats.pkl"), "rb"))


@pytest.mark.parametrize("line", list(LINES))
def test_switch_on_solo_evaluation_is_one_launch_of_the_new_entry(monkeypatch, tmp_path, line):
    mod, new, f32, _ = LINES[line]
    switches(monkeypatch, line)
    exp = mod.make(tmp_path)
    cfg = exp.exp_cfg
    assert fast_update.eval_rollout_path(cfg) == "hip" and fast_update.eval_scoring(cfg) == "f16x3"
    assert exp.eval_f16x3_switches == (line == "sqrl", line == "qsample")
    monkeypatch.delenv(new)                                  # read once, when the loop was built: the evaluations below keep it
    iterate(exp, 12)
    assert "evaluation" not in exp.vector_rules and "evaluation_scoring" not in exp.vector_rules
    calls = record_entries(monkeypatch)
    out = exp.get_test_rollout_vectorized(7)
    in_range(out, 7)
    assert [c for c in calls if c.startswith("rrl_eval_rollout")] == [f32 + "_f16x3"] and calls.count("rrl_w2_pack_f16x3") == 1
    assert calls.index("rrl_w2_pack_f16x3") < calls.index(f32 + "_f16x3")               # the stream is made right before the launch
    assert exp.vector_rules["evaluation"] == "hip" and exp.vector_rules["evaluation_scoring"] == "f16x3"
    rollout = exp.eval_rollout()
    assert rollout.f16x3 and rollout.qw2h is not None and bool(torch.isfinite(rollout.qw2h).all())
    assert rollout.sqrl == (line == "sqrl") and rollout.qsample == (line == "qsample")
    env, horizon = exp.eval_env(), exp.eval_env()._max_episode_steps
    assert env.tick.tolist() == [horizon + 2, 0]
    # eval_stats is the stats() of a hand-made launch from the same weights, seed and tick
    env.tick.zero_()
    hand = EvalRollout(exp.agent.fast, env, cfg.eps_safe, cfg.use_recovery, qsample=line == "qsample", sqrl=line == "sqrl",
                       f16x3=True)
    hand.launch(horizon + 1)
    assert hand.stats(7) == out and env.tick.tolist() == [horizon + 2, 0]
    for name in ("ret", "success", "violation", "steps"):
        assert torch.equal(getattr(hand, name), getattr(rollout, name)), name
    # ... and it is not the f32 launch: same start, other scores (the results may or may not differ; the launch does)
    env.tick.zero_()
    plain = EvalRollout(exp.agent.fast, env, cfg.eps_safe, cfg.use_recovery, qsample=line == "qsample", sqrl=line == "sqrl")
    assert not plain.f16x3 and plain.qw2h is None
    T = horizon + 1
    q32 = torch.zeros(T, 128, device=env.device)
    plain.launch(T, trace={"tr_q": q32})
    env.tick.zero_()
    q16 = torch.zeros(T, 128, device=env.device)
    hand.launch(T, trace={"tr_q": q16})
    assert not torch.equal(q32, q16) and bool((q16[0] - q32[0]).abs().max() < 1e-4)     # (step 0: the same states and draws)
    with pytest.raises(_lib.RRLError):
        fast_update.eval_rollouts_packed([hand, plain], T)                              # a mix of scorings in one call
    # a solo run under the switches records the scoring in run_stats.pkl and in its checkpoint
    monkeypatch.setenv(new, "1")
    run = Experiment(mod._cfg(tmp_path / "run", ["--num_steps", str(128 * 20)]))
    run.get_test_rollout_vectorized(0)                       # (the run is too short to reach its own first evaluation)
    run.run()
    for rules in (_stats(run.logdir)["vector_rules"],
                  torch.load(os.path.join(run.logdir, "checkpoint.pt"), map_location="cpu", weights_only=False)["extra"]["vector_rules"]):
        assert rules["evaluation"] == "hip" and rules["evaluation_scoring"] == "f16x3"


@pytest.mark.parametrize("line", list(LINES))
def test_switch_off_is_the_parents_run(monkeypatch, tmp_path, line):
    mod, new, f32, _ = LINES[line]
    outs = []
    for tag, value in (("unset", None), ("zero", "0"), ("never", None)):
        switches(monkeypatch, line, on=False)
        if value is not None:
            monkeypatch.setenv(new, value)
        exp = mod.make(tmp_path / tag)
        iterate(exp, 12)
        if tag == "never":       # a run in which the switch was never heard of: the parent's EvalRollout, built by hand
            exp._eval_rollout = EvalRollout(exp.agent.fast, exp.eval_env(), exp.exp_cfg.eps_safe, exp.exp_cfg.use_recovery,
                                            qsample=line == "qsample", sqrl=line == "sqrl")
        assert exp.eval_f16x3_switches == (False, False)
        monkeypatch.setenv(new, "1")                         # the switch was read when the loop was built: too late now
        calls = record_entries(monkeypatch)
        outs.append(exp.get_test_rollout_vectorized(3))
        assert [c for c in calls if c.startswith("rrl_eval_rollout")] == [f32] and "rrl_w2_pack_f16x3" not in calls
        assert exp.vector_rules["evaluation"] == "hip" and exp.vector_rules["evaluation_scoring"] == "f32"
        assert not exp.eval_rollout().f16x3 and exp.eval_rollout().qw2h is None
        monkeypatch.undo()
    assert outs[0] == outs[1] == outs[2]                                                 # same seed: bit-equal floats


@pytest.mark.parametrize("line", list(LINES))
def test_evaluation_under_the_switch_is_an_observer(monkeypatch, tmp_path, line):
    """The existing observer test, restated by running it with the new switch set: loop generator, acting tick, torch
    generators and parameters are untouched."""
    mod, new, f32, _ = LINES[line]
    monkeypatch.setenv(new, "1")
    calls = record_entries(monkeypatch)
    mod.test_evaluation_is_an_observer(monkeypatch, tmp_path)
    assert f32 + "_f16x3" in calls and f32 not in calls


@pytest.mark.parametrize("line", list(LINES))
def test_packed_seeds_evaluate_as_their_solo_runs(monkeypatch, tmp_path, line):
    """`--seeds_per_gpu 2 --eval True` under the line's pack switch and the new switch: every packed seed's eval_stats and
    vector_rules equal its solo run's under the same switches; run_stats.pkl and the checkpoint record the scoring."""
    mod, new, f32, pack = LINES[line]
    budget = ["--eval", "True", "--log_every", "100", "--num_steps", str(128 * 2200 - 1)]
    switches(monkeypatch, line, acting=True)
    monkeypatch.setenv(pack, "1")
    calls = record_entries(monkeypatch)
    run_packed(mod._cfg(tmp_path / "packed", budget + ["--seeds_per_gpu", "2"]))
    assert f32 + "_f16x3_packed" in calls and f32 + "_packed" not in calls and f32 not in calls
    dirs = sorted(os.listdir(tmp_path / "packed"))
    got = [_stats(tmp_path / "packed" / d) for d in dirs]
    assert len(got) == 2 and got[0]["eval_stats"] != got[1]["eval_stats"]
    for d, g, seed in zip(dirs, got, (4, 5)):
        solo = Experiment(mod._cfg(tmp_path / ("solo%d" % seed), budget + ["--seed", str(seed)]))
        solo.run()
        want = _stats(solo.logdir)
        assert d.endswith("_seed%d" % seed)
        for rules in (g["vector_rules"], want["vector_rules"]):
            assert rules["evaluation"] == "hip" and rules["evaluation_scoring"] == "f16x3"
        assert g["vector_rules"] == want["vector_rules"]
        assert len(g["eval_stats"]) == len(want["eval_stats"]) >= 2
        for a, b in zip(g["eval_stats"], want["eval_stats"]):
            assert a == b
            in_range(a, a["label"])
        ck = torch.load(os.path.join(solo.logdir, "checkpoint.pt"), map_location="cpu", weights_only=False)
        assert ck["extra"]["vector_rules"]["evaluation_scoring"] == "f16x3" and ck["extra"]["evals"] == want["eval_stats"]


@pytest.mark.parametrize("line", list(LINES))
def test_resume_across_the_other_evaluation_scoring_warns_and_continues(monkeypatch, tmp_path, capsys, line):
    mod, new, f32, _ = LINES[line]
    steps = lambda iters: ["--num_steps", str(128 * iters)]
    switches(monkeypatch, line)
    part = Experiment(mod._cfg(tmp_path / "part", steps(20)))
    part.get_test_rollout_vectorized(0)                      # an observer; the rule it leaves goes into the checkpoint
    part.run()
    ck = os.path.join(part.logdir, "checkpoint.pt")
    assert torch.load(ck, map_location="cpu", weights_only=False)["extra"]["vector_rules"]["evaluation_scoring"] == "f16x3"
    capsys.readouterr()
    same = Experiment(mod._cfg(tmp_path / "same", steps(40) + ["--resume", ck]))
    same.run()
    assert "evaluation scoring" not in capsys.readouterr().out
    monkeypatch.delenv(new)
    cont = Experiment(mod._cfg(tmp_path / "cont", steps(40) + ["--resume", ck]))
    hist = cont.run()
    out = capsys.readouterr().out
    assert "WARNING: the checkpoint was written with evaluation scoring f16x3, this run continues with f32" in out
    assert hist[-1]["iteration"] >= 40 and "Resumed from" in out
    in_range(cont.get_test_rollout_vectorized(1), 1)
    assert cont.vector_rules["evaluation_scoring"] == "f32"
