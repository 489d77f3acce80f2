"""RRL_SQRL_F16X3=1 in the driver: the run record names the scoring, a run without the switch is the run the switch does not
exist for, a resumed run equals the uninterrupted one, a checkpoint refuses the other scoring, and every packed seed equals
its solo f16x3 run."""
import os
import pickle

import numpy as np
import pytest
import torch

import arg_utils
from recovery_rl_amd import checkpoint, fast_update
from recovery_rl_amd import packed as packed_module
from recovery_rl_amd.experiment import Experiment, run_packed
from recovery_rl_amd.packed import PackedLoop
from test_sqrl_act_cpu import SQRL
from test_sqrl_act_gpu import _diff

pytestmark = pytest.mark.gpu
ENVS = 128                               # --start_steps 100 (the default): iteration 1 acts at random
SWITCHES = ("RRL_FAST_BASELINES", "RRL_FAST_SQRL", "RRL_SQRL_F16X3")


def _cfg(tmp, iters, extra=()):
    """A run that ends by its step budget, at the first log point past `iters` iterations."""
    return arg_utils.get_args(["--env-name", "navigation1", "--cuda", "--hidden_size", "256", "--logdir", str(tmp),
                               "--seed", "5", "--num_unsafe_transitions", "2000", "--critic_safe_pretraining_steps",
                               "20", "--num_envs", str(ENVS), "--log_every", "10", "--num_steps", str(ENVS * iters),
                               "--gamma_safe", "0.8", "--eps_safe", "0.3"] + SQRL + list(extra))


def _run_stats(exp):
    return pickle.load(open(os.path.join(exp.logdir, "run_stats.pkl"), "rb"))


def test_the_run_records_its_scoring_and_without_the_switch_nothing_moved(tmp_path, monkeypatch):
    for name in SWITCHES:
        monkeypatch.setenv(name, "1")
    on = Experiment(_cfg(tmp_path / "on", 40))
    assert on.loop.sqrl_hip and on.loop.sqrl_f16x3
    assert on.vector_rules["sqrl_acting"] == "hip" and on.vector_rules["sqrl_scoring"] == "f16x3"
    iters = on.run()[-1]["iteration"]
    assert on.loop.graph is not None                      # the steady state replays the captured iteration, pack included
    actor = on.loop.sqrl_actor()
    assert actor.sqrl_f16x3 and actor.sqrl_w2h is not None and int(actor.sqrl_tick[0]) == iters - 1
    rs_on = _run_stats(on)
    assert rs_on["vector_rules"]["sqrl_acting"] == "hip" and rs_on["vector_rules"]["sqrl_scoring"] == "f16x3"
    assert bool(torch.isfinite(actor.sqrl_w2h).all())
    # without the switch: the parent's path -- rrl_sqrl_act on the fragment-order copy, no stream, no pack call
    monkeypatch.delenv("RRL_SQRL_F16X3")
    calls = []
    real = fast_update.record
    monkeypatch.setattr(fast_update, "record", lambda kind, *p: (calls.append(kind), real(kind, *p))[1])
    a = Experiment(_cfg(tmp_path / "a", 40))
    assert a.loop.sqrl_hip and not a.loop.sqrl_f16x3 and a.vector_rules["sqrl_scoring"] == "f32"
    a.run()
    assert a.loop.sqrl_actor().sqrl_w2h is None and "sqrl" in calls and "sqrl_f16x3" not in calls
    b = Experiment(_cfg(tmp_path / "b", 40))
    b.loop.sqrl_f16x3 = False                              # what a build without the switch runs
    b.run()
    rs_a, rs_b = _run_stats(a), _run_stats(b)
    assert rs_a["vector_rules"]["sqrl_scoring"] == "f32"
    for key in rs_a:
        d = _diff(rs_a[key], rs_b[key], key)
        assert not d, d
    # the f16x3 run is recorded as what it was, whether or not a decision differed within its 40 iterations
    assert rs_on["vector_rules"] != rs_a["vector_rules"]


def test_resumed_run_equals_the_uninterrupted_one_and_the_other_scoring_is_refused(tmp_path, monkeypatch):
    for name in SWITCHES:
        monkeypatch.setenv(name, "1")
    full = Experiment(_cfg(tmp_path / "full", 40))
    full.run()
    part = Experiment(_cfg(tmp_path / "part", 20))
    part.run()
    ck = os.path.join(part.logdir, "checkpoint.pt")
    mid = torch.load(ck, map_location="cpu", weights_only=False)
    assert mid["extra"]["vector_rules"]["sqrl_scoring"] == "f16x3" and mid["loop"]["sqrl_scoring"] == "f16x3"
    assert int(mid["loop"]["sqrl_tick"][0]) == mid["extra"]["iteration"] - 1      # the Philox tick: unchanged protocol
    cont = Experiment(_cfg(tmp_path / "cont", 40, ["--resume", ck]))
    cont.run()
    a = torch.load(os.path.join(full.logdir, "checkpoint.pt"), map_location="cpu", weights_only=False)
    b = torch.load(os.path.join(cont.logdir, "checkpoint.pt"), map_location="cpu", weights_only=False)
    assert a["extra"]["iteration"] == b["extra"]["iteration"] >= 40 > mid["extra"]["iteration"] >= 20
    d = _diff(a, b)
    assert not d, "\n".join(d)
    # the other scoring refuses the checkpoint and names the switch -- both ways
    monkeypatch.delenv("RRL_SQRL_F16X3")
    other = Experiment(_cfg(tmp_path / "other", 20))
    with pytest.raises(ValueError, match="RRL_SQRL_F16X3"):
        checkpoint.load(other, ck)
    other.run()
    assert torch.load(os.path.join(other.logdir, "checkpoint.pt"), map_location="cpu",
                      weights_only=False)["loop"]["sqrl_scoring"] == "f32"
    monkeypatch.setenv("RRL_SQRL_F16X3", "1")
    with pytest.raises(ValueError, match="RRL_SQRL_F16X3"):
        checkpoint.load(Experiment(_cfg(tmp_path / "back", 20)), os.path.join(other.logdir, "checkpoint.pt"))


def test_seeds_per_gpu_packs_the_f16x3_line_and_every_seed_equals_its_solo_run(tmp_path, monkeypatch):
    """The comparison of tests/test_packed_sqrl_gpu.py's driver test under the four switches: two experiments advanced by one
    shared graph whose acting stage is rrl_sqrl_act_f16x3_packed behind the two per-seed pack calls; the second seed's counters,
    log-multiplier and tick equal the solo f16x3 run of that seed stepped through the same phases."""
    for name in SWITCHES + ("RRL_PACK_SQRL",):
        monkeypatch.setenv(name, "1")
    made = []

    class Spy(PackedLoop):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            made.append(self)
    monkeypatch.setattr(packed_module, "PackedLoop", Spy)
    argv = ["--env-name", "navigation1", "--cuda"] + SQRL + ["--gamma_safe", "0.8",
            "--eps_safe", "0.3", "--num_unsafe_transitions", "3000", "--critic_safe_pretraining_steps", "30", "--num_envs",
            str(ENVS), "--log_every", "20", "--num_eps", "100000", "--num_steps", str(ENVS * 40 - 1)]
    hists = run_packed(arg_utils.get_args(argv + ["--seed", "4", "--seeds_per_gpu", "2", "--logdir", str(tmp_path / "packed")]))
    assert len(hists) == 2 and all(h[-1]["iteration"] == 40 and h[-1]["env_steps"] == 40 * ENVS for h in hists)
    dirs = sorted(os.listdir(tmp_path / "packed"))
    assert len(made) == 1 and made[0].S == 2 and made[0].graph is not None           # one captured graph
    kinds = [op[0] for op in made[0].tapes[0]]
    assert "unsupported" not in kinds and kinds.count("sqrl_f16x3") == 1 and kinds.count("sqrl") == 0
    at = kinds.index("sqrl_f16x3")
    assert kinds[at - 1] == "call" and made[0].tapes[0][at - 1][1].__name__ == "rrl_w2_pack_f16x3"
    assert [st[0] for st in made[0].stages if st[2][0][0] == "sqrl_f16x3"] == [made[0].lib.rrl_sqrl_act_f16x3_packed]
    for d in dirs:
        rs = pickle.load(open(os.path.join(tmp_path / "packed", d, "run_stats.pkl"), "rb"))
        assert rs["vector_rules"]["sqrl_acting"] == "hip" and rs["vector_rules"]["sqrl_scoring"] == "f16x3"
        assert rs["seeds_per_gpu"] == 2
    assert hists[0][-1]["sac_updates"] > 30 and hists[0][-1] != hists[1][-1]
    log_nu = made[0].loops[1].agent.log_nu.detach().clone()
    tick = made[0].loops[1].sqrl_actor().sqrl_tick.clone()
    solo_cfg = arg_utils.get_args(argv + ["--seed", "5", "--logdir", str(tmp_path / "solo")])
    ref = Experiment(solo_cfg)
    assert ref.agent.fast is not None and ref.loop.sqrl_hip and ref.loop.sqrl_f16x3
    ref.pretrain_critic_recovery()
    loop = ref.loop
    loop.start()
    for _ in range(40):
        loop.vector_step(do_update=len(ref.memory) > solo_cfg.batch_size,
                         random_actions=solo_cfg.start_steps > loop.total_numsteps, online_qrisk=ref.online_qrisk_enabled())
    want = loop.read_stats()
    got = {k: v for k, v in hists[1][-1].items() if k != "iteration"}
    assert got == want
    assert torch.equal(log_nu, ref.agent.log_nu.detach())
    assert torch.equal(tick, loop.sqrl_actor().sqrl_tick) and int(tick[0]) > 30
    assert float(log_nu) != float(np.log(5000.0).astype(np.float32))
