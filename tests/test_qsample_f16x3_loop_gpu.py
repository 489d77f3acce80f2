"""RRL_QSAMPLE_F16X3=1 in the loop (on top of RRL_FAST_QSAMPLE=1): the run record names the scoring, the gate is mixed and the
gated actions reach the recovery ring, two runs are bit-identical, capture + replay equals the eager run, a checkpoint resumes
bit for bit and refuses the other scoring, the first acting pass differs from the f32 pass only where rule Q allows it, every
packed seed equals its solo run -- and without the switch the run is the parent's.  The small loop of
tests/test_qsample_act_gpu.py: 128 envs (the smallest count its _set_eps start mixes the gate at), 12 iterations, hidden 256."""
import os
import pickle

import numpy as np
import pytest
import torch

import arg_utils
import qsample_f16x3_cases as QC
import sqrl_f16x3_cases as SC
from recovery_rl_amd import checkpoint, fast_update
from recovery_rl_amd import packed as packed_module
from recovery_rl_amd.experiment import Experiment, run_packed
from recovery_rl_amd.packed import PackedLoop
from test_qsample_act_cpu import QS, restate, weights64
from test_qsample_act_gpu import ENVS, ITERS, _cfg, _diff, _eager, _set_eps, _start, _state

pytestmark = pytest.mark.gpu
DEV = "cuda"
SWITCHES = ("RRL_FAST_QSAMPLE", "RRL_QSAMPLE_F16X3")


def _first_pass(exp, off):
    return {"recovery": exp.loop._last_recovery.clone(), "real": exp.loop._last_real_action.clone(),
            "task": exp.loop._actor.task_action.clone(), "ring": exp.recovery_memory.a[off:off + ENVS].clone()}


@pytest.fixture(scope="module")
def eager_run(tmp_path_factory):
    """ITERS eager iterations under both switches, and what the first of them did.  Shared, not modified."""
    mp = pytest.MonkeyPatch()
    for name in SWITCHES:
        mp.setenv(name, "1")
    mp.delenv("RRL_PACK_QSAMPLE", raising=False)
    try:
        exp, eps = _start(tmp_path_factory.mktemp("eager"))
        assert exp.agent.fast is not None and exp.loop.qsample_hip and exp.loop.qsample_f16x3
        off = len(exp.recovery_memory)
        _eager(exp, 1)
        first = _first_pass(exp, off)
        _eager(exp, ITERS - 1)
        yield exp, eps, first, _state(exp)
    finally:
        mp.undo()


def test_loop_records_its_scoring_the_gate_is_mixed_and_gated_actions_reach_the_ring(eager_run):
    exp, _, first, state = eager_run
    assert exp.vector_rules["qsample_acting"] == "hip" and exp.vector_rules["qsample_scoring"] == "f16x3"
    actor = exp.loop.qsample_actor()
    assert actor.qsample_f16x3 and actor.qsample_w2h is not None and bool(torch.isfinite(actor.qsample_w2h).all())
    rec = first["recovery"].bool()
    assert 0 < int(rec.sum()) < ENVS
    lo, hi = (torch.tensor(b, dtype=torch.float32, device=DEV) for b in (exp.env.action_space.low, exp.env.action_space.high))
    assert bool(((first["real"][rec] >= lo) & (first["real"][rec] <= hi)).all())
    assert torch.equal(first["real"][~rec], first["task"][~rec]) and not torch.equal(first["real"][rec], first["task"][rec])
    assert torch.equal(first["ring"], first["real"])                      # the recovery ring holds the executed actions
    assert state["loop"]["qsample_tick"].tolist() == [ITERS, 0] and state["loop"]["qsample_scoring"] == "f16x3"
    assert state["loop"]["host_updates"] == [ITERS - 3, ITERS - 3]


def test_loop_is_deterministic_and_independent_of_the_global_generator(eager_run, tmp_path, monkeypatch):
    for name in SWITCHES:
        monkeypatch.setenv(name, "1")
    _, eps, _, want = eager_run
    exp, eps2 = _start(tmp_path)
    assert eps2 == eps and exp.loop.qsample_f16x3
    _eager(exp, ITERS, between=lambda: (torch.rand(7, device=DEV), torch.rand(3)))
    d = _diff(want, _state(exp))
    assert not d, "\n".join(d)


def test_loop_capture_and_replay_equal_the_eager_run(eager_run, tmp_path, monkeypatch):
    for name in SWITCHES:
        monkeypatch.setenv(name, "1")
    _, _, _, want = eager_run
    exp, _ = _start(tmp_path)
    _eager(exp, 4)
    warm = exp.loop.capture(online_qrisk=True)
    assert exp.loop.graph is not None
    for _ in range(ITERS - 4 - warm):
        exp.loop.replay()
    got = _state(exp)
    assert got["loop"]["qsample_tick"].tolist() == [ITERS, 0]
    d = _diff(want, got)
    assert not d, "\n".join(d)


def test_loop_checkpoint_resumes_bit_for_bit_and_the_other_scoring_is_refused(eager_run, tmp_path, monkeypatch):
    for name in SWITCHES:
        monkeypatch.setenv(name, "1")
    _, eps, _, want = eager_run
    part, _ = _start(tmp_path / "part")
    _eager(part, 6)
    ck = checkpoint.save(part, str(tmp_path / "mid.pt"))
    mid = torch.load(ck, map_location="cpu", weights_only=False)
    assert mid["loop"]["qsample_tick"].tolist() == [6, 0] and mid["loop"]["qsample_scoring"] == "f16x3"
    cont = Experiment(_cfg(tmp_path / "cont"))
    assert cont.loop.qsample_hip and cont.loop.qsample_f16x3
    checkpoint.load(cont, ck)
    cont._apply_demo_share()                 # as the driver's --resume does
    _set_eps(cont, eps)
    _eager(cont, ITERS - 6)
    d = _diff(want, _state(cont))
    assert not d, "\n".join(d)
    # the other scoring refuses the checkpoint and names the switch -- both ways
    monkeypatch.delenv("RRL_QSAMPLE_F16X3")
    other = Experiment(_cfg(tmp_path / "other"))
    assert other.loop.qsample_hip and not other.loop.qsample_f16x3 and other.vector_rules["qsample_scoring"] == "f32"
    with pytest.raises(ValueError, match="RRL_QSAMPLE_F16X3"):
        checkpoint.load(other, ck)
    other.pretrain_critic_recovery()
    other.loop.start()
    _eager(other, 1)
    ck2 = checkpoint.save(other, str(tmp_path / "f32.pt"))
    assert torch.load(ck2, map_location="cpu", weights_only=False)["loop"]["qsample_scoring"] == "f32"
    monkeypatch.setenv("RRL_QSAMPLE_F16X3", "1")
    with pytest.raises(ValueError, match="RRL_QSAMPLE_F16X3"):
        checkpoint.load(Experiment(_cfg(tmp_path / "back")), ck2)


def test_first_acting_pass_differs_from_the_f32_pass_only_where_rule_q_allows(tmp_path, monkeypatch):
    """Two experiments from one identical starting state (the seed's start is deterministic), the first acting pass under f32
    and under f16x3 with the launch's diagnostics: the same recovery mask, task actions and candidates; every differing action
    satisfies rule Q against float64."""
    monkeypatch.setenv("RRL_FAST_QSAMPLE", "1")
    out, k = {}, 1000
    for scoring in ("f32", "f16x3"):
        if scoring == "f16x3":
            monkeypatch.setenv("RRL_QSAMPLE_F16X3", "1")
        else:
            monkeypatch.delenv("RRL_QSAMPLE_F16X3", raising=False)
        exp, eps = _start(tmp_path / scoring)
        assert exp.loop.qsample_f16x3 == (scoring == "f16x3")
        actor = exp.loop.qsample_actor()
        diag = {"cand": torch.full((ENVS, k, 2), float("nan"), device=DEV), "pick": torch.full((ENVS,), -1, dtype=torch.int32, device=DEV)}
        task, real, rec = actor.act_qsample(exp.loop.obs, eps, k=k, diag=diag)
        torch.cuda.synchronize()
        out[scoring] = {"obs": exp.loop.obs.clone(), "eps": eps, "task": task.clone(), "real": real.clone(), "rec": rec.clone(),
                        **{n: t.clone() for n, t in diag.items()}}
    a, b = out["f32"], out["f16x3"]
    assert a["eps"] == b["eps"] and torch.equal(a["obs"], b["obs"])
    assert torch.equal(a["rec"], b["rec"]) and torch.equal(a["task"], b["task"]) and 0 < int(a["rec"].sum()) < ENVS
    assert torch.equal(a["cand"].view(torch.int32), b["cand"].view(torch.int32))
    g = np.flatnonzero(a["rec"].cpu().numpy().astype(bool))
    W = weights64(exp.agent.safety_critic.safety_critic)
    obs_h, cand = a["obs"].cpu().numpy()[g], a["cand"].cpu().numpy()[g]
    z64 = restate(W, obs_h, cand)
    B = SC.bound(z64["z"], QC.emulate(W, obs_h, cand, np.float32)["z"])
    pick = b["pick"].cpu().numpy()[g]
    differ = int((a["real"] != b["real"]).any(1).sum())
    print("%d gated envs, %d actions differ from the f32 pass; bound %.3e" % (len(g), differ, B))
    assert QC.rule_q_holds(z64["q"], pick, B)
    assert np.array_equal(b["real"].cpu().numpy()[g], cand[np.arange(len(g)), pick])
    assert torch.equal(a["real"][~a["rec"].bool()], b["real"][~b["rec"].bool()])


def test_without_the_switch_the_run_is_the_parents(tmp_path, monkeypatch):
    """RRL_FAST_QSAMPLE=1 alone: no "qsample_f16x3" entry on the tape, no stream, scoring recorded as f32 -- and the state equals
    a loop whose attribute was forced off (what a build without the switch runs)."""
    monkeypatch.setenv("RRL_FAST_QSAMPLE", "1")
    monkeypatch.delenv("RRL_QSAMPLE_F16X3", raising=False)
    calls = []
    real = fast_update.record
    monkeypatch.setattr(fast_update, "record", lambda kind, *p: (calls.append(kind), real(kind, *p))[1])
    a, eps = _start(tmp_path / "a")
    assert a.loop.qsample_hip and not a.loop.qsample_f16x3 and a.vector_rules["qsample_scoring"] == "f32"
    _eager(a, 5)
    assert a.loop.qsample_actor().qsample_w2h is None and "qsample" in calls and "qsample_f16x3" not in calls
    monkeypatch.setenv("RRL_QSAMPLE_F16X3", "1")
    b, eps_b = _start(tmp_path / "b")
    assert b.loop.qsample_f16x3 and eps_b == eps
    b.loop.qsample_f16x3 = False                           # what a build without the switch runs
    _eager(b, 5)
    sa, sb = _state(a), _state(b)
    assert sa["loop"]["qsample_scoring"] == sb["loop"]["qsample_scoring"] == "f32"
    d = _diff(sa, sb)
    assert not d, "\n".join(d)


def test_seeds_per_gpu_packs_the_f16x3_line_and_every_seed_equals_its_solo_run(tmp_path, monkeypatch):
    """`--seeds_per_gpu 2` under the three switches: one shared graph whose acting stage is rrl_qsample_act_f16x3_packed behind
    the two per-seed pack calls; each seed's counters, tick, env state and Q_risk parameters equal the solo run of that seed
    under the same switches stepped through the same phases, and the records carry the same vector_rules."""
    for name in SWITCHES + ("RRL_PACK_QSAMPLE",):
        monkeypatch.setenv(name, "1")
    made = []

    class Spy(PackedLoop):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            made.append(self)
    monkeypatch.setattr(packed_module, "PackedLoop", Spy)
    argv = ["--env-name", "navigation1", "--cuda", "--hidden_size", "256"] + QS + [
        "--gamma_safe", "0.8", "--eps_safe", "0.3", "--num_unsafe_transitions", "3000", "--critic_safe_pretraining_steps", "30",
        "--num_envs", "128", "--log_every", "20", "--num_eps", "100000", "--num_steps", str(128 * 40 - 1)]
    hists = run_packed(arg_utils.get_args(argv + ["--seed", "4", "--seeds_per_gpu", "2", "--logdir", str(tmp_path / "packed")]))
    assert len(hists) == 2 and all(h[-1]["iteration"] == 40 and h[-1]["env_steps"] == 40 * 128 for h in hists)
    dirs = sorted(os.listdir(tmp_path / "packed"))
    assert len(made) == 1 and made[0].S == 2 and made[0].graph is not None           # one captured graph
    kinds = [op[0] for op in made[0].tapes[0]]
    assert "unsupported" not in kinds and kinds.count("qsample_f16x3") == 1 and kinds.count("qsample") == 0
    at = kinds.index("qsample_f16x3")
    assert kinds[at - 1] == "call" and made[0].tapes[0][at - 1][1].__name__ == "rrl_w2_pack_f16x3"
    assert [st[0] for st in made[0].stages if st[2][0][0] == "qsample_f16x3"] == [made[0].lib.rrl_qsample_act_f16x3_packed]
    records = [pickle.load(open(os.path.join(tmp_path / "packed", d, "run_stats.pkl"), "rb")) for d in dirs]
    for rs in records:
        assert rs["vector_rules"]["qsample_acting"] == "hip" and rs["vector_rules"]["qsample_scoring"] == "f16x3"
        assert rs["vector_rules"]["qsample_gate"] == "in_launch" and rs["seeds_per_gpu"] == 2
    assert hists[0][-1] != hists[1][-1]
    for s, seed in enumerate((4, 5)):
        loop_p = made[0].loops[s]
        tick, pos = loop_p.qsample_actor().qsample_tick.clone(), loop_p.env.pos.clone()
        flats = [getattr(loop_p.agent.fast, net).flat.clone() for net in ("qrisk", "policy")]
        solo_cfg = arg_utils.get_args(argv + ["--seed", str(seed), "--logdir", str(tmp_path / ("solo%d" % seed))])
        ref = Experiment(solo_cfg)
        assert ref.loop.qsample_hip and ref.loop.qsample_gated and ref.loop.qsample_f16x3
        assert ref.vector_rules["qsample_scoring"] == records[s]["vector_rules"]["qsample_scoring"]
        assert ref.vector_rules["qsample_acting"] == records[s]["vector_rules"]["qsample_acting"]
        assert ref.vector_rules["qsample_gate"] == records[s]["vector_rules"]["qsample_gate"]
        ref.pretrain_critic_recovery()
        loop = ref.loop
        loop.start()
        for _ in range(40):
            loop.vector_step(do_update=len(ref.memory) > solo_cfg.batch_size,
                             random_actions=solo_cfg.start_steps > loop.total_numsteps, online_qrisk=ref.online_qrisk_enabled())
        want = loop.read_stats()
        got = {k: v for k, v in hists[s][-1].items() if k != "iteration"}
        assert got == want, seed
        assert torch.equal(tick, loop.qsample_actor().qsample_tick) and int(tick[0]) > 30
        assert torch.equal(pos, loop.env.pos)
        for net, flat in zip(("qrisk", "policy"), flats):
            assert torch.equal(flat, getattr(ref.agent.fast, net).flat), (seed, net)
