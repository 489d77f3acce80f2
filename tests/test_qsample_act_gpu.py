"""Q-sampling recovery acting on the rrl_qsample_act kernels (RRL_FAST_QSAMPLE=1) against the float64 restatement of
tests/test_qsample_act_cpu.py, against the module path (QRiskWrapper.get_value on the same device, weights and candidates) and
against the reference's recorded answer (tests/golden/select_golden.npz).  The kernel's own Philox draws are regenerated bit
for bit through the C oracle, so every comparison runs on the values the kernel really drew."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import arg_utils
from recovery_rl_amd import _lib, checkpoint
from recovery_rl_amd.experiment import Experiment
from recovery_rl_amd.fast_update import FastActor
from test_qsample_act_cpu import BOXES, KS, NS, PHILOX_SEED, QS, TICK, argmin_first, candidates, case, make_agent

pytestmark = pytest.mark.gpu
DEV = "cuda"
DIAG = {"q": ("f", "nk"), "z": ("f", "2nk"), "cand": ("f", "nk2"), "pick": ("i", "n")}
POISON_I = -77


@pytest.fixture(scope="module")
def rigs():
    """Per action box: the agent on the device, its fused path, Q_risk's weights as the launch takes them."""
    out = {}
    for box in BOXES:
        agent = make_agent(DEV, box)
        fast = agent.enable_fast_path(256)
        out[box] = (agent, fast, weights_of(fast))
    return out


def weights_of(fast):
    P = fast.qrisk.p
    return {"W1": P["W1"], "b1": P["b1"], "W2p": fast.qrisk.w2_packed(), "b2": P["b2"], "W3": P["W3"], "b3": P["b3"]}


def buffers(n, k):
    """Output buffers of one launch, poisoned: an element the kernels do not write shows.  `action` holds finite bytes of
    its own (an ungated env's action must keep exactly those)."""
    shape = {"nk": (n, k), "nk2": (n, k, 2), "2nk": (2, n, k), "n": (n,)}
    out = {name: (torch.full(shape[s], float("nan"), device=DEV) if t == "f" else
                  torch.full(shape[s], POISON_I, dtype=torch.int32, device=DEV)) for name, (t, s) in DIAG.items()}
    out["action"] = 1000.0 + torch.arange(2 * n, dtype=torch.float32, device=DEV).reshape(n, 2)
    return out


def launch(W, obs, k, box, mask=None, cand_in=None, seed=PHILOX_SEED, counter=TICK, tick=None, inc=1, out=None):
    """One rrl_qsample_act call.  tick = int64[2] device tensor: the device-side counter, advanced by `inc`."""
    n = obs.shape[0]
    out = buffers(n, k) if out is None else out
    lib = _lib.load()
    lo, hi = (torch.tensor(b, dtype=torch.float32, device=DEV) for b in BOXES[box])
    scratch = torch.full((int(lib.rrl_qsample_scratch_floats(n, k)),), float("nan"), device=DEV)
    p = _lib.ptr
    a = _lib.rrl_qsample_act_t(n=n, k=k, H=256, d_obs=2, d_act=2, obs=p(obs), mask=p(mask), lo=p(lo), hi=p(hi),
                               seed=seed, counter=counter if tick is None else 0, counter_dev=p(tick),
                               counter_inc=0 if tick is None else inc, cand_in=p(cand_in), scratch=p(scratch),
                               **{name: p(t) for name, t in W.items()}, **{name: p(t) for name, t in out.items()})
    _lib.check(lib.rrl_qsample_act(C.byref(a), _lib.current_stream()), "rrl_qsample_act")
    torch.cuda.synchronize()            # (lo, hi and scratch live until the kernels have run)
    return out


def same(a, b):
    """bit for bit, NaN poison included"""
    return all(torch.equal(a[name].view(torch.int32), b[name].view(torch.int32)) for name in a)


def masks(n):
    """NULL, all ones, all zeros, alternating (first -- and at odd n the last -- env gated), the first and the last env only"""
    e = torch.arange(n, device=DEV)
    return {"null": None, "ones": torch.ones(n, dtype=torch.uint8, device=DEV),
            "zeros": torch.zeros(n, dtype=torch.uint8, device=DEV), "alternating": (e % 2 == 0).to(torch.uint8),
            "ends": ((e == 0) | (e == n - 1)).to(torch.uint8)}


def gated_rows(mask, n):
    return np.ones(n, bool) if mask is None else mask.cpu().numpy().astype(bool)


def check_ungated(out, fresh, gated):
    """Nothing of an ungated env was written: diagnostics keep their poison, the action the bytes it held."""
    off = torch.as_tensor(~gated, device=DEV)
    assert torch.equal(out["action"][off], fresh["action"][off])
    assert bool(torch.isnan(out["q"][off]).all()) and bool(torch.isnan(out["cand"][off]).all())
    assert bool(torch.isnan(out["z"][:, off]).all()) and bool((out["pick"][off] == POISON_I).all())


@torch.no_grad()
def module_q(agent, obs, cand):
    n, k = cand.shape[:2]
    return agent.safety_critic.get_value(obs.unsqueeze(1).expand(n, k, 2).reshape(n * k, 2),
                                         cand.reshape(n * k, 2)).reshape(n, k).double().cpu().numpy()


@pytest.mark.parametrize("box", list(BOXES))
@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("k", KS)
def test_draws_scores_and_pick(rigs, n, k, box):
    """Every shape, box and mask: the kernel drew exactly the restatement's candidates, its scores stay inside the project's
    bar (z within 1e-4 of the tensor's scale; |q - q64| <= 1e-5), the pick is the lowest-index argmin of its
    own q with no row left out, the action is the candidate at the pick bit for bit, and that candidate's float64 score --
    and its score on the module path -- is within twice the q bar of the best (the pick's score and the true minimum's may
    each be off by one bar).  Nothing of an ungated env is written."""
    agent, _, W = rigs[box]
    c = case(n, k, box)
    obs, cand32 = torch.tensor(c["obs"], device=DEV), torch.tensor(c["cand"], device=DEV)
    qmod = module_q(agent, obs, cand32)
    fresh = buffers(n, k)
    for name, mask in masks(n).items():
        own = launch(W, obs, k, box, mask=mask)                       # the kernel's own draws at (PHILOX_SEED, TICK)
        inj = launch(W, obs, k, box, mask=mask, cand_in=cand32)       # the oracle's regeneration of them, injected
        assert same(own, inj), name
        gated = gated_rows(mask, n)
        check_ungated(own, fresh, gated)
        if not gated.any():
            continue
        g = np.flatnonzero(gated)
        got = {key: t.cpu().numpy() for key, t in own.items()}
        assert got["cand"][g].tobytes() == c["cand"][g].tobytes(), name                 # bit for bit
        z, z64 = got["z"][:, g].astype(np.float64), c["z"][:, g]
        err, scale = float(np.abs(z - z64).max()), float(np.abs(z64).max())
        qerr = float(np.abs(got["q"][g].astype(np.float64) - c["q"][g]).max())
        print("n=%d k=%d %s %s: z max error %.3e, scale %.3e; q max error %.3e" % (n, k, box, name, err, scale, qerr))
        assert err <= 1e-4 * scale + 1e-9, (name, err, scale)
        assert qerr <= 1e-5, (name, qerr)
        pick = got["pick"][g]
        assert np.array_equal(pick, argmin_first(got["q"][g])), name
        assert got["action"][g].tobytes() == got["cand"][g, pick].tobytes(), name
        for q64 in (c["q"], qmod):
            assert (q64[g, pick] <= q64[g].min(1) + 2e-5).all(), (name, float((q64[g, pick] - q64[g].min(1)).max()))


def test_ties_and_nan(rigs):
    """All candidates identical: pick 0.  The best candidate duplicated into an earlier and a later chunk: the earliest copy.
    One candidate with a NaN action: that index is picked and the action is NaN."""
    _, _, W = rigs["unit"]
    n, k = 3, 1000
    c = case(n, k, "unit")
    obs, rows = torch.tensor(c["obs"], device=DEV), torch.arange(n, device=DEV)
    flat = torch.tensor(c["cand"][:, :1], device=DEV).expand(n, k, 2).contiguous()
    out = launch(W, obs, k, "unit", cand_in=flat)
    assert out["pick"].tolist() == [0] * n and bool((out["q"] == out["q"][:, :1]).all())
    assert torch.equal(out["action"], flat[:, 0])

    base = launch(W, obs, k, "unit", cand_in=torch.tensor(c["cand"], device=DEV))
    best = base["pick"].long()
    dup = torch.tensor(c["cand"], device=DEV)
    for at in (5, 100, 640, 900, 999):                                    # chunks 0, 0, 5, 7, 7 (the last: 104 rows)
        dup[rows, at] = dup[rows, best]
    out = launch(W, obs, k, "unit", cand_in=dup)
    assert torch.equal(out["pick"].long(), best.clamp(max=5))             # the earliest copy, whichever chunk holds the original
    assert torch.equal(out["action"], dup[rows, best]) and torch.equal(out["q"][rows, 5], base["q"][rows, best])
    for at in (0, 127, 128, 900, 999):                                    # one copy: the lower index of the two
        one = torch.tensor(c["cand"], device=DEV)
        one[rows, at] = one[rows, best]
        assert torch.equal(launch(W, obs, k, "unit", cand_in=one)["pick"].long(), best.clamp(max=at)), at

    for at in (0, 130, 700, 999):
        bad = torch.tensor(c["cand"], device=DEV)
        bad[:, at, 1] = float("nan")
        out = launch(W, obs, k, "unit", cand_in=bad)
        assert out["pick"].tolist() == [at] * n
        assert bool(torch.isnan(out["action"][:, 1]).all()) and torch.equal(out["action"][:, 0], bad[:, at, 0])
        assert bool(torch.isnan(out["q"][:, at]).all()) and int(torch.isnan(out["q"]).sum()) == n
    two = torch.tensor(c["cand"], device=DEV)
    two[:, 300, 0] = float("nan")
    two[:, 40, 0] = float("nan")
    assert launch(W, obs, k, "unit", cand_in=two)["pick"].tolist() == [40] * n       # the first NaN


def test_tick_and_graph(rigs):
    """The device tick advances by exactly counter_inc per call whatever the mask holds (an all-zero mask included); two
    consecutive calls draw different candidates, those the oracle regenerates for the two ticks; a captured graph holding
    the call, replayed twice, gives those two results."""
    _, _, W = rigs["asym"]
    n, k, t0, inc = 3, 129, 1234567, 3
    obs = torch.tensor(case(n, k, "asym")["obs"], device=DEV)
    m = masks(n)
    tick = torch.tensor([t0, 0], dtype=torch.int64, device=DEV)
    fresh = buffers(n, k)
    none = launch(W, obs, k, "asym", mask=m["zeros"], tick=tick, inc=inc)
    assert tick.tolist() == [t0 + inc, 0] and same(none, fresh)
    tick.copy_(torch.tensor([t0, 0]))
    first = launch(W, obs, k, "asym", mask=m["alternating"], tick=tick, inc=inc)
    second = launch(W, obs, k, "asym", mask=m["alternating"], tick=tick, inc=inc)
    assert tick.tolist() == [t0 + 2 * inc, 0]
    assert not torch.equal(first["cand"][0], second["cand"][0]) and not torch.equal(first["action"][0], second["action"][0])
    for t, got in ((t0, first), (t0 + inc, second)):
        want = torch.tensor(candidates(n, k, "asym", PHILOX_SEED, t), device=DEV)
        assert torch.equal(got["cand"][0], want[0]) and torch.equal(got["cand"][2], want[2])
        assert same(got, launch(W, obs, k, "asym", mask=m["alternating"], cand_in=want))
    tick.copy_(torch.tensor([t0, 0]))
    out = buffers(n, k)
    lib = _lib.load()
    lo, hi = (torch.tensor(b, dtype=torch.float32, device=DEV) for b in BOXES["asym"])
    scratch = torch.empty(int(lib.rrl_qsample_scratch_floats(n, k)), device=DEV)
    p = _lib.ptr
    a = _lib.rrl_qsample_act_t(n=n, k=k, H=256, d_obs=2, d_act=2, obs=p(obs), mask=p(m["alternating"]), lo=p(lo), hi=p(hi),
                               seed=PHILOX_SEED, counter=0, counter_dev=p(tick), counter_inc=inc, scratch=p(scratch),
                               **{name: p(t) for name, t in W.items()}, **{name: p(t) for name, t in out.items()})
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        _lib.check(lib.rrl_qsample_act(C.byref(a), _lib.current_stream()), "rrl_qsample_act")
    assert tick.tolist() == [t0, 0]                                    # the capture executed nothing
    for want in (first, second):
        g.replay()
        torch.cuda.synchronize()
        assert same(want, out)
    assert tick.tolist() == [t0 + 2 * inc, 0]


def test_reference_known_answer(golden_dir):
    """The reference's own Q-sampling selection (select_golden.npz: its hidden-16 Q_risk, four states, its 1000 candidates
    each, the action it executed).  The network is zero-padded to width 256 -- padding units contribute exact zeros -- and
    W2 packed with rrl_w2_pack; with the candidates injected the kernel's action is the reference's, bit for bit (float64 on
    the CPU: the argmin is the reference's action in all four, 3.9e-4 .. 1.3e-3 ahead of the runner-up)."""
    S = np.load(os.path.join(golden_dir, "select_golden.npz"))
    h, H = 16, 256
    W = {"W1": torch.zeros(2, H, 4), "b1": torch.zeros(2, H), "W2": torch.zeros(2, H, H), "b2": torch.zeros(2, H),
         "W3": torch.zeros(2, 1, H), "b3": torch.zeros(2, 1)}
    for head, (l1, l2, l3) in enumerate((("linear1", "linear2", "linear3"), ("linear4", "linear5", "linear6"))):
        get = lambda name: torch.tensor(S["qs.qrisk." + name])
        W["W1"][head, :h], W["b1"][head, :h] = get(l1 + ".weight"), get(l1 + ".bias")
        W["W2"][head, :h, :h], W["b2"][head, :h] = get(l2 + ".weight"), get(l2 + ".bias")
        W["W3"][head, :, :h], W["b3"][head] = get(l3 + ".weight"), get(l3 + ".bias")
    W = {name: t.to(DEV).contiguous() for name, t in W.items()}
    W2 = W.pop("W2")
    W["W2p"] = torch.empty(2 * H * H, device=DEV)
    _lib.check(_lib.load().rrl_w2_pack(2, H, W2.data_ptr(), W["W2p"].data_ptr(), _lib.current_stream()), "rrl_w2_pack")
    obs = torch.tensor(S["qs.state"], dtype=torch.float32, device=DEV)
    cand = torch.tensor(S["qs.candidates"], device=DEV)
    out = launch(W, obs, 1000, "unit", cand_in=cand)
    assert out["action"].cpu().numpy().tobytes() == S["qs.action"].tobytes()
    hit = (S["qs.candidates"] == S["qs.action"][:, None]).all(2)
    assert out["pick"].tolist() == [int(np.flatnonzero(r)[0]) for r in hit]


def test_fast_actor_act_qsample_is_the_gate_then_the_call(rigs):
    """FastActor.act_qsample: act_gate's buffers, then the call on the gate's mask at the actor's seed and device tick --
    gated envs execute the kernel's pick, the others their task action."""
    agent, fast, W = rigs["unit"]
    n, k = 65, 129
    obs = torch.tensor(case(n, k, "unit")["obs"], device=DEV)
    with torch.no_grad():
        mean = agent.policy.sample(obs)[2]
        eps_safe = float(agent.safety_critic.get_value(obs, mean).median())
    actor = FastActor(fast, n)
    actor.qsample_seed = PHILOX_SEED
    actor.qsample_tick[0] = TICK
    diag = {name: t for name, t in buffers(n, k).items() if name != "action"}
    task, real, rec = actor.act_qsample(obs, eps_safe, k=k, diag=diag)
    torch.cuda.synchronize()
    assert task is actor.task_action and real is actor.real_action and rec is actor.recovery
    assert actor.qsample_tick.tolist() == [TICK + 1, 0] and rec.dtype == torch.uint8
    gate = rec.bool()
    assert 0 < int(gate.sum()) < n
    direct = launch(weights_of(fast), obs, k, "unit", mask=rec)
    assert torch.equal(real[gate], direct["action"][gate]) and torch.equal(real[~gate], task[~gate])
    assert not torch.equal(real[gate], task[gate])
    assert all(torch.equal(diag[name].view(torch.int32), direct[name].view(torch.int32)) for name in diag)
    with torch.no_grad():                   # the gate is Q_risk(obs, task action) > eps_safe (rows within the f32 paths' error aside)
        q = agent.safety_critic.get_value(obs, task).squeeze(1)
    clear = (q - eps_safe).abs() > 1e-5
    assert torch.equal((q > eps_safe)[clear], gate[clear]) and int(clear.sum()) >= n - 2


# ---- loop ------------------------------------------------------------------------------------------------------------------
ENVS, ITERS = 128, 12


def _cfg(tmp):
    return arg_utils.get_args(["--env-name", "navigation1", "--cuda", "--hidden_size", "256", "--logdir", str(tmp), "--seed", "5",
                               "--num_unsafe_transitions", "2000", "--critic_safe_pretraining_steps", "20", "--num_envs",
                               str(ENVS), "--gamma_safe", "0.8", "--eps_safe", "0.3"] + QS)


def _set_eps(exp, eps):
    exp.exp_cfg.eps_safe = exp.loop.cfg.eps_safe = exp.agent.eps_safe = eps


def _start(tmp):
    """An experiment after pretrain_critic_recovery, on its start states, with eps_safe = the median of Q_risk(obs, task
    action) there: the gate is mixed."""
    exp = Experiment(_cfg(tmp))
    exp.pretrain_critic_recovery()
    obs = exp.loop.start()
    with torch.no_grad():
        action = exp.agent.policy.sample(obs)[0]
        eps = float(exp.agent.safety_critic.get_value(obs, action).median())
    _set_eps(exp, eps)
    return exp, eps


def _eager(exp, iters, between=None):
    for _ in range(iters):
        exp.loop.vector_step(do_update=len(exp.memory) > exp.exp_cfg.batch_size, random_actions=False)
        if between is not None:
            between()


def _state(exp):
    """Env state, both rings, parameters and moments of all networks, loop counters and the tick -- the checkpoint's tree
    without the host generators."""
    torch.cuda.synchronize()
    sd = checkpoint.experiment_state(exp)
    del sd["rng"], sd["extra"]
    return sd


def _diff(a, b, path=""):
    """Paths at which two checkpoint trees differ (tests/test_checkpoint_gpu.py, restated)."""
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


@pytest.fixture(scope="module")
def eager_run(tmp_path_factory):
    """ITERS eager iterations under the switch, and what the first of them did.  Shared, not modified."""
    mp = pytest.MonkeyPatch()
    mp.setenv("RRL_FAST_QSAMPLE", "1")
    try:
        exp, eps = _start(tmp_path_factory.mktemp("eager"))
        assert exp.agent.fast is not None and exp.loop.qsample_hip and exp.vector_rules["qsample_acting"] == "hip"
        off = len(exp.recovery_memory)
        _eager(exp, 1)
        first = {"recovery": exp.loop._last_recovery.clone(), "real": exp.loop._last_real_action.clone(),
                 "task": exp.loop._actor.task_action.clone(), "ring": exp.recovery_memory.a[off:off + ENVS].clone()}
        _eager(exp, ITERS - 1)
        yield exp, eps, first, _state(exp)
    finally:
        mp.undo()


def test_loop_gate_is_mixed_and_gated_actions_are_in_the_box_and_in_the_recovery_ring(eager_run):
    exp, _, first, state = eager_run
    rec = first["recovery"].bool()
    assert 0 < int(rec.sum()) < ENVS
    lo, hi = (torch.tensor(b, dtype=torch.float32, device=DEV) for b in (exp.env.action_space.low, exp.env.action_space.high))
    assert bool(((first["real"][rec] >= lo) & (first["real"][rec] <= hi)).all())
    assert torch.equal(first["real"][~rec], first["task"][~rec]) and not torch.equal(first["real"][rec], first["task"][rec])
    assert torch.equal(first["ring"], first["real"])                      # the recovery ring holds the executed actions
    assert exp.vector_rules["qsample_acting"] == "hip"
    assert state["loop"]["qsample_tick"].tolist() == [ITERS, 0]          # one tick per acting pass
    assert state["loop"]["host_updates"] == [ITERS - 3, ITERS - 3]        # trained once the task ring held more than a batch


def test_loop_is_deterministic_and_independent_of_the_global_generator(eager_run, tmp_path, monkeypatch):
    """A second run of the seed is bit-identical in env state, both rings, parameters and moments of all networks -- with
    torch.rand calls on the global generator between its iterations."""
    monkeypatch.setenv("RRL_FAST_QSAMPLE", "1")
    _, eps, _, want = eager_run
    exp, eps2 = _start(tmp_path)
    assert eps2 == eps
    _eager(exp, ITERS, between=lambda: (torch.rand(7, device=DEV), torch.rand(3)))
    d = _diff(want, _state(exp))
    assert not d, "\n".join(d)


def test_loop_capture_and_replay_equal_the_eager_run(eager_run, tmp_path, monkeypatch):
    monkeypatch.setenv("RRL_FAST_QSAMPLE", "1")
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


def test_loop_checkpoint_resumes_bit_for_bit_and_the_other_path_is_refused(eager_run, tmp_path, monkeypatch):
    monkeypatch.setenv("RRL_FAST_QSAMPLE", "1")
    _, eps, _, want = eager_run
    part, _ = _start(tmp_path / "part")
    _eager(part, 6)
    ck = checkpoint.save(part, str(tmp_path / "mid.pt"))
    mid = torch.load(ck, map_location="cpu", weights_only=False)
    assert mid["loop"]["qsample_tick"].tolist() == [6, 0]
    cont = Experiment(_cfg(tmp_path / "cont"))
    assert cont.loop.qsample_hip
    checkpoint.load(cont, ck)
    cont._apply_demo_share()                 # as the driver's --resume does: the Q_risk batch mix is a setting, not checkpoint state
    _set_eps(cont, eps)
    assert cont.loop.qsample_actor().qsample_tick.tolist() == [6, 0]
    _eager(cont, ITERS - 6)
    d = _diff(want, _state(cont))
    assert not d, "\n".join(d)
    # a run with the switch in the other position refuses the checkpoint, naming the switch -- both ways
    monkeypatch.delenv("RRL_FAST_QSAMPLE")
    other = Experiment(_cfg(tmp_path / "other"))
    assert not other.loop.qsample_hip and other.vector_rules["qsample_acting"] == "modules"
    with pytest.raises(ValueError, match="RRL_FAST_QSAMPLE"):
        checkpoint.load(other, ck)
    other.pretrain_critic_recovery()
    other.loop.start()
    _eager(other, 1)
    ck2 = checkpoint.save(other, str(tmp_path / "modules.pt"))
    monkeypatch.setenv("RRL_FAST_QSAMPLE", "1")
    with pytest.raises(ValueError, match="RRL_FAST_QSAMPLE"):
        checkpoint.load(Experiment(_cfg(tmp_path / "back")), ck2)
