"""SQRL constraint-sampling acting on the rrl_sqrl_act kernel (RRL_FAST_SQRL=1) against its yardstick, the module path
SAC._sqrl_action(state, eps=..., draw=...) on the same device and weights (pinned to the reference by select_golden.npz,
tests/test_models_cpu.py), and against the float64 restatement of tests/test_sqrl_act_cpu.py.  The kernel's own Philox draws
are regenerated bit for bit through the C oracle, so every comparison runs on the values the kernel really drew."""
import ctypes as C
import functools
import os
import pickle

import numpy as np
import pytest
import torch

import arg_utils
from recovery_rl_amd import _lib, checkpoint
from recovery_rl_amd.experiment import Experiment, VectorLoop
from recovery_rl_amd.fast_update import FastActor
from recovery_rl_amd.sac import SAC
from test_sqrl_act_cpu import KS, MODES, NS, PHILOX_SEED, SQRL, TICK, case, draws, left_out_cap, make_agent

pytestmark = pytest.mark.gpu
DEV = "cuda"
DIAG = {"q": ("f", "nk"), "logp": ("f", "nk"), "cand": ("f", "nk2"), "z": ("f", "2nk"), "pick": ("i", "n"),
        "cstar": ("i", "n"), "n_safe": ("i", "n")}


@pytest.fixture(scope="module")
def rig():
    agent = make_agent(DEV)
    fast = agent.enable_fast_path(256)
    cases = functools.lru_cache(maxsize=None)(lambda n, k: case(agent, n, k, device=DEV))   # one restatement per shape, shared
    return agent, fast, cases


def buffers(n, k):
    """Output buffers of one launch, poisoned: an element the kernel does not write shows."""
    shape = {"nk": (n, k), "nk2": (n, k, 2), "2nk": (2, n, k), "n": (n,)}
    out = {name: (torch.full(shape[s], float("nan"), device=DEV) if t == "f" else
                  torch.full(shape[s], -77, dtype=torch.int32, device=DEV)) for name, (t, s) in DIAG.items()}
    out["action"] = torch.full((n, 2), float("nan"), device=DEV)
    return out


def launch(fast, obs, head, k, eps_safe, n_part=1, part_stride=0, eps=None, u=None, seed=PHILOX_SEED, counter=TICK,
           tick=None, out=None):
    """One rrl_sqrl_act launch on Q_risk's live weights.  tick = int64[2] device tensor {tick, ticket}: the device-side
    counter, advanced by one."""
    n = obs.shape[0]
    out = buffers(n, k) if out is None else out
    p, P = _lib.ptr, fast.qrisk.p
    a = _lib.rrl_sqrl_act_t(n=n, k=k, H=256, d_obs=2, d_act=2, obs=p(obs), head=p(head), n_part=n_part,
                            part_stride=part_stride, scale=p(fast.scale), bias=p(fast.bias), W1=p(P["W1"]), b1=p(P["b1"]),
                            W2p=p(fast.qrisk.w2_packed()), b2=p(P["b2"]), W3=p(P["W3"]), b3=p(P["b3"]),
                            eps_safe=float(eps_safe), seed=seed, counter=counter if tick is None else 0,
                            counter_dev=p(tick), counter_inc=0 if tick is None else 1, eps_in=p(eps), u_in=p(u),
                            **{name: p(t) for name, t in out.items()})
    _lib.check(_lib.load().rrl_sqrl_act(C.byref(a), _lib.current_stream()), "rrl_sqrl_act")
    return out


def same(a, b):
    return all(torch.equal(a[name], b[name]) for name in a)


@torch.no_grad()
def module_scores(agent, obs, eps, k):
    """cand, logp and Q_risk's two pre-activations as the module path computes them: the policy and the critic's layers on
    the n k expanded rows (SAC._sqrl_action's first three lines)."""
    n = obs.shape[0]
    sb = obs.unsqueeze(1).expand(n, k, 2).reshape(n * k, 2)
    pi, logp, _ = agent.policy.sample(sb, eps.reshape(n * k, 2))
    qr = agent.safety_critic.safety_critic
    xu = torch.cat([sb, pi], 1)
    relu = torch.nn.functional.relu
    z = torch.stack([qr.linear3(relu(qr.linear2(relu(qr.linear1(xu))))), qr.linear6(relu(qr.linear5(relu(qr.linear4(xu)))))])
    return {"cand": pi.reshape(n, k, 2), "logp": logp.reshape(n, k), "z": z.reshape(2, n, k)}


def errors(got, ref64):
    """max |got - float64| per quantity, and the quantity's scale max |float64|"""
    return {name: (float(np.abs(got[name].double().cpu().numpy() - ref64[name]).max()), float(np.abs(ref64[name]).max()))
            for name in ("cand", "logp", "z")}


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("k", KS)
def test_scores_and_decisions(rig, n, k):
    """Every shape, the three thresholds (nothing safe / all safe / the median of q): the kernel drew exactly the oracle's
    values, its scores stay inside the project's bar (max error <= 1e-4 of the tensor's scale), its
    decisions equal the float64 restatement's on every row that is not ambiguous, the action is the candidate at the pick,
    bit for bit, and the module path with the same draws takes the same action."""
    agent, fast, cases = rig
    c = cases(n, k)
    obs, head = c["obs"], c["head"]
    eps, u = torch.as_tensor(c["eps"], device=DEV), torch.as_tensor(c["u"], device=DEV)
    rows = torch.arange(n, device=DEV)
    for mode in MODES:
        thr, want = c["thr"][mode], c["pick"][mode]
        own = launch(fast, obs, head, k, thr)                       # the kernel's own draws at (PHILOX_SEED, TICK)
        inj = launch(fast, obs, head, k, thr, eps=eps, u=u)         # the oracle's regeneration of them, injected
        assert same(own, inj), mode
        assert not any(bool(torch.isnan(t).any()) for t in own.values() if t.is_floating_point())
        for name, (err, scale) in errors(own, c["scores"]).items():
            print("n=%d k=%d %s: kernel max error %.3e, scale %.3e" % (n, k, name, err, scale))
            assert err <= 1e-4 * scale + 1e-9, (name, err, scale)
        # q itself, sigmoid included: the 1e-5 margin around eps_safe that makes a row ambiguous presumes an error below it
        assert float(np.abs(own["q"].double().cpu().numpy() - c["scores"]["q"]).max()) <= 1e-5
        keep = ~want["ambiguous"]
        assert (~keep).sum() <= left_out_cap(n), (mode, int((~keep).sum()))
        for name in ("n_safe", "cstar", "pick"):
            got = own[name].cpu().numpy()
            assert np.array_equal(got[keep], want[name][keep]), (mode, name, np.flatnonzero(got != want[name]))
        assert torch.equal(own["action"], own["cand"][rows, own["pick"].long()]), mode
        agent.eps_safe = thr
        draw = np.where(want["n_safe"] > 0, want["pick"], 0)
        mod = agent._sqrl_action(obs, safe_samples=k, eps=eps, draw=draw)
        k_t = torch.as_tensor(keep, device=DEV)
        assert torch.allclose(own["action"][k_t], mod[k_t], rtol=1e-5, atol=1e-6), mode
        if mode == "mixed" and (n, k) == (65, 100):
            ns = own["n_safe"].cpu().numpy()
            counts = [int((ns == 0).sum()), int(((ns > 0) & (ns < k)).sum()), int((ns == k).sum())]
            assert min(counts) >= 8, counts                          # argmin rows, mixed rows, all-safe rows


def test_numeric_agreement_with_float64_is_the_module_paths(rig):
    """cand, logp and the two pre-activations against the float64 restatement, the kernel beside the module path on the
    same inputs (observations, weights, draws): the kernel's largest error is at most twice the module path's own (differing
    expf / tanhf / summation order), and inside 1e-4 of the tensor's scale.  The largest error is taken over all the
    shapes of this file together: at n = k = 1 a "largest error" is one rounding, and the ratio of two roundings says
    nothing.  The pair is printed per quantity; DESIGN.md section 5 records it."""
    agent, fast, cases = rig
    worst = {name: [0.0, 0.0, 0.0] for name in ("cand", "logp", "z")}
    for n in NS:
        for k in KS:
            c = cases(n, k)
            eps = torch.as_tensor(c["eps"], device=DEV)
            ker = errors(launch(fast, c["obs"], c["head"], k, 0.5, eps=eps), c["scores"])
            mod = errors(module_scores(agent, c["obs"], eps, k), c["scores"])
            for name in worst:
                worst[name] = [max(worst[name][0], ker[name][0]), max(worst[name][1], mod[name][0]),
                               max(worst[name][2], ker[name][1])]
    for name, (ker, mod, scale) in worst.items():
        print("%s: largest error against float64: kernel %.3e, module path %.3e (scale %.3e)" % (name, ker, mod, scale))
    for name, (ker, mod, scale) in worst.items():
        assert ker <= 2 * mod, (name, ker, mod)
        assert ker <= 1e-4 * scale, (name, ker, scale)


def test_partial_sums_of_the_head_equal_the_summed_head(rig):
    _, fast, cases = rig
    n, k = 65, 100
    c = cases(n, k)
    g = torch.Generator(device=DEV).manual_seed(3)
    parts = torch.randn(4, n, 4, device=DEV, generator=g) * 0.4
    parts[0] += c["head"]
    summed = ((parts[0] + parts[1]) + parts[2]) + parts[3]               # psum's fixed order
    a = launch(fast, c["obs"], parts, k, c["thr"]["mixed"], n_part=4, part_stride=parts.stride(0))
    b = launch(fast, c["obs"], summed.contiguous(), k, c["thr"]["mixed"])
    assert same(a, b)
    two = launch(fast, c["obs"], parts, k, c["thr"]["mixed"], n_part=2, part_stride=parts.stride(0))
    assert same(two, launch(fast, c["obs"], (parts[0] + parts[1]).contiguous(), k, c["thr"]["mixed"]))
    assert not same(a, two)


def test_tick_and_graph(rig):
    """Two eager launches at device ticks t and t + 1 differ and equal the launches with the oracle's draws for those ticks
    injected; a captured graph holding the launch, replayed twice from tick t, gives exactly those two results and leaves the
    tick at t + 2."""
    _, fast, cases = rig
    n, k, t0 = 65, 100, 1234567
    c = cases(n, k)
    thr = c["thr"]["mixed"]
    tick = torch.tensor([t0, 0], dtype=torch.int64, device=DEV)
    first = launch(fast, c["obs"], c["head"], k, thr, tick=tick)
    second = launch(fast, c["obs"], c["head"], k, thr, tick=tick)
    assert tick.tolist() == [t0 + 2, 0]
    assert not torch.equal(first["action"], second["action"]) and not torch.equal(first["cand"], second["cand"])
    for t, got in ((t0, first), (t0 + 1, second)):
        eps, u = draws(n, k, PHILOX_SEED, t)
        assert same(got, launch(fast, c["obs"], c["head"], k, thr, eps=torch.as_tensor(eps, device=DEV),
                                u=torch.as_tensor(u, device=DEV)))
    tick.copy_(torch.tensor([t0, 0]))
    out = buffers(n, k)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        launch(fast, c["obs"], c["head"], k, thr, tick=tick, out=out)
    assert tick.tolist() == [t0, 0]                                    # the capture executed nothing
    for want in (first, second):
        g.replay()
        torch.cuda.synchronize()
        assert same(want, out)
    assert tick.tolist() == [t0 + 2, 0]


def test_fast_actor_act_sqrl_is_the_launch_on_its_own_policy_forward(rig):
    """FastActor.act_sqrl: the task policy's forward through the group entry point (its last-layer partial sums left in
    pol.parts), then the kernel at the actor's seed and device tick."""
    agent, fast, cases = rig
    n, k = 65, 100
    c = cases(n, k)
    actor = FastActor(fast, n)
    actor.sqrl_seed = PHILOX_SEED
    actor.sqrl_tick[0] = TICK
    diag = {name: t for name, t in buffers(n, k).items() if name != "action"}
    action = actor.act_sqrl(c["obs"], c["thr"]["mixed"], k=k, diag=diag)
    assert action is actor.task_action and actor.sqrl_tick.tolist() == [TICK + 1, 0]
    head, n_part, ps = actor.pol.parts
    direct = launch(fast, c["obs"], head, k, c["thr"]["mixed"], n_part=n_part, part_stride=ps)
    assert torch.equal(action, direct["action"]) and all(torch.equal(diag[name], direct[name]) for name in diag)
    summed = head.reshape(n_part, -1)[:, :4 * n].sum(0) if n_part > 1 else head.reshape(-1)[:4 * n]
    assert torch.allclose(summed.reshape(n, 4), c["head"], rtol=1e-4, atol=1e-5)          # the fused forward's head
    assert not torch.equal(actor.act_sqrl(c["obs"], c["thr"]["mixed"], k=k).clone(), direct["action"])   # next tick


# ---- driver ----------------------------------------------------------------------------------------------------------------
ENVS, RANDOM_ITERS = 64, 2              # --start_steps 100 (the default) at 64 envs: iterations 1 and 2 act at random


def _cfg(tmp, iters, extra=()):
    """A run that ends by its step budget -- at the first log point past `iters` iterations, iters + 10 here -- however many
    episodes those iterations finish (--num_eps keeps its default, which no such run reaches)."""
    return arg_utils.get_args(["--env-name", "navigation1", "--cuda", "--hidden_size", "256", "--logdir", str(tmp),
                               "--seed", "5", "--num_unsafe_transitions", "2000", "--critic_safe_pretraining_steps",
                               "20", "--num_envs", str(ENVS), "--log_every", "10", "--num_steps", str(ENVS * iters),
                               "--gamma_safe", "0.8", "--eps_safe", "0.3"] + SQRL + list(extra))


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


@pytest.fixture
def sqrl_calls(monkeypatch):
    """(training action of the loop?, rows) of every SAC._sqrl_action call."""
    calls, training = [], [False]
    orig_sqrl, orig_act = SAC._sqrl_action, VectorLoop.act

    def act(self, obs, random_actions=False, train=True):
        training[0] = bool(train and not random_actions)
        try:
            return orig_act(self, obs, random_actions, train)
        finally:
            training[0] = False

    def counted(self, *a, **k):
        calls.append((training[0], a[0].shape[0]))
        return orig_sqrl(self, *a, **k)
    monkeypatch.setattr(VectorLoop, "act", act)
    monkeypatch.setattr(SAC, "_sqrl_action", counted)
    return calls


def test_driver_acts_on_the_kernel_under_the_switch(tmp_path, monkeypatch, sqrl_calls):
    monkeypatch.setenv("RRL_FAST_BASELINES", "1")
    monkeypatch.setenv("RRL_FAST_SQRL", "1")
    exp = Experiment(_cfg(tmp_path / "on", 150))
    assert exp.agent.fast is not None and exp.loop.sqrl_hip and exp.vector_rules["sqrl_acting"] == "hip"
    iters = exp.run()[-1]["iteration"]
    assert iters >= 150
    rs = pickle.load(open(os.path.join(exp.logdir, "run_stats.pkl"), "rb"))
    assert rs["vector_rules"]["sqrl_acting"] == "hip" and rs["vector_rules"]["update_path"] == "fused"
    assert not [c for c in sqrl_calls if c[0]], sqrl_calls          # no training action through the modules
    assert exp.loop.graph is not None                                # the steady state replays the captured iteration
    # ... in which the acting launch kept drawing: one tick per iteration that did not act at random, eager or replayed
    assert int(exp.loop.sqrl_actor().sqrl_tick[0]) == iters - RANDOM_ITERS
    assert float(exp.agent.log_nu.detach()) != float(np.log(5000.0).astype(np.float32))
    # the switch off: the same command acts through SAC._sqrl_action
    monkeypatch.delenv("RRL_FAST_SQRL")
    del sqrl_calls[:]
    off = Experiment(_cfg(tmp_path / "off", 20))
    assert not off.loop.sqrl_hip and off.vector_rules["sqrl_acting"] == "modules"
    off.run()
    rs = pickle.load(open(os.path.join(off.logdir, "run_stats.pkl"), "rb"))
    assert rs["vector_rules"]["sqrl_acting"] == "modules"
    assert (True, 64) in sqrl_calls


def test_resumed_run_equals_the_uninterrupted_one(tmp_path, monkeypatch):
    monkeypatch.setenv("RRL_FAST_BASELINES", "1")
    monkeypatch.setenv("RRL_FAST_SQRL", "1")
    full = Experiment(_cfg(tmp_path / "full", 40))
    full.run()
    part = Experiment(_cfg(tmp_path / "part", 20))
    part.run()
    ck = os.path.join(part.logdir, "checkpoint.pt")
    mid = torch.load(ck, map_location="cpu", weights_only=False)
    assert mid["extra"]["vector_rules"]["sqrl_acting"] == "hip" and int(mid["loop"]["sqrl_tick"][0]) > 0
    cont = Experiment(_cfg(tmp_path / "cont", 40, ["--resume", ck]))
    cont.run()
    a = torch.load(os.path.join(full.logdir, "checkpoint.pt"), map_location="cpu", weights_only=False)
    b = torch.load(os.path.join(cont.logdir, "checkpoint.pt"), map_location="cpu", weights_only=False)
    assert a["extra"]["iteration"] == b["extra"]["iteration"] >= 40 > mid["extra"]["iteration"] >= 20
    assert all(int(x["loop"]["sqrl_tick"][0]) == x["extra"]["iteration"] - RANDOM_ITERS for x in (a, b, mid))
    d = _diff(a, b)
    assert not d, "\n".join(d)
    # a run with the switch in the other position refuses the checkpoint, naming the switch -- both ways
    monkeypatch.delenv("RRL_FAST_SQRL")
    other = Experiment(_cfg(tmp_path / "other", 20))
    with pytest.raises(ValueError, match="RRL_FAST_SQRL"):
        checkpoint.load(other, ck)
    other.run()
    monkeypatch.setenv("RRL_FAST_SQRL", "1")
    with pytest.raises(ValueError, match="RRL_FAST_SQRL"):
        checkpoint.load(Experiment(_cfg(tmp_path / "back", 20)), os.path.join(other.logdir, "checkpoint.pt"))
