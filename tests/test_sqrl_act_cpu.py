"""SQRL constraint-sampling acting on the rrl_sqrl_act kernel, the parts that need no GPU: the two symbols are declared
and exported, the descriptor is validated before any launch, the switch matrix (which configurations take the kernel), seed
packing keeps refusing SQRL -- and the float64 restatement of the kernel's steps (candidate, score, pick) that
tests/test_sqrl_act_gpu.py measures the kernel against, checked here against SAC._sqrl_action on CPU modules."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest
import torch

import arg_utils
from oracle import c_oracle as co
from recovery_rl_amd import _lib, fast_update
from recovery_rl_amd.experiment import run_packed
from recovery_rl_amd.sac import SAC
from recovery_rl_amd.spaces import Box

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ACT = Box(-np.ones(2), np.ones(2))
OBS = Box(-np.ones(2) * np.inf, np.ones(2) * np.inf)
SQRL = ["--DGD_constraints", "--use_constraint_sampling", "--nu", "5000", "--update_nu"]      # scripts/navigation1.sh
EINVAL, ERANGE = -1, -3
STREAM_SQRL, STREAM_SQRL_PICK = 9, 10

# the shapes of the GPU tests: the smallest at which the kernel's tiling can go wrong (one row, one tile, one tile + 1 row,
# the production 100 = 6.25 tiles in two passes, the full 128; one env, a few, more than one wave of workgroups)
NS, KS = (1, 3, 65), (1, 16, 17, 100, 128)
PHILOX_SEED, TICK = 0x5EED0123456789, 41
MODES = ("none_safe", "all_safe", "mixed")


# ---- ABI ---------------------------------------------------------------------------------------------------------------
def test_symbols_are_declared_exported_and_additive():
    src = open(os.path.join(ROOT, "include", "rrl_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"\bint\s+rrl_sqrl_act\s*\(\s*const\s+rrl_sqrl_act_t\s*\*", code)
    assert re.search(r"\blong long\s+rrl_sqrl_scratch_floats\s*\(", code)
    assert re.search(r"RRL_STREAM_SQRL\s*=\s*9\b", code) and re.search(r"RRL_STREAM_SQRL_PICK\s*=\s*10\b", code)
    for name in ("rrl_sqrl_act", "rrl_sqrl_scratch_floats"):
        assert name in _lib.EXPORTS
    assert "sqrl_kernels.hip" in _lib.HIP_SOURCES
    assert (_lib.STREAM_SQRL, _lib.STREAM_SQRL_PICK) == (STREAM_SQRL, STREAM_SQRL_PICK)
    lib = _lib.load()
    assert lib.rrl_abi_version() == 8                       # nothing existing changed layout
    assert lib.rrl_sqrl_act.argtypes[0] == C.POINTER(_lib.rrl_sqrl_act_t)
    assert "rrl_sqrl_act" in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def _desc(**fields):
    """A well-formed rrl_sqrl_act_t whose device pointers are dummy non-null integers (validation never follows them)."""
    d = 0x1000
    a = _lib.rrl_sqrl_act_t(n=8, k=100, H=256, d_obs=2, d_act=2, obs=d, head=d, n_part=1, part_stride=0, scale=d, bias=d,
                            W1=d, b1=d, W2p=d, b2=d, W3=d, b3=d, eps_safe=0.3, action=d)
    for k, v in fields.items():
        setattr(a, k, v)
    return a


def test_descriptor_validation_without_gpu():
    lib = _lib.load()
    assert lib.rrl_sqrl_act(None, None) == EINVAL
    for name in ("obs", "head", "scale", "bias", "W1", "b1", "W2p", "b2", "W3", "b3", "action"):
        assert lib.rrl_sqrl_act(C.byref(_desc(**{name: None})), None) == EINVAL, name
    for fields in (dict(n=0), dict(n=-4), dict(H=32), dict(H=512), dict(d_obs=3), dict(d_act=1), dict(n_part=0),
                   dict(n_part=5), dict(W2p=0x1004), dict(W2p=0x1008)):
        assert lib.rrl_sqrl_act(C.byref(_desc(**fields)), None) == EINVAL, fields
    for fields in (dict(k=0), dict(k=-1), dict(k=129), dict(n=2 ** 31 - 1, k=3), dict(n=2 ** 25, k=128)):
        assert lib.rrl_sqrl_act(C.byref(_desc(**fields)), None) == ERANGE, fields
    # an invalid field wins over a size out of range, whatever the order of the struct
    assert lib.rrl_sqrl_act(C.byref(_desc(k=500, H=32)), None) == EINVAL


def test_scratch_floats():
    lib = _lib.load()
    for n, k in ((1, 1), (4096, 100), (65, 128), (2 ** 25 - 1, 128)):
        assert lib.rrl_sqrl_scratch_floats(n, k) == 0, (n, k)         # the one-kernel form: everything stays in LDS
    assert lib.rrl_sqrl_scratch_floats(0, 100) == EINVAL and lib.rrl_sqrl_scratch_floats(-1, 100) == EINVAL
    for n, k in ((8, 0), (8, 129), (2 ** 25, 128), (2 ** 32, 1)):
        assert lib.rrl_sqrl_scratch_floats(n, k) == ERANGE, (n, k)


# ---- the switch --------------------------------------------------------------------------------------------------------
def _cfg(*flags):
    return arg_utils.get_args(["--env-name", "navigation1", "--gamma_safe", "0.8", "--eps_safe", "0.3"] + list(flags))


@pytest.mark.parametrize("baselines,sqrl,flags,want", [
    ("1", "1", SQRL, "hip"),
    ("1", "1", ["--use_constraint_sampling"], "hip"),
    ("1", "1", SQRL + ["--hidden_size", "256"], "hip"),
    ("1", None, SQRL, "modules"),                                             # the switch is opt-in
    ("1", "0", SQRL, "modules"),
    (None, "1", SQRL, "modules"),                                             # ... and needs the fused path
    ("0", "1", SQRL, "modules"),
    ("1", "1", SQRL + ["--use_recovery", "--MF_recovery"], "modules"),        # with a recovery policy
    ("1", "1", SQRL + ["--use_recovery"], "modules"),
    ("1", "1", SQRL + ["--hidden_size", "32"], "modules"),                    # other hidden widths
    ("1", "1", SQRL + ["--hidden_size", "512"], "modules"),
    ("1", "1", SQRL + ["--no_fast_path"], "modules"),
    ("1", "1", SQRL + ["--automatic_entropy_tuning", "True"], "modules"),     # no fused path at all
    ("1", "1", ["--DGD_constraints", "--nu", "5000", "--update_nu"], "modules"),   # LR: no constraint sampling
    ("1", "1", [], "modules"),
])
def test_switch_matrix(monkeypatch, baselines, sqrl, flags, want):
    for name, val in (("RRL_FAST_BASELINES", baselines), ("RRL_FAST_SQRL", sqrl)):
        if val is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, val)
    monkeypatch.delenv("RRL_W2_FRAG", raising=False)
    assert fast_update.sqrl_acting_path(_cfg(*flags)) == want
    if want == "hip":
        monkeypatch.setenv("RRL_W2_FRAG", "0")              # without the fragment-order W2 copy there is nothing to read
        assert fast_update.sqrl_acting_path(_cfg(*flags)) == "modules"


@pytest.mark.parametrize("extra", ([], ["--use_recovery", "--MF_recovery"]))
def test_run_packed_still_refuses_sqrl_with_the_switch_on(monkeypatch, tmp_path, extra):
    monkeypatch.setenv("RRL_FAST_BASELINES", "1")
    monkeypatch.setenv("RRL_FAST_SQRL", "1")
    cfg = arg_utils.get_args(["--env-name", "navigation1", "--cuda", "--num_envs", "128", "--seeds_per_gpu", "2",
                              "--gamma_safe", "0.8", "--eps_safe", "0.3", "--logdir", str(tmp_path)] + SQRL + extra)
    with pytest.raises(ValueError, match="use_constraint_sampling"):
        run_packed(cfg)
    assert not os.listdir(tmp_path)


def test_act_sqrl_is_the_policy_forward_and_one_launch_on_the_tape_as_sqrl(monkeypatch):
    """FastActor.act_sqrl with the library's calls recorded (nothing runs): the policy forward through the group entry point,
    then rrl_sqrl_act on Q_risk's flat weights and fragment-order W2, the actor's seed and device tick; kind "sqrl" on the
    launch tape."""
    real, names = _lib.load(), []

    class Recorder:
        def __getattr__(self, name):
            if name in ("rrl_mlp3_is_split", "rrl_abi_version", "rrl_last_hip_error"):
                return getattr(real, name)
            return lambda *args: names.append(name[4:]) or 0

    monkeypatch.setattr(_lib, "_lib", Recorder())
    monkeypatch.setattr(_lib, "current_stream", lambda: 0)
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: False)
    fast = make_agent("cpu").enable_fast_path(256)
    n = 128
    actor = fast_update.FastActor(fast, n)
    with pytest.raises(_lib.RRLError, match="fragment-order"):
        actor.act_sqrl(torch.zeros(n, 2), 0.3)            # (a CPU FlatNet keeps no fragment-order copy)
    fast.qrisk.w2p = torch.empty(2 * 256 * 256)
    actor.sqrl_seed = 77
    del names[:]
    tape = []
    fast_update.set_tape(tape)
    try:
        out = actor.act_sqrl(torch.zeros(n, 2), 0.3)
    finally:
        fast_update.set_tape(None)
    assert out is actor.task_action
    assert names == ["w2_pack", "mlp3_forward_multi", "sqrl_act"] and [op[0] for op in tape] == ["forward", "sqrl"]
    a = tape[1][1]
    assert isinstance(a, _lib.rrl_sqrl_act_t) and (a.n, a.k, a.H, a.d_obs, a.d_act) == (n, 100, 256, 2, 2)
    head, n_part, ps = actor.pol.parts
    assert (a.head, a.n_part, a.part_stride) == (head.data_ptr(), n_part, ps) and n_part == actor.pol.nsplit > 1
    assert a.W2p == fast.qrisk.w2p.data_ptr() and a.W1 == fast.qrisk.p["W1"].data_ptr()
    assert (a.seed, a.counter, a.counter_inc, a.counter_dev) == (77, 0, 1, actor.sqrl_tick.data_ptr())
    assert a.action == actor.task_action.data_ptr() and abs(a.eps_safe - 0.3) < 1e-7
    assert not (a.eps_in or a.u_in or a.scratch or a.q or a.logp or a.cand or a.z or a.pick or a.cstar or a.n_safe)


# ---- inputs shared with the GPU tests ----------------------------------------------------------------------------------
def make_agent(device="cpu"):
    """SAC at hidden 256 with seeded weights (the modules are initialised on the CPU generator and then moved: the same
    values on every device).  Biases are re-drawn (the reference's zero biases make every first-layer unit pass through the
    origin) and Q_risk's last layers are scaled so that q spreads over (0, 1) instead of sitting at 1/2."""
    torch.manual_seed(20)
    args = arg_utils.get_args(["--env-name", "navigation1", "--hidden_size", "256", "--gamma_safe", "0.8", "--eps_safe", "0.3"]
                              + SQRL + (["--cuda"] if device != "cpu" else []))
    agent = SAC(OBS, ACT, args, "/tmp")
    g = torch.Generator().manual_seed(21)
    qr, pol = agent.safety_critic.safety_critic, agent.policy
    with torch.no_grad():
        for lin in (qr.linear1, qr.linear2, qr.linear3, qr.linear4, qr.linear5, qr.linear6, pol.linear1, pol.linear2,
                    pol.mean_linear, pol.log_std_linear):
            lin.bias.copy_(0.1 * torch.randn(lin.bias.shape, generator=g))
        for lin in (qr.linear3, qr.linear6):
            lin.weight.mul_(6.0)
        pol.log_std_linear.bias.sub_(0.5)
    return agent


def observations(n, k):
    rng = np.random.default_rng(1000 * n + k)
    return rng.uniform(-6.0, 6.0, size=(n, 2)).astype(np.float32)


def unit_open(bits64):
    """rrl::unit_open: ((bits >> 12) + 1/2) / 2^52"""
    return (float(bits64 >> 12) + 0.5) / 4503599627370496.0


@functools.lru_cache(maxsize=None)
def draws(n, k, seed=PHILOX_SEED, tick=TICK):
    """The kernel's own draws, regenerated through the C oracle: eps [n, k, 2] f32 (the normal pair of row e k + c of
    stream RRL_STREAM_SQRL, rounded to f32) and u [n] f64 (the low 64 bits of row e of RRL_STREAM_SQRL_PICK)."""
    eps = np.stack([co.normal2(seed, r, STREAM_SQRL, tick) for r in range(n * k)]).astype(np.float32).reshape(n, k, 2)
    u = np.empty(n, np.float64)
    for e in range(n):
        w = co.philox4x32((e, STREAM_SQRL_PICK, tick & 0xFFFFFFFF, tick >> 32), (seed & 0xFFFFFFFF, seed >> 32))
        u[e] = unit_open((w[1] << 32) | w[0])
    return eps, u


def weights64(agent):
    """Q_risk's twin heads as float64 numpy: [(W1, b1, W2, b2, W3, b3)] * 2"""
    qr = agent.safety_critic.safety_critic
    f = lambda lin: (lin.weight.detach().cpu().double().numpy(), lin.bias.detach().cpu().double().numpy())
    return [f(qr.linear1) + f(qr.linear2) + f(qr.linear3), f(qr.linear4) + f(qr.linear5) + f(qr.linear6)]


def policy_head(agent, obs):
    """(mean0, mean1, log_std0, log_std1) before the clamp: what the last layer of the task policy puts out, [n, 4] f32."""
    pol = agent.policy
    with torch.no_grad():
        x = pol.trunk(obs)
        return torch.cat([pol.mean_linear(x), pol.log_std_linear(x)], 1).contiguous()


def restate_scores(W, head, obs, eps, scale=1.0, bias=0.0):
    """Steps 3 and 4 of the kernel in float64: candidates and log-probabilities (GaussianPolicy.sample, model.py:324-340),
    the two pre-activations of Q_risk and q = max sigmoid."""
    head, e = head.astype(np.float64), eps.astype(np.float64)
    mean, ls = head[:, None, 0:2], np.clip(head[:, None, 2:4], -20.0, 2.0)
    y = np.tanh(mean + np.exp(ls) * e)
    cand = y * scale + bias
    logp = (-0.5 * e * e - ls - 0.5 * np.log(2 * np.pi) - np.log(scale * (1 - y * y) + 1e-6)).sum(-1)
    x = np.concatenate([np.broadcast_to(obs.astype(np.float64)[:, None, :], cand.shape), cand], -1)
    z = np.stack([np.maximum(np.maximum(x @ W1.T + b1, 0) @ W2.T + b2, 0) @ W3.T[:, 0] + b3[0]
                  for W1, b1, W2, b2, W3, b3 in W])
    with np.errstate(over="ignore"):
        q = (1.0 / (1.0 + np.exp(-z))).max(0)
    return {"cand": cand, "logp": logp, "z": z, "q": q}


def restate_pick(q, logp, u, eps_safe):
    """Step 5 in float64, bug-compatible with sac.py:153-158 as SAC._sqrl_action documents.  -> n_safe, cstar (-1 on the
    argmin branch), pick, and `ambiguous`: the rows whose decisions a rounding error of the f32 paths may flip."""
    n, k = q.shape
    eps_safe = float(np.float32(eps_safe))                    # the kernel and the modules compare against the f32 value
    safe = q <= eps_safe
    n_safe = safe.sum(1)
    cstar, pick = np.full(n, -1, np.int64), np.zeros(n, np.int64)
    amb = (np.abs(q - eps_safe) < 1e-5).any(1)
    for e in range(n):
        if n_safe[e] == 0:
            pick[e] = int(np.argmin(q[e]))
            s = np.sort(q[e])
            amb[e] |= k > 1 and s[1] - s[0] < 1e-6
            continue
        idx = np.flatnonzero(safe[e])
        w = np.exp(logp[e, idx] - logp[e, idx].max())
        run = np.cumsum(w)                                   # ascending c
        T = run[-1]
        over = np.flatnonzero(run > u[e] * T)
        j = int(over[0]) if over.size else idx.size - 1      # position in the safe list = safe candidates <= c*, minus one
        cstar[e], pick[e] = idx[j], j                        # ... applied to the FULL list
        amb[e] |= bool((np.abs(run - u[e] * T) < 1e-6 * T).any())
    return {"n_safe": n_safe, "cstar": cstar, "pick": pick, "ambiguous": amb}


def thresholds(q):
    """eps_safe per mode: 0 (nothing safe: argmin), 1 (all safe), and the median of q (mixed) -- taken half-way between the
    two values around the median position, so that the threshold itself is no candidate's q."""
    s = np.unique(q)
    m = s.size // 2
    mid = 0.5 * (s[m - 1] + s[m]) if s.size > 1 else 0.5 * (s[0] + 1.0)
    return {"none_safe": 0.0, "all_safe": 1.0, "mixed": float(np.float32(mid))}


def case(agent, n, k, device="cpu"):
    """Inputs and float64 restatement of one (n, k) shape: obs, head (the task policy's modules on the n rows), the kernel's
    own draws, the scores, and per mode the threshold and the pick."""
    obs = torch.as_tensor(observations(n, k), device=device)
    head = policy_head(agent, obs)
    eps, u = draws(n, k)
    sc = restate_scores(weights64(agent), head.cpu().numpy(), obs.cpu().numpy(), eps)
    thr = thresholds(sc["q"])
    return {"obs": obs, "head": head, "eps": eps, "u": u, "scores": sc, "thr": thr,
            "pick": {m: restate_pick(sc["q"], sc["logp"], u, thr[m]) for m in MODES}}


def left_out_cap(n):
    """At most 2 % of a test's rows may be ambiguous."""
    return int(0.02 * n)


@pytest.fixture(scope="module")
def agent():
    return make_agent("cpu")


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("k", KS)
def test_restatement_reproduces_sqrl_action_on_cpu_modules(agent, n, k):
    """The restatement's pick, handed to SAC._sqrl_action as `draw`, and its candidate at that pick: the same action, on
    every row that is not ambiguous -- and the ambiguous ones stay under the cap for the seeds the GPU tests use."""
    c = case(agent, n, k)
    for mode in MODES:
        p = c["pick"][mode]
        keep = ~p["ambiguous"]
        assert (~keep).sum() <= left_out_cap(n), (mode, int((~keep).sum()))
        agent.eps_safe = c["thr"][mode]
        # `draw` is the position in the safe list; where nothing is safe the modules take their own argmin
        draw = np.where(p["n_safe"] > 0, p["pick"], 0)
        got = agent._sqrl_action(c["obs"], safe_samples=k, eps=torch.as_tensor(c["eps"]), draw=draw).numpy()
        want = c["scores"]["cand"][np.arange(n), p["pick"]]
        assert np.allclose(got[keep], want[keep], rtol=1e-5, atol=1e-6), (mode, np.abs(got - want).max())
        if mode == "none_safe":
            assert (p["n_safe"] == 0).all() and (p["cstar"] == -1).all()
        if mode == "all_safe":
            assert (p["n_safe"] == k).all() and (p["cstar"] == p["pick"]).all()
    # the injected draw is what the modules' own categorical would index: the position among the safe candidates
    p = c["pick"]["mixed"]
    safe = c["scores"]["q"] <= c["thr"]["mixed"]
    rows = np.flatnonzero(p["n_safe"] > 0)
    assert all(safe[e, :p["cstar"][e] + 1].sum() - 1 == p["pick"][e] and safe[e, p["cstar"][e]] for e in rows)


def test_mixed_threshold_covers_the_three_branches(agent):
    """One threshold, the median of q at n = 65, k = 100: rows with no safe candidate, rows with some, rows with all."""
    p = case(agent, 65, 100)["pick"]["mixed"]
    counts = [int((p["n_safe"] == 0).sum()), int(((p["n_safe"] > 0) & (p["n_safe"] < 100)).sum()),
              int((p["n_safe"] == 100).sum())]
    assert min(counts) >= 8, counts
    q = case(agent, 65, 100)["scores"]["q"]
    assert q.min() < 0.2 and q.max() > 0.8                    # q spreads over (0, 1)
