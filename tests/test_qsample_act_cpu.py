"""Q-sampling recovery acting on the rrl_qsample_act kernels, the parts that need no GPU: the two symbols are declared and
exported, the descriptor is validated before any launch, the switch matrix (which configurations take the kernels), seed
packing keeps refusing the flag, FastActor.act_qsample issues the gate's launches and then the one call -- and the float64
restatement of the kernel's steps (candidate, score, argmin) that tests/test_qsample_act_gpu.py measures the kernel against,
checked here against QRiskWrapper.select_action(obs, candidates=...) on CPU modules."""
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
OBS = Box(-np.ones(2) * np.inf, np.ones(2) * np.inf)
QS = ["--use_recovery", "--Q_sampling_recovery"]
EINVAL, ERANGE = -1, -3
STREAM_QSAMPLE = 11

# the shapes of the GPU tests: one row, one tile, one tile + 1 row, one workgroup, one workgroup + 1 row, the production
# count (7 full chunks + 104 rows), the maximum; one env, a few, more than one wave of workgroups
NS, KS = (1, 3, 65), (1, 16, 17, 128, 129, 1000, 1024)
BOXES = {"unit": ((-1.0, -1.0), (1.0, 1.0)), "maze": ((-0.1, -0.1), (0.1, 0.1)), "asym": ((-1.0, 0.25), (0.5, 2.0))}
PHILOX_SEED, TICK = 0x5EED0123456789, 41


# ---- ABI ---------------------------------------------------------------------------------------------------------------
def test_symbols_are_declared_exported_and_additive():
    src = open(os.path.join(ROOT, "include", "rrl_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"\bint\s+rrl_qsample_act\s*\(\s*const\s+rrl_qsample_act_t\s*\*", code)
    assert re.search(r"\blong long\s+rrl_qsample_scratch_floats\s*\(", code)
    assert re.search(r"RRL_STREAM_QSAMPLE\s*=\s*11\b", code)
    for name in ("rrl_qsample_act", "rrl_qsample_scratch_floats"):
        assert name in _lib.EXPORTS
    assert "qsample_kernels.hip" in _lib.HIP_SOURCES
    assert _lib.STREAM_QSAMPLE == STREAM_QSAMPLE
    lib = _lib.load()
    assert lib.rrl_abi_version() == 8                       # additive: nothing existing changed layout
    assert lib.rrl_qsample_act.argtypes[0] == C.POINTER(_lib.rrl_qsample_act_t)
    assert lib.rrl_qsample_scratch_floats.restype == C.c_longlong
    assert "rrl_qsample_act" in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def test_struct_layout_follows_the_header():
    """The ctypes fields, in order, are the header's members (names; every pointer is a void*, the rest by C type)."""
    src = open(os.path.join(ROOT, "include", "rrl_hip.h")).read()
    body = re.search(r"typedef struct \{((?:(?!typedef).)*?)\} rrl_qsample_act_t;", src, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    want = []
    for decl in filter(None, (d.strip() for d in body.split(";"))):
        base, rest = re.match(r"(?:const\s+)?(\w+)\s*(.*)", decl, flags=re.S).groups()
        for name in rest.split(","):
            name = name.strip()
            want.append((name.lstrip("* "), C.c_void_p if name.startswith("*") else {"int": C.c_int, "uint64_t": C.c_uint64}[base]))
    assert [(n, t) for n, t in _lib.rrl_qsample_act_t._fields_] == want


def _desc(**fields):
    """A well-formed rrl_qsample_act_t whose device pointers are dummy non-null integers (validation never follows them)."""
    d = 0x1000
    a = _lib.rrl_qsample_act_t(n=8, k=1000, H=256, d_obs=2, d_act=2, obs=d, lo=d, hi=d, W1=d, b1=d, W2p=d, b2=d, W3=d, b3=d,
                               scratch=d, action=d)
    for k, v in fields.items():
        setattr(a, k, v)
    return a


def test_descriptor_validation_without_gpu():
    lib = _lib.load()
    assert lib.rrl_qsample_act(None, None) == EINVAL
    for name in ("obs", "lo", "hi", "W1", "b1", "W2p", "b2", "W3", "b3", "scratch", "action"):
        assert lib.rrl_qsample_act(C.byref(_desc(**{name: None})), None) == EINVAL, name
    for fields in (dict(n=0), dict(n=-4), dict(H=32), dict(H=512), dict(d_obs=3), dict(d_act=1), dict(W2p=0x1004),
                   dict(W2p=0x1008)):
        assert lib.rrl_qsample_act(C.byref(_desc(**fields)), None) == EINVAL, fields
    for fields in (dict(k=0), dict(k=-1), dict(k=1025), dict(n=2 ** 31 - 1, k=3), dict(n=2 ** 22, k=1024)):
        assert lib.rrl_qsample_act(C.byref(_desc(**fields)), None) == ERANGE, fields
    # an invalid field wins over a size out of range, whatever the order of the struct
    assert lib.rrl_qsample_act(C.byref(_desc(k=5000, H=32)), None) == EINVAL
    assert lib.rrl_qsample_act(C.byref(_desc(k=0, scratch=None)), None) == EINVAL


def test_scratch_floats():
    lib = _lib.load()
    # one (q_min, index, candidate) partial of 4 floats per workgroup: n x ceil(k / 128) of them
    for n, k, chunks in ((1, 1, 1), (1, 128, 1), (1, 129, 2), (4096, 1000, 8), (65, 1024, 8), (2 ** 22 - 1, 1024, 8)):
        assert lib.rrl_qsample_scratch_floats(n, k) == 4 * n * chunks, (n, k)
    assert lib.rrl_qsample_scratch_floats(0, 100) == EINVAL and lib.rrl_qsample_scratch_floats(-1, 100) == EINVAL
    for n, k in ((8, 0), (8, 1025), (2 ** 22, 1024), (2 ** 32, 1)):
        assert lib.rrl_qsample_scratch_floats(n, k) == ERANGE, (n, k)


# ---- the switch --------------------------------------------------------------------------------------------------------
def _cfg(*flags):
    return arg_utils.get_args(["--env-name", "navigation1", "--gamma_safe", "0.8", "--eps_safe", "0.3"] + list(flags))


@pytest.mark.parametrize("switch,flags,want", [
    ("1", QS, "hip"),
    ("1", QS + ["--hidden_size", "256"], "hip"),
    (None, QS, "modules"),                                                  # the switch is opt-in
    ("0", QS, "modules"),
    ("1", QS + ["--MF_recovery"], "modules"),                               # model-free wins in the module code
    ("1", ["--Q_sampling_recovery"], "modules"),                            # without --use_recovery nothing recovers
    ("1", ["--use_recovery"], "modules"),                                   # model-based recovery
    ("1", [], "modules"),
    ("1", QS + ["--hidden_size", "32"], "modules"),                         # other hidden widths
    ("1", QS + ["--hidden_size", "512"], "modules"),
    ("1", QS + ["--no_fast_path"], "modules"),
    ("1", QS + ["--automatic_entropy_tuning", "True"], "modules"),          # no fused path at all
    ("1", QS + ["--use_constraint_sampling"], "modules"),
])
def test_switch_matrix(monkeypatch, switch, flags, want):
    if switch is None:
        monkeypatch.delenv("RRL_FAST_QSAMPLE", raising=False)
    else:
        monkeypatch.setenv("RRL_FAST_QSAMPLE", switch)
    monkeypatch.setenv("RRL_FAST_BASELINES", "1")           # (so that --use_constraint_sampling alone would keep the fused path)
    monkeypatch.delenv("RRL_W2_FRAG", raising=False)
    assert fast_update.fast_qsample_enabled() == (switch == "1")
    assert fast_update.qsample_acting_path(_cfg(*flags)) == want
    if want == "hip":
        monkeypatch.delenv("RRL_FAST_BASELINES")            # the Recovery-RL configurations need no other switch
        assert fast_update.qsample_acting_path(_cfg(*flags)) == "hip"
        monkeypatch.setenv("RRL_W2_FRAG", "0")              # without the fragment-order W2 copy there is nothing to read
        assert fast_update.qsample_acting_path(_cfg(*flags)) == "modules"


def test_run_packed_still_refuses_q_sampling_with_the_switch_on(monkeypatch, tmp_path):
    monkeypatch.setenv("RRL_FAST_QSAMPLE", "1")
    cfg = arg_utils.get_args(["--env-name", "navigation1", "--cuda", "--num_envs", "128", "--seeds_per_gpu", "2",
                              "--hidden_size", "256", "--gamma_safe", "0.8", "--eps_safe", "0.3", "--logdir", str(tmp_path)] + QS)
    with pytest.raises(ValueError, match="Q_sampling_recovery"):
        run_packed(cfg)
    assert not os.listdir(tmp_path)


def test_act_qsample_is_the_gate_and_one_call_on_the_tape_as_qsample(monkeypatch):
    """FastActor.act_qsample with the library's calls recorded (nothing runs): the launches of act_gate -- policy forward,
    task head, Q_risk forward, rrl_recovery_select -- and then rrl_qsample_act on Q_risk's flat weights and fragment-order
    W2, the gate's mask, the executed-action buffer, the actor's seed and device tick; kind "qsample" on the launch tape."""
    real, names = _lib.load(), []

    class Recorder:
        def __getattr__(self, name):
            if name in ("rrl_mlp3_is_split", "rrl_abi_version", "rrl_last_hip_error", "rrl_qsample_scratch_floats"):
                return getattr(real, name)
            return lambda *args: names.append(name[4:]) or 0

    monkeypatch.setattr(_lib, "_lib", Recorder())
    monkeypatch.setattr(_lib, "current_stream", lambda: 0)
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: False)
    fast = make_agent("cpu").enable_fast_path(256)
    n = 128
    actor = fast_update.FastActor(fast, n)
    obs = torch.zeros(n, 2)
    with pytest.raises(_lib.RRLError, match="fragment-order"):
        actor.act_qsample(obs, 0.3)                       # (a CPU FlatNet keeps no fragment-order copy)
    fast.qrisk.w2p = torch.empty(2 * 256 * 256)
    del names[:]
    actor.act_gate(obs, 0.3)
    gate = list(names)
    assert gate[-1] == "recovery_select" and len(gate) >= 4
    actor.qsample_seed = 77
    del names[:]
    tape = []
    fast_update.set_tape(tape)
    try:
        out = actor.act_qsample(obs, 0.3)
    finally:
        fast_update.set_tape(None)
    assert out[0] is actor.task_action and out[1] is actor.real_action and out[2] is actor.recovery
    assert names == ["w2_pack"] + gate + ["qsample_act"]
    assert [op[0] for op in tape].count("qsample") == 1 and tape[-1][0] == "qsample"
    a = tape[-1][1]
    assert isinstance(a, _lib.rrl_qsample_act_t) and (a.n, a.k, a.H, a.d_obs, a.d_act) == (n, 1000, 256, 2, 2)
    P = fast.qrisk.p
    assert a.W2p == fast.qrisk.w2p.data_ptr()
    assert [getattr(a, w) for w in ("W1", "b1", "b2", "W3", "b3")] == [P[w].data_ptr() for w in ("W1", "b1", "b2", "W3", "b3")]
    assert (a.seed, a.counter, a.counter_inc, a.counter_dev) == (77, 0, 1, actor.qsample_tick.data_ptr())
    assert actor.qsample_tick.dtype == torch.int64 and actor.qsample_tick.shape == (2,)
    assert a.obs == obs.data_ptr() and a.mask == actor.recovery.data_ptr() and a.action == actor.real_action.data_ptr()
    lo, hi = actor.qsample_box
    assert (a.lo, a.hi) == (lo.data_ptr(), hi.data_ptr()) and lo.tolist() == [-1.0, -1.0] and hi.tolist() == [1.0, 1.0]
    assert a.scratch == actor._qsample_scratch.data_ptr() and actor._qsample_scratch.numel() == 4 * n * 8
    assert not (a.cand_in or a.q or a.z or a.cand or a.pick)


# ---- inputs shared with the GPU tests ----------------------------------------------------------------------------------
def make_agent(device="cpu", box="unit"):
    """SAC with Q-sampling recovery at hidden 256 and seeded weights (initialised on the CPU generator, then moved: the same
    values on every device).  Biases are re-drawn (the reference's zero biases make every first-layer unit pass through the
    origin) and Q_risk's last layers are scaled so that q spreads over (0, 1) instead of sitting at 1/2."""
    torch.manual_seed(20)
    args = arg_utils.get_args(["--env-name", "navigation1", "--hidden_size", "256", "--gamma_safe", "0.8", "--eps_safe", "0.3"]
                              + QS + (["--cuda"] if device != "cpu" else []))
    lo, hi = BOXES[box]
    agent = SAC(OBS, Box(np.array(lo), np.array(hi)), args, "/tmp")
    g = torch.Generator().manual_seed(21)
    qr, pol = agent.safety_critic.safety_critic, agent.policy
    with torch.no_grad():
        for lin in (qr.linear1, qr.linear2, qr.linear3, qr.linear4, qr.linear5, qr.linear6, pol.linear1, pol.linear2,
                    pol.mean_linear, pol.log_std_linear):
            lin.bias.copy_(0.1 * torch.randn(lin.bias.shape, generator=g))
        for lin in (qr.linear3, qr.linear6):
            lin.weight.mul_(6.0)
    return agent


def observations(n, k):
    rng = np.random.default_rng(1000 * n + k)
    return rng.uniform(-6.0, 6.0, size=(n, 2)).astype(np.float32)


def unit_open(bits64):
    """rrl::unit_open: ((bits >> 12) + 1/2) / 2^52"""
    return (float(bits64 >> 12) + 0.5) / 4503599627370496.0


@functools.lru_cache(maxsize=None)
def uniforms(n, k, seed=PHILOX_SEED, tick=TICK):
    """The kernel's own uniforms, regenerated through the C oracle: u [n, k, 2] f64 -- the open-unit doubles of the low and
    the high 64 bits of Philox (seed, row e k + c, RRL_STREAM_QSAMPLE, tick)."""
    u = np.empty((n * k, 2), np.float64)
    for r in range(n * k):
        w = co.philox4x32((r, STREAM_QSAMPLE, tick & 0xFFFFFFFF, tick >> 32), (seed & 0xFFFFFFFF, seed >> 32))
        u[r] = unit_open((w[1] << 32) | w[0]), unit_open((w[3] << 32) | w[2])
    u.setflags(write=False)
    return u.reshape(n, k, 2)


def candidates(n, k, box, seed=PHILOX_SEED, tick=TICK):
    """a_j = float(double(lo_j) + (double(hi_j) - double(lo_j)) u_j): double arithmetic, one rounding, on the f32 box."""
    lo, hi = (np.asarray(b, np.float32).astype(np.float64) for b in BOXES[box])
    return (lo + (hi - lo) * uniforms(n, k, seed, tick)).astype(np.float32)


def weights64(qr):
    """A QNetworkConstraint's twin heads as float64 numpy: [(W1, b1, W2, b2, W3, b3)] * 2"""
    f = lambda lin: (lin.weight.detach().cpu().double().numpy(), lin.bias.detach().cpu().double().numpy())
    return [f(qr.linear1) + f(qr.linear2) + f(qr.linear3), f(qr.linear4) + f(qr.linear5) + f(qr.linear6)]


def argmin_first(q):
    """torch.argmin's rule per row: NaN counts as the smallest, the lowest index wins ties."""
    return np.argmin(np.where(np.isnan(q), -np.inf, q), axis=1)


def restate(W, obs, cand):
    """Score and pick in float64: the two pre-activations of Q_risk on [obs_e | a_ec], q = max sigmoid, argmin."""
    cand = cand.astype(np.float64)
    x = np.concatenate([np.broadcast_to(obs.astype(np.float64)[:, None, :], cand.shape), cand], -1)
    z = np.stack([np.maximum(np.maximum(x @ W1.T + b1, 0) @ W2.T + b2, 0) @ W3.T[:, 0] + b3[0] for W1, b1, W2, b2, W3, b3 in W])
    with np.errstate(over="ignore"):
        q = (1.0 / (1.0 + np.exp(-z))).max(0)
    return {"z": z, "q": q, "pick": argmin_first(q)}


@functools.lru_cache(maxsize=None)
def _agent(box):
    return make_agent("cpu", box)


@functools.lru_cache(maxsize=None)
def case(n, k, box):
    """Inputs and float64 restatement of one (n, k, box): obs, the kernel's own candidates, scores, pick.  Computed once and
    shared; nobody writes to it."""
    obs, cand = observations(n, k), candidates(n, k, box)
    out = {"obs": obs, "cand": cand, **restate(weights64(_agent(box).safety_critic.safety_critic), obs, cand)}
    for v in out.values():
        v.setflags(write=False)
    return out


def test_candidates_fill_the_open_box():
    for box, (lo, hi) in BOXES.items():
        c = candidates(65, 1000, box)
        lo, hi = np.asarray(lo, np.float32), np.asarray(hi, np.float32)
        assert c.dtype == np.float32 and (c >= lo).all() and (c <= hi).all()
        span = (hi - lo).astype(np.float64)
        assert (np.abs(c.mean((0, 1)) - (lo + hi) / 2) < 0.01 * span).all()             # 65 000 draws: sd = 0.0011 span
        assert (c.min((0, 1)) < lo + 0.001 * span).all() and (c.max((0, 1)) > hi - 0.001 * span).all()
    u = uniforms(65, 1000)
    assert len(np.unique(u)) == u.size and 0.0 < u.min() and u.max() < 1.0
    assert not np.array_equal(uniforms(3, 16, PHILOX_SEED, TICK), uniforms(3, 16, PHILOX_SEED, TICK + 1))


def test_argmin_rule_is_torchs():
    for row, want in (([.3, np.nan, .1, .1], 1), ([.3, .1, .1, .2], 1), ([np.nan, np.nan, 0.], 0), ([.5], 0)):
        assert argmin_first(np.array([row]))[0] == want == int(torch.argmin(torch.tensor(row)))


@pytest.mark.parametrize("box", list(BOXES))
@pytest.mark.parametrize("n,k", [(1, 1), (3, 17), (65, 129), (3, 1000)])
def test_restatement_reproduces_select_action_on_cpu_modules(n, k, box):
    """The restatement's candidates handed to QRiskWrapper.select_action: the module path (f32) executes the restatement's
    pick on every env whose two best float64 scores are further apart than twice the f32 path's error bar (1e-5) -- and the
    others take a candidate that is within that bar of the best."""
    c = case(n, k, box)
    qr = _agent(box).safety_critic
    if k == 1000:
        got = qr.select_action(torch.tensor(c["obs"]), candidates=c["cand"].copy()).numpy()
    else:            # select_action is written for the reference's 1000 candidates: its argmin over k, restated on its get_value
        with torch.no_grad():
            q = qr.get_value(torch.tensor(c["obs"]).unsqueeze(1).expand(n, k, 2).reshape(n * k, 2),
                             torch.tensor(c["cand"]).reshape(n * k, 2)).reshape(n, k)
        got = c["cand"][np.arange(n), q.argmin(1).numpy()]
    want = c["cand"][np.arange(n), c["pick"]]
    s = np.sort(c["q"], 1)
    clear = np.ones(n, bool) if k == 1 else s[:, 1] - s[:, 0] > 2e-5
    assert np.array_equal(got[clear], want[clear])
    assert clear.sum() >= n - max(1, n // 10)
    for e in np.flatnonzero(~clear):
        hit = np.flatnonzero((c["cand"][e] == got[e]).all(1))
        assert hit.size and c["q"][e, hit[0]] <= s[e, 0] + 2e-5
