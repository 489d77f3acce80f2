"""Q-sampling recovery with the gate in the launch and its packed form (RRL_PACK_QSAMPLE=1): rrl_qsample_act_gated against
rrl_recovery_select followed by rrl_qsample_act, rrl_qsample_act_packed against the stand-alone calls of its seeds, refusals
that leave the device untouched, the packed call in a hipGraph, every packed Q-sampling seed against its solo runs (with the
switch and on the un-switched path), and the driver.  Every comparison is bit for bit (int32 views, NaN poison included)."""
import ctypes as C
import os
import pickle
import types

import numpy as np
import pytest
import torch

import arg_utils
from recovery_rl_amd import _lib
from recovery_rl_amd import packed as packed_module
from recovery_rl_amd.experiment import Experiment, run_packed
from recovery_rl_amd.packed import PackedLoop
from test_qsample_act_cpu import BOXES, PHILOX_SEED, QS, make_agent, observations
from test_qsample_act_gpu import POISON_I, _diff, _set_eps, _state, buffers, masks, weights_of

pytestmark = pytest.mark.gpu
DEV = "cuda"
EINVAL, ERANGE = -1, -3
MAX_SEEDS = 16
EPS = 0.3
F32 = np.float32


@pytest.fixture(scope="module")
def nets():
    """Q_risk's weights as the launch takes them, for 16 seeds: the agent of tests/test_qsample_act_gpu.py and seeded
    perturbations of it, every W2 packed in fragment order."""
    fast = make_agent(DEV, "unit").enable_fast_path(256)
    base = weights_of(fast)
    W2 = fast.qrisk.p["W2"]
    out = [dict(base)]
    for s in range(1, MAX_SEEDS):
        g = torch.Generator(device=DEV).manual_seed(900 + s)
        W = {name: (t + 0.05 * torch.randn(t.shape, device=DEV, generator=g)).contiguous()
             for name, t in base.items() if name != "W2p"}
        w2 = (W2 + 0.05 * torch.randn(W2.shape, device=DEV, generator=g)).contiguous()
        W["W2p"] = torch.empty_like(base["W2p"])
        _lib.check(_lib.load().rrl_w2_pack(2, 256, w2.data_ptr(), W["W2p"].data_ptr(), _lib.current_stream()), "rrl_w2_pack")
        out.append(W)
    torch.cuda.synchronize()
    assert not torch.equal(out[1]["W2p"], out[0]["W2p"])
    return out


BOX = {}


def box():
    if not BOX:
        BOX["lo"], BOX["hi"] = (torch.tensor(b, dtype=torch.float32, device=DEV) for b in BOXES["asym"])
    return BOX["lo"], BOX["hi"]


def outputs(n, k):
    """The poisoned buffers of tests/test_qsample_act_gpu.py plus what a gate in the launch writes: recovery (poison 9) and
    task_out (NaN)."""
    out = buffers(n, k)
    out["recovery"] = torch.full((n,), 9, dtype=torch.uint8, device=DEV)
    out["task_out"] = torch.full((n, 2), float("nan"), device=DEV)
    return out


def same(a, b, names=None):
    def bits(t):
        return t if t.dtype == torch.uint8 else t.view(torch.int32)
    return [name for name in (names or a) if not torch.equal(bits(a[name]), bits(b[name]))]


def descriptor(W, obs, k, out, scratch, mask=None, seed=PHILOX_SEED, tick=None, inc=1, cand_in=None, diag=True):
    p = _lib.ptr
    lo, hi = box()
    names = ("action", "q", "z", "cand", "pick") if diag else ("action",)
    return _lib.rrl_qsample_act_t(n=obs.shape[0], k=k, H=256, d_obs=2, d_act=2, obs=p(obs), mask=p(mask), lo=p(lo), hi=p(hi),
                                  seed=seed, counter=0, counter_dev=p(tick), counter_inc=inc, cand_in=p(cand_in),
                                  scratch=p(scratch), **{name: p(t) for name, t in W.items()},
                                  **{name: p(out[name]) for name in names})


def gate_of(parts, eps, xa, out):
    p = _lib.ptr
    return _lib.rrl_qsample_gate_t(z=p(parts), n_part=parts.shape[0], part_stride=parts.stride(0), eps_safe=float(eps),
                                   task_action=p(xa[:, 2:4]), ld_task=xa.stride(0), task_out=p(out["task_out"]),
                                   recovery_out=p(out["recovery"]))


def scratch_for(n, k):
    return torch.full((int(_lib.load().rrl_qsample_scratch_floats(n, k)),), float("nan"), device=DEV)


def host_sum(parts):
    """The f32 sum of the partials [n_part, 2, n] taken in order, on the host."""
    with np.errstate(all="ignore"):
        z = parts[0].copy()
        for k in range(1, parts.shape[0]):
            z = (z + parts[k]).astype(F32)
    return z


def sigmoid32(z):
    with np.errstate(all="ignore"):
        return (F32(1) / (F32(1) + np.exp(-z.astype(F32)).astype(F32))).astype(F32)


def special_rows(n_part):
    """(z0, z1) pairs as lists of n_part partials each: the threshold's neighbourhood in either head, infinities and NaN in one
    head and in both, partials that cancel."""
    logit = F32(np.log(EPS / (1 - EPS)))
    near = [logit]
    for _ in range(8):
        near = [np.nextafter(near[0], F32(-np.inf))] + near + [np.nextafter(near[-1], F32(np.inf))]
    low, inf, nan = F32(-30.0), F32(np.inf), F32(np.nan)
    rows = [(z, low) for z in near] + [(low, z) for z in near]
    rows += [(inf, low), (-inf, F32(5)), (-inf, -inf), (inf, inf), (nan, F32(5)), (nan, F32(-5)), (F32(5), nan), (F32(-5), nan),
             (nan, nan), (inf, nan), (nan, -inf)]
    out = []
    for i, (z0, z1) in enumerate(rows):          # the value in partial i % n_part, +0 in the others: the sum is the value
        p0, p1 = [F32(0)] * n_part, [F32(0)] * n_part
        p0[i % n_part], p1[(i + 1) % n_part] = z0, z1
        out.append((p0, p1))
    if n_part > 1:                               # partials that cancel: the in-order sum, and no other, gives these
        big = F32(1e8)
        tail = [F32(0)] * (n_part - 2)
        out.append(([big, -big] + tail, [F32(-5)] + [F32(0)] * (n_part - 1)))                 # 0 -> q = 1/2: fires
        if n_part > 2:
            out.append(([big, -big, F32(-5)] + tail[1:], [F32(-5)] + [F32(0)] * (n_part - 1)))     # -5: does not fire
            out.append(([F32(-5), big, -big] + tail[1:], [F32(-5)] + [F32(0)] * (n_part - 1)))     # (-5 + 1e8) - 1e8 = 0: fires
    return out, near


def gate_partials(n, n_part, turn):
    """Partials [n_part, 2, n] of z: env 0 fires, env 1 does not, then the special rows (all of them at n = 130, a window that
    moves with `turn` otherwise), then random splits around the threshold."""
    rng = np.random.default_rng(31 * n + n_part)
    parts = rng.normal(0.0, 0.8, size=(n_part, 2, n)).astype(F32)
    parts[0] += F32(np.log(EPS / (1 - EPS)))
    special, near = special_rows(n_part)
    fixed = [([F32(5)] + [F32(0)] * (n_part - 1),) * 2, ([F32(-5)] + [F32(0)] * (n_part - 1),) * 2]
    if n == 1:
        fixed = []
    room = max(0, min(len(special), n - len(fixed) - (4 if n > 100 else 0)))
    chosen = fixed + [special[(turn * 7 + i) % len(special)] for i in range(room)]
    for e, (p0, p1) in enumerate(chosen):
        parts[:, 0, e], parts[:, 1, e] = p0, p1
    return parts, len(special), room, near


def test_threshold_rows_hold_eps_and_its_two_neighbours():
    _, near = special_rows(1)
    q = set(sigmoid32(np.array(near)).tolist())
    e = F32(EPS)
    assert {float(np.nextafter(e, F32(0))), float(e), float(np.nextafter(e, F32(1)))} <= q


# ---- the gate in the launch against the separate launches -------------------------------------------------------------------
@pytest.mark.parametrize("n", (1, 17, 130))
@pytest.mark.parametrize("k", (1, 129, 1000))
def test_gated_call_equals_recovery_select_then_the_masked_call(nets, n, k):
    lib, W, st = _lib.load(), nets[0], _lib.current_stream()
    obs = torch.tensor(observations(n, k), device=DEV)
    g = torch.Generator(device=DEV).manual_seed(n * 1000 + k)
    xa = torch.randn(n, 4, device=DEV, generator=g)                     # [s | a_task]: the task action at stride 4
    t0, inc = 4321, 2
    for n_part in (1, 2, 3, 4):
        parts_h, n_special, room, _ = gate_partials(n, n_part, turn=n_part + k)
        assert n < 130 or room == n_special                              # every special row is in at n = 130
        parts = torch.tensor(parts_h, device=DEV)
        zsum = torch.tensor(host_sum(parts_h), device=DEV)
        # the parent's sequence: select on the summed tensor (dummy recovery action), then the call on its mask
        want = outputs(n, k)
        tick = torch.tensor([t0, 0], dtype=torch.int64, device=DEV)
        dummy = torch.zeros(n, 2, device=DEV)
        _lib.check(lib.rrl_recovery_select(n, zsum.data_ptr(), EPS, xa[:, 2:4].data_ptr(), 4, dummy.data_ptr(),
                                           want["action"].data_ptr(), want["recovery"].data_ptr(), want["task_out"].data_ptr(),
                                           st), "rrl_recovery_select")
        scratch = scratch_for(n, k)
        a = descriptor(W, obs, k, want, scratch, mask=want["recovery"], tick=tick, inc=inc)
        _lib.check(lib.rrl_qsample_act(C.byref(a), st), "rrl_qsample_act")
        # the gated call
        got = outputs(n, k)
        tick2 = torch.tensor([t0, 0], dtype=torch.int64, device=DEV)
        scratch2 = scratch_for(n, k)
        a2 = descriptor(W, obs, k, got, scratch2, tick=tick2, inc=inc)
        g2 = gate_of(parts, EPS, xa, got)
        _lib.check(lib.rrl_qsample_act_gated(C.byref(a2), C.byref(g2), st), "rrl_qsample_act_gated")
        torch.cuda.synchronize()
        assert not same(got, want), (n_part, same(got, want))
        assert tick.tolist() == tick2.tolist() == [t0 + inc, 0]
        rec = got["recovery"].bool()
        assert n == 1 or 0 < int(rec.sum()) < n, (n_part, int(rec.sum()))
        assert bool((got["recovery"] <= 1).all()) and torch.equal(got["task_out"], xa[:, 2:4])
        # ungated envs: the action is the task action, the diagnostics keep their poison
        assert torch.equal(got["action"][~rec], xa[:, 2:4][~rec])
        assert bool(torch.isnan(got["q"][~rec]).all()) and bool(torch.isnan(got["cand"][~rec]).all())
        assert bool(torch.isnan(got["z"][:, ~rec]).all()) and bool((got["pick"][~rec] == POISON_I).all())
        assert not bool(torch.isnan(got["q"][rec]).any()) and bool((got["pick"][rec] >= 0).all())
        # without task_out nothing else changes
        got3 = outputs(n, k)
        tick2.copy_(torch.tensor([t0, 0]))
        a3, g3 = descriptor(W, obs, k, got3, scratch2, tick=tick2, inc=inc), gate_of(parts, EPS, xa, got3)
        g3.task_out = None
        _lib.check(lib.rrl_qsample_act_gated(C.byref(a3), C.byref(g3), st), "rrl_qsample_act_gated")
        torch.cuda.synchronize()
        assert same(got3, want) == ["task_out"] and bool(torch.isnan(got3["task_out"]).all())


# ---- packed against stand-alone ------------------------------------------------------------------------------------------------
def seed_inputs(nets, s, k):
    """Seed s of a call: its own env count, weights, observations, threshold, Philox seed, starting tick, tick increment, gate
    family (none / all / alternating / ends, rotated over the seeds), number of partials and diagnostics."""
    n = 3 + 5 * s
    family = ("zeros", "ones", "alternating", "ends")[s % 4]
    mask = masks(n)[family]
    eps = 0.2 + 0.02 * s
    n_part = 1 + s % 4
    rng = np.random.default_rng(77 + s)
    # z = +-5 in both heads by the mask, spread over the partials: sigmoid 0.993 / 0.0067 against thresholds in [0.2, 0.5]
    z = np.where(mask.cpu().numpy().astype(bool), 5.0, -5.0).astype(F32)
    parts = rng.normal(0.0, 0.05, size=(n_part, 2, n)).astype(F32)
    parts[s % n_part] += z
    g = torch.Generator(device=DEV).manual_seed(300 + s)
    return types.SimpleNamespace(n=n, k=k, W=nets[s], obs=torch.tensor(observations(n, 11 + s), device=DEV), mask=mask, eps=eps,
                                 parts=torch.tensor(parts, device=DEV), xa=torch.randn(n, 4, device=DEV, generator=g),
                                 seed=PHILOX_SEED + 7919 * s, t0=1000 + 17 * s, inc=1 + s % 3, diag=s % 3 != 2,
                                 scratch=scratch_for(n, k))


def tick_of(x):
    return torch.tensor([x.t0, 0], dtype=torch.int64, device=DEV)


def arrays(xs, ticks, outs, gated):
    S = len(xs)
    args = (_lib.rrl_qsample_act_t * S)(*[descriptor(x.W, x.obs, x.k, o, x.scratch, mask=None if gated else x.mask, seed=x.seed,
                                                     tick=t, inc=x.inc, diag=x.diag) for x, t, o in zip(xs, ticks, outs)])
    gates = (_lib.rrl_qsample_gate_t * S)(*[gate_of(x.parts, x.eps, x.xa, o) for x, o in zip(xs, outs)]) if gated else None
    return args, gates


def solo_call(x, tick, out, gated):
    lib, st = _lib.load(), _lib.current_stream()
    a = descriptor(x.W, x.obs, x.k, out, x.scratch, mask=None if gated else x.mask, seed=x.seed, tick=tick, inc=x.inc, diag=x.diag)
    if gated:
        g = gate_of(x.parts, x.eps, x.xa, out)
        _lib.check(lib.rrl_qsample_act_gated(C.byref(a), C.byref(g), st), "rrl_qsample_act_gated")
    else:
        _lib.check(lib.rrl_qsample_act(C.byref(a), st), "rrl_qsample_act")
    torch.cuda.synchronize()
    return out


# S: the solo path, pinned with p = 4, pinned with padding workgroups, the linear mapping, pinned with p = 1, two seeds taking
# turns on every XCD; None: a different k per seed
@pytest.mark.parametrize("S,k", [(1, 1000), (2, 17), (3, 129), (5, 128), (8, 1000), (16, 1), (4, None)])
def test_packed_equals_stand_alone_bit_for_bit(nets, S, k):
    lib, st = _lib.load(), _lib.current_stream()
    ks = [k] * S if k is not None else [1000, 1, 129, 17]
    xs = [seed_inputs(nets, s, ks[s]) for s in range(S)]
    for gated in (True, False):
        want = []
        for x in xs:                                 # every seed alone, twice
            tick = tick_of(x)
            first, second = solo_call(x, tick, outputs(x.n, x.k), gated), solo_call(x, tick, outputs(x.n, x.k), gated)
            assert tick.tolist() == [x.t0 + 2 * x.inc, 0]
            want.append((first, second))
        ticks = [tick_of(x) for x in xs]             # the pack, twice
        got = [outputs(x.n, x.k) for x in xs], [outputs(x.n, x.k) for x in xs]
        for outs in got:
            args, gates = arrays(xs, ticks, outs, gated)
            assert lib.rrl_qsample_act_packed(S, args, gates, st) == 0
        torch.cuda.synchronize()
        fresh = {x.n: outputs(x.n, x.k) for x in xs}
        for s, x in enumerate(xs):
            assert not same(got[0][s], want[s][0]) and not same(got[1][s], want[s][1]), (gated, s)
            assert ticks[s].tolist() == [x.t0 + 2 * x.inc, 0], (gated, s)     # the seed's own tick, by its own increment
            out, f = got[0][s], fresh[x.n]
            on = x.mask.bool()
            if on.any() and x.k > 1:
                assert not torch.equal(got[0][s]["action"][on], got[1][s]["action"][on])   # the second call drew at the next tick
            if gated:
                assert torch.equal(out["recovery"], x.mask) and torch.equal(out["task_out"], x.xa[:, 2:4])
                assert torch.equal(out["action"][~on], x.xa[:, 2:4][~on])
            else:                                    # ungated rows are untouched, and so is what only a gate writes
                assert torch.equal(out["action"][~on], f["action"][~on])
                assert not same(out, f, ["recovery", "task_out"])
            if x.diag:
                assert bool(torch.isnan(out["q"][~on]).all()) and bool((out["pick"][~on] == POISON_I).all())
                assert not bool(torch.isnan(out["q"][on]).any()) and not bool(torch.isnan(out["cand"][on]).any())
            else:                                    # diagnostics that were not asked for are not written
                assert not same(out, f, ["q", "z", "cand", "pick"])
    lib.rrl_pack_clear()


def test_refusals_leave_the_device_untouched(nets):
    lib, st, S = _lib.load(), _lib.current_stream(), 3
    xs = [seed_inputs(nets, s + 1, 129) for s in range(S)]
    ticks, outs = [tick_of(x) for x in xs], [outputs(x.n, x.k) for x in xs]
    lib.rrl_pack_clear()

    def refused(code, S=S, gated=True, **edit):
        args, gates = arrays(xs, ticks, outs, gated)
        for target, fields in edit.items():
            for name, v in fields.items():
                setattr({"arg": args, "gate": gates}[target][2], name, v)
        assert lib.rrl_qsample_act_packed(S, args, gates, st) == code, edit

    refused(ERANGE, arg=dict(k=1025))                                   # one bad seed
    refused(ERANGE, gated=False, arg=dict(k=1025))
    refused(EINVAL, arg=dict(mask=xs[2].mask.data_ptr()))               # a mask given with a gate
    refused(EINVAL, gate=dict(n_part=5))
    refused(EINVAL, gate=dict(n_part=0))
    refused(EINVAL, gate=dict(z=None))
    refused(EINVAL, gate=dict(task_action=None))
    refused(EINVAL, gate=dict(recovery_out=None))
    refused(EINVAL, gate=dict(ld_task=3))
    refused(EINVAL, gate=dict(ld_task=0))
    refused(EINVAL, arg=dict(k=1025), gate=dict(n_part=5))              # an invalid field wins
    refused(EINVAL, arg=dict(W2p=xs[2].W["W2p"].data_ptr() + 8))
    args, gates = arrays(xs, ticks, outs, True)
    big = (_lib.rrl_qsample_act_t * 17)(*([args[0]] * 17))
    bigg = (_lib.rrl_qsample_gate_t * 17)(*([gates[0]] * 17))
    assert lib.rrl_qsample_act_packed(17, big, bigg, st) == EINVAL
    assert lib.rrl_qsample_act_packed(0, args, gates, st) == EINVAL
    assert lib.rrl_qsample_act_packed(S, None, gates, st) == EINVAL
    # the stand-alone gated entry: the same codes
    bad = gate_of(xs[0].parts, EPS, xs[0].xa, outs[0])
    bad.n_part = 5
    assert lib.rrl_qsample_act_gated(C.byref(args[0]), C.byref(bad), st) == EINVAL
    assert lib.rrl_qsample_act_gated(C.byref(args[0]), None, st) == EINVAL
    with_mask = descriptor(xs[0].W, xs[0].obs, 129, outs[0], xs[0].scratch, mask=xs[0].mask, tick=ticks[0])
    assert lib.rrl_qsample_act_gated(C.byref(with_mask), C.byref(gates[0]), st) == EINVAL
    torch.cuda.synchronize()
    for s, x in enumerate(xs):
        assert ticks[s].tolist() == [x.t0, 0], s
        assert not same(outs[s], outputs(x.n, x.k)), s                  # no output byte changed
        assert bool(torch.isnan(x.scratch).all())
    assert lib.rrl_pack_clear() == 0                                    # nothing was stored either


def test_packed_call_in_a_graph(nets):
    lib, st, S = _lib.load(), _lib.current_stream(), 3
    xs = [seed_inputs(nets, s + 1, 129) for s in range(S)]
    want = []
    for x in xs:                                     # three eager stand-alone calls per seed
        tick = tick_of(x)
        want.append([solo_call(x, tick, outputs(x.n, x.k), True) for _ in range(3)])
    ticks, outs = [tick_of(x) for x in xs], [outputs(x.n, x.k) for x in xs]
    args, gates = arrays(xs, ticks, outs, True)
    lib.rrl_pack_clear()
    g = torch.cuda.CUDAGraph()                       # a block the library has not seen cannot be built inside a capture
    with pytest.raises(_lib.RRLError, match="capturing"):
        with torch.cuda.graph(g):
            _lib.check(lib.rrl_qsample_act_packed(S, args, gates, _lib.current_stream()), "rrl_qsample_act_packed")
    del g
    torch.cuda.synchronize()
    assert lib.rrl_qsample_act_packed(S, args, gates, st) == 0          # one warm call: the plan exists
    torch.cuda.synchronize()
    for s, x in enumerate(xs):
        ticks[s].copy_(tick_of(x))
        for name, t in outs[s].items():
            t.copy_(outputs(x.n, x.k)[name])
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        _lib.check(lib.rrl_qsample_act_packed(S, args, gates, _lib.current_stream()), "rrl_qsample_act_packed")
    assert all(t.tolist() == [x.t0, 0] for t, x in zip(ticks, xs))     # the capture executed nothing
    for turn in range(3):
        g.replay()
        torch.cuda.synchronize()
        for s in range(S):
            assert not same(outs[s], want[s][turn]), (turn, s)
    assert all(t.tolist() == [x.t0 + 3 * x.inc, 0] for t, x in zip(ticks, xs))
    del g
    lib.rrl_pack_clear()


# ---- every packed Q-sampling seed equals its solo runs -------------------------------------------------------------------------
ENVS, EAGER, K = 128, 4, 9


def _start(tmp, seed):
    """tests/test_qsample_act_gpu.py's _start for a given seed: an experiment after pretrain_critic_recovery, on its start
    states, with eps_safe = the median of Q_risk(obs, task action) there."""
    exp = Experiment(arg_utils.get_args(
        ["--env-name", "navigation1", "--cuda", "--hidden_size", "256", "--logdir", str(tmp), "--seed", str(seed),
         "--num_unsafe_transitions", "2000", "--critic_safe_pretraining_steps", "20", "--num_envs", str(ENVS), "--gamma_safe",
         "0.8", "--eps_safe", "0.3"] + QS))
    exp.pretrain_critic_recovery()
    obs = exp.loop.start()
    with torch.no_grad():
        action = exp.agent.policy.sample(obs)[0]
        eps = float(exp.agent.safety_critic.get_value(obs, action).median())
    _set_eps(exp, eps)
    return exp, eps


def _step(exp):
    exp.loop.vector_step(do_update=len(exp.memory) > exp.exp_cfg.batch_size, random_actions=False)


SOLO = {}


def solo_state(tmp_factory, seed, gate_in_launch, iters):
    """The checkpoint tree of seed `seed` after `iters` eager iterations under RRL_FAST_QSAMPLE=1, with the gate in the launch
    (both switches) or on the parent's path.  Computed once per (seed, path), shared, not modified."""
    key = (seed, gate_in_launch, iters)
    if key not in SOLO:
        SOLO[key] = _solo_state(tmp_factory, seed, gate_in_launch, iters)
    return SOLO[key]


def _solo_state(tmp_factory, seed, gate_in_launch, iters):
    mp = pytest.MonkeyPatch()
    mp.setenv("RRL_FAST_QSAMPLE", "1")
    if gate_in_launch:
        mp.setenv("RRL_PACK_QSAMPLE", "1")
    else:
        mp.delenv("RRL_PACK_QSAMPLE", raising=False)
    try:
        exp, eps = _start(tmp_factory.mktemp("solo"), seed)
        assert exp.loop.qsample_hip and ("qsample_gate" in exp.vector_rules) == gate_in_launch
        for _ in range(iters):
            _step(exp)
        return eps, _state(exp)
    finally:
        mp.undo()


@pytest.mark.parametrize("S", (3, 8))
def test_every_packed_qsample_seed_equals_its_solo_runs(monkeypatch, tmp_path_factory, S):
    """EAGER eager iterations (the task ring holds more than a batch after the third), capture (5 real iterations), the single
    graph once, the four-iteration graph once, singles for the rest of K.  The acting pass runs in every iteration, the
    updates from the fourth on: qsample_tick counts the iterations, host_updates three fewer."""
    monkeypatch.setenv("RRL_FAST_QSAMPLE", "1")
    monkeypatch.setenv("RRL_PACK_QSAMPLE", "1")
    exps, epss = zip(*[_start(tmp_path_factory.mktemp("packed"), 1 + s) for s in range(S)])
    loops = [e.loop for e in exps]
    assert all(l.qsample_hip and e.vector_rules["qsample_gate"] == "in_launch" for l, e in zip(loops, exps))
    for s, e in enumerate(exps):
        _step(e)
        rec = e.loop._last_recovery.bool()
        assert 0 < int(rec.sum()) < ENVS, (s, int(rec.sum()))             # the first iteration's gate is mixed
        for _ in range(EAGER - 1):
            _step(e)
        assert len(e.memory) > e.exp_cfg.batch_size
    packed = PackedLoop(loops, online_qrisk=True)
    done = packed.capture()
    kinds = [op[0] for op in packed.tapes[0]]
    assert kinds.count("qsample") == 1 and "unsupported" not in kinds and kinds.count("step") == 1, kinds
    assert [st[0] for st in packed.stages if st[2][0][0] == "qsample"] == [packed.lib.rrl_qsample_act_packed]
    assert packed.launches == len(packed.stages) + sum(len(st[2]) - 1 for st in packed.stages if st[2][0][0] == "call")
    packed.replay()                  # one single iteration,
    packed.advance(4)                # one four-iteration graph,
    for _ in range(K - 5):           # then singles
        packed.replay()
    assert packed.graph_many_iters == 4 and packed.graph_many is not None
    got = [_state(e) for e in exps]
    packed.close()
    iters = EAGER + done + K
    for s in range(S):
        assert got[s]["loop"]["qsample_tick"].tolist() == [iters, 0]
        assert got[s]["loop"]["host_updates"] == [iters - 3, iters - 3]
        for gate_in_launch in (True, False):         # (a) both switches, (b) RRL_FAST_QSAMPLE=1 alone: the parent's path
            eps, want = solo_state(tmp_path_factory, 1 + s, gate_in_launch, iters)
            assert eps == epss[s]
            d = _diff(want, got[s])
            assert not d, "seed %d, gate in launch %s:\n%s" % (1 + s, gate_in_launch, "\n".join(d))
    assert _diff(got[0], got[1])                     # the seeds are different learners


def test_packed_loop_refuses_nine_qsample_loops(monkeypatch, tmp_path):
    monkeypatch.setenv("RRL_FAST_QSAMPLE", "1")
    monkeypatch.setenv("RRL_PACK_QSAMPLE", "1")
    exp, _ = _start(tmp_path, 1)
    assert exp.loop.qsample_hip
    with pytest.raises(ValueError, match="at most 8 seeds"):
        PackedLoop([exp.loop] * 9, online_qrisk=True)
    assert exp.agent.fast.qrisk.w2p is not None            # refused before any net gave up its fragment-order copy


# ---- the driver ----------------------------------------------------------------------------------------------------------------
def test_seeds_per_gpu_runs_the_q_sampling_line_packed(tmp_path, monkeypatch):
    """`--seeds_per_gpu 2` on the Q-sampling line under the two switches: two experiments (own log directories) advanced by one
    shared graph whose acting call is rrl_qsample_act_packed; the second one's counters and tick equal the solo run of that seed
    stepped through the same phases, and so do its env state and Q_risk's parameters.  --start_steps stays at its default: the
    first iteration acts at random and sends the gated envs through QRiskWrapper.select_action -- on candidates from the
    loop's own generator under the switch, so the seeds of one process do not meet in torch's global one."""
    monkeypatch.setenv("RRL_FAST_QSAMPLE", "1")
    monkeypatch.setenv("RRL_PACK_QSAMPLE", "1")
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
    assert len(dirs) == 2 and dirs[0].endswith("_seed4") and dirs[1].endswith("_seed5")
    assert len(made) == 1 and made[0].S == 2 and made[0].graph is not None           # one captured graph
    kinds = [op[0] for op in made[0].tapes[0]]
    assert "unsupported" not in kinds and kinds.count("qsample") == 1
    for d in dirs:
        rs = pickle.load(open(os.path.join(tmp_path / "packed", d, "run_stats.pkl"), "rb"))
        assert rs["vector_rules"]["qsample_acting"] == "hip" and rs["vector_rules"]["qsample_gate"] == "in_launch"
        assert rs["seeds_per_gpu"] == 2
    assert hists[0][-1]["sac_updates"] > 30 and hists[0][-1] != hists[1][-1]
    tick = made[0].loops[1].qsample_actor().qsample_tick.clone()
    pos, flat = made[0].loops[1].env.pos.clone(), made[0].loops[1].agent.fast.qrisk.flat.clone()
    solo_cfg = arg_utils.get_args(argv + ["--seed", "5", "--logdir", str(tmp_path / "solo")])
    ref = Experiment(solo_cfg)
    assert ref.agent.fast is not None and ref.loop.qsample_hip and ref.loop.qsample_gated and solo_cfg.start_steps == 100
    torch.rand(5, device=DEV)                # (the global generator is nobody's input)
    ref.pretrain_critic_recovery()
    loop = ref.loop
    loop.start()
    for _ in range(40):
        loop.vector_step(do_update=len(ref.memory) > solo_cfg.batch_size,
                         random_actions=solo_cfg.start_steps > loop.total_numsteps, online_qrisk=ref.online_qrisk_enabled())
    want = loop.read_stats()
    got = {k: v for k, v in hists[1][-1].items() if k != "iteration"}
    assert got == want
    assert torch.equal(tick, loop.qsample_actor().qsample_tick) and int(tick[0]) == 39       # one random-action iteration
    torch.cuda.synchronize()
    assert torch.equal(pos, ref.env.pos) and torch.equal(flat, ref.agent.fast.qrisk.flat)
