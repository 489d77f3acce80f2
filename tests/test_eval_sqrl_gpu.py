"""rrl_eval_rollout_sqrl on the device, over the case table of eval_sqrl_cases.py (which test_eval_sqrl_cpu.py proves fair).

Env, results and tick: the trace-driven checks of test_eval_qsample_gpu.check_case, restated -- a second eager env stepped with
the traced executed actions agrees bit for bit, the results are the fold of the trace, the tick advances by T + reset, dead
rows' entries are untouched, tr_z and tr_eps are never written and flag bit 4 is never set.  Head: tr_task is, bit for bit, a
one-step launch of the EXISTING rrl_eval_rollout[_maze] (its two-output policy stack) at each step's traced states; tr_head
against the float64 stack at the rule of tests/plan_cases.py.  Candidates, scores and pick: the bits of one rrl_sqrl_act launch
per step at the traced obs and head, with the regenerated draws of streams 14 / 15 injected -- a kernel already pinned to
float64 and to SAC._sqrl_action; and q against float64 directly at the bar of test_sqrl_act_gpu.  Then ties and NaN,
determinism and independence, and the packed launch against the solo ones."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import eval_sqrl_cases as SC
import test_eval_maze_gpu as TM
import test_eval_rollout_gpu as TG
from recovery_rl_amd import _lib
from recovery_rl_amd.env.maze import MazeVecEnv
from recovery_rl_amd.env.navigation import ENV_KIND, NavigationVecEnv
from test_eval_rollout_gpu import DEV, GUARD, RESULTS, TRACES, guarded
from test_sqrl_act_cpu import restate_scores

pytestmark = pytest.mark.gpu
EINVAL = -1
SQ_TRACES = {"tr_head": (torch.float32, 4), "tr_pick": (torch.int32, 1), "tr_cstar": (torch.int32, 1),
             "tr_nsafe": (torch.int32, 1), "tr_q": (torch.float32, 1)}
NETS = ("pW1", "pb1", "pW2p", "pb2", "pW3", "pb3", "scale", "bias")
QGROUP = ("qW1", "qb1", "qW2p", "qb2", "qW3", "qb3")


@functools.lru_cache(maxsize=None)
def dev_weights(kind):
    """The kind's weights (eval_sqrl_cases.weights32) on the device by descriptor field, W2 in fragment order (rrl_w2_pack)."""
    lib, out = _lib.load(), {}
    for k, v in SC.weights32(kind).items():
        t = torch.tensor(v, device=DEV).contiguous()
        if k.endswith("W2"):
            packed = torch.empty(t.numel(), dtype=torch.float32, device=DEV)
            _lib.check(lib.rrl_w2_pack(t.shape[0], t.shape[1], t.data_ptr(), packed.data_ptr(), _lib.current_stream()), "w2_pack")
            out[k + "p"] = packed
        else:
            out[k] = t
    return out


class Launch:
    """Buffers and descriptor of one SQRL rollout: every output longer than needed, filled with its guard value."""

    def __init__(self, kind, n, T, k, reset, mode="mixed", horizon=0, eps_safe=None, pos=None, tick=SC.TICK, seed=SC.SEED,
                 weights=None):
        self.case = (kind, n, T, k, reset, mode, horizon)
        self.kind, self.n, self.T, self.k, self.reset, self.horizon = kind, n, T, k, reset, horizon
        self.w = w = dict(dev_weights(kind), **(weights or {}))
        self.buf = {name: guarded(dt, n) for name, dt in RESULTS.items()}
        self.buf.update({name: guarded(dt, T * n * width) for name, (dt, width) in TRACES.items()})
        self.buf.update({name: guarded(dt, T * n * width) for name, (dt, width) in SQ_TRACES.items()})
        self.tick = torch.tensor([tick, 0], dtype=torch.int64, device=DEV)
        if pos is None and not reset:
            pos = SC.start_states(kind, n)
        self.pos = None if pos is None else torch.tensor(np.asarray(pos), dtype=torch.float64, device=DEV).contiguous()
        self.eps_safe = SC.eps_safe(kind, n, T, k, reset, mode, horizon or None) if eps_safe is None else eps_safe
        p = _lib.ptr
        base = _lib.rrl_eval_rollout_t(n=n, T=T, H=256, d_obs=2, d_act=2, env_kind=2 if kind == "maze" else ENV_KIND[kind],
                                       reset=reset, pos=p(self.pos), seed=seed, counter=0, counter_dev=p(self.tick),
                                       eps_safe=self.eps_safe, **{name: p(w[name]) for name in NETS + QGROUP},
                                       **{name: p(t) for name, t in self.buf.items() if name not in SQ_TRACES})
        self.args = _lib.rrl_eval_rollout_sqrl_t(base=base, k=k, horizon=horizon,
                                                 **{name: p(self.buf[name]) for name in SQ_TRACES})

    def run(self):
        _lib.check(_lib.load().rrl_eval_rollout_sqrl(C.byref(self.args), _lib.current_stream()), "rrl_eval_rollout_sqrl")
        return self.read()

    def read(self):
        out = {name: t.cpu().numpy() for name, t in self.buf.items()}
        out["tick"] = self.tick.cpu().tolist()
        return out


def packed_call(launches):
    args = (_lib.rrl_eval_rollout_sqrl_t * len(launches))(*[l.args for l in launches])
    return _lib.load().rrl_eval_rollout_sqrl_packed(len(launches), args, _lib.current_stream())


def same_bits(a, b):
    return all(a[name].tobytes() == b[name].tobytes() for name in a if name != "tick") and a["tick"] == b["tick"]


def views(out, n, T):
    """The used part of every buffer in its shape; asserts the guards behind it."""
    v = TG.views(out, n, T)
    for name, (dt, width) in SQ_TRACES.items():
        assert (out[name][T * n * width:] == GUARD[dt]).all(), name
        v[name] = out[name][:T * n * width].reshape((T, n, width) if width > 1 else (T, n))
    return v


def task_launch(kind, n, horizon, pos, tick):
    """One step of the EXISTING rollout entry, task policy only (its two-output stack), at `pos` and `tick`: tr_task"""
    if kind == "maze":
        one = TM.Launch(n, 1, max(horizon, 1), False, 0, pos=pos, tick=tick)
    else:
        one = TG.Launch(kind, n, 1, False, 0, pos=pos, tick=tick)
    return TG.views(one.run(), n, 1)["tr_task"][0]


def sqrl_act(w, obs, head, k, eps_safe, eps, u):
    """One rrl_sqrl_act launch on the case's Q_risk weights with the draws injected (test_sqrl_act_gpu.launch reads a
    FastUpdater; this one reads the descriptor fields of the rollout): action, cand, q, logp, pick, cstar, n_safe"""
    n = obs.shape[0]
    f32, i32 = dict(dtype=torch.float32, device=DEV), dict(dtype=torch.int32, device=DEV)
    out = {"action": torch.zeros(n, 2, **f32), "cand": torch.zeros(n, k, 2, **f32), "q": torch.zeros(n, k, **f32),
           "logp": torch.zeros(n, k, **f32), "pick": torch.zeros(n, **i32), "cstar": torch.zeros(n, **i32),
           "n_safe": torch.zeros(n, **i32)}
    p = _lib.ptr
    a = _lib.rrl_sqrl_act_t(n=n, k=k, H=256, d_obs=2, d_act=2, obs=p(obs), head=p(head), n_part=1, part_stride=0,
                            scale=p(w["scale"]), bias=p(w["bias"]), W1=p(w["qW1"]), b1=p(w["qb1"]), W2p=p(w["qW2p"]),
                            b2=p(w["qb2"]), W3=p(w["qW3"]), b3=p(w["qb3"]), eps_safe=float(eps_safe), seed=0, counter=0,
                            counter_dev=None, counter_inc=0, eps_in=p(eps), u_in=p(u), **{name: p(t) for name, t in out.items()})
    _lib.check(_lib.load().rrl_sqrl_act(C.byref(a), _lib.current_stream()), "rrl_sqrl_act")
    return {name: t.cpu().numpy() for name, t in out.items()}


def check_case(l, out, float64=False):
    kind, n, T, k, reset, mode, horizon = l.case
    v = views(out, n, T)
    flags = v["tr_flags"]
    # ---- alive from the trace itself; dead rows' entries untouched; tr_z and tr_eps never written; no recovery bit ----
    alive = np.ones((T, n), bool)
    for j in range(1, T):
        alive[j] = alive[j - 1] & ((flags[j - 1] >> 1) & 1 == 0)
    assert ((flags[alive] & 1) == 1).all() and (flags[~alive] == GUARD[torch.uint8]).all()
    assert ((flags[alive] >> 4) == 0).all()
    for name, (dt, width) in list(TRACES.items()) + list(SQ_TRACES.items()):
        a = np.moveaxis(v[name], 1, 2) if name == "tr_z" else v[name]
        if name in ("tr_z", "tr_eps"):
            assert (a == GUARD[dt]).all(), name
            continue
        assert (a[~alive] == GUARD[dt]).all(), name
        if dt != torch.int32:
            assert np.isfinite(a[alive].astype(np.float64)).all() and (a[alive] != GUARD[dt]).all(), name
    assert out["tick"] == [SC.TICK + T + reset, 0]

    # ---- env, exact: a second env at the same seed and tick, stepped with the traced executed actions ----
    if kind == "maze":
        env = MazeVecEnv("maze", n, device=DEV, seed=SC.SEED, horizon=horizon, auto_reset=False)
    else:
        env = NavigationVecEnv(kind, n, device=DEV, seed=SC.SEED, auto_reset=False)
    env.tick[0] = SC.TICK
    if reset:
        env.reset()
    else:
        env.pos.copy_(torch.tensor(SC.start_states(kind, n), device=DEV))
    real = torch.tensor(v["tr_real"], device=DEV)
    pos, rew, fl = [], [], []
    for j in range(T):
        pos.append(env.pos.clone())
        _, r, d, info = env.step(real[j].contiguous())
        rew.append(r.clone())
        fl.append(torch.stack([d, info["constraint"], info["success"]]).clone())
    assert int(env.tick[0].item()) == out["tick"][0]
    pos, rew, fl = torch.stack(pos).cpu().numpy(), torch.stack(rew).cpu().numpy(), torch.stack(fl).cpu().numpy()
    assert v["tr_pos"][alive].tobytes() == pos[alive].tobytes()
    assert v["tr_reward"][alive].tobytes() == rew[alive].tobytes()
    for bit, name in enumerate(("done", "constraint", "success")):
        assert np.array_equal((flags[alive] >> (bit + 1)) & 1, fl[:, bit][alive]), name

    # ---- results: the fold of the trace, f32 adds in step order ----
    ret = np.zeros(n, np.float32)
    for j in range(T):
        ret = np.where(alive[j], ret + v["tr_reward"][j], ret).astype(np.float32)
    assert v["ret"].tobytes() == ret.tobytes()
    assert np.array_equal(v["success"], (alive & ((flags >> 3) & 1 == 1)).any(0))
    assert np.array_equal(v["violation"], (alive & ((flags >> 2) & 1 == 1)).any(0))
    assert np.array_equal(v["steps"], alive.sum(0))
    if kind == "maze":
        assert (v["steps"] <= horizon).all()

    # ---- per step: the head from the existing entry and float64, candidates / scores / pick from rrl_sqrl_act ----
    dev, dev32, top = 0.0, 0.0, 0.0
    for j in range(T):
        ctr = SC.TICK + reset + j
        a = alive[j]
        rows = np.flatnonzero(a)
        if not rows.size:                                    # every row has ended: the step wrote nothing (checked above)
            continue
        at = np.where(a[:, None], v["tr_pos"][j], 0.0)
        obs32 = at.astype(np.float32)
        assert v["tr_task"][j][a].tobytes() == task_launch(kind, n, horizon, at, ctr)[a].tobytes(), j
        # (tr_task is tanh(mean) * scale + bias of head rows 0 .. 1; under SQRL it is not executed)
        h64 = SC.head_chain(kind, obs32[rows])
        dev = max(dev, float(np.abs(v["tr_head"][j][rows] - h64).max()))
        dev32 = max(dev32, float(np.abs(SC.head_chain(kind, obs32[rows], np.float32) - h64).max()))
        top = max(top, float(np.abs(h64).max()))
        head = np.where(a[:, None], v["tr_head"][j], 0.0).astype(np.float32)
        eps, u = SC.noise(n, k, ctr), SC.uniforms(n, ctr)
        got = sqrl_act(l.w, torch.tensor(obs32, device=DEV), torch.tensor(head, device=DEV), k, l.eps_safe,
                       torch.tensor(eps, device=DEV), torch.tensor(u, device=DEV))
        assert v["tr_pick"][j][rows].tobytes() == got["pick"][rows].tobytes(), j
        assert v["tr_cstar"][j][rows].tobytes() == got["cstar"][rows].tobytes(), j
        assert v["tr_nsafe"][j][rows].tobytes() == got["n_safe"][rows].tobytes(), j
        assert v["tr_real"][j][rows].tobytes() == got["action"][rows].tobytes(), j
        assert v["tr_q"][j][rows].tobytes() == got["q"][rows, got["pick"][rows]].tobytes(), j
        assert ((v["tr_pick"][j][rows] >= 0) & (v["tr_pick"][j][rows] < k)).all()
        # ... and the executed action is the regenerated candidate at the pick (rrl_sqrl_act's `cand` from the injected eps)
        assert v["tr_real"][j][rows].tobytes() == got["cand"][rows, v["tr_pick"][j][rows]].tobytes(), j
        if mode == "none_safe":
            assert (v["tr_nsafe"][j][rows] == 0).all() and (v["tr_cstar"][j][rows] == -1).all()
        if mode == "all_safe":
            assert (v["tr_nsafe"][j][rows] == k).all() and (v["tr_cstar"][j][rows] == v["tr_pick"][j][rows]).all()
        if float64:
            w = SC.weights32(kind)
            sc = restate_scores(SC.qrisk64(kind), head[rows], obs32[rows], eps[rows], scale=w["scale"].astype(np.float64),
                                bias=w["bias"].astype(np.float64))
            err = float(np.abs(got["q"][rows] - sc["q"]).max())
            print("step %d: %d live rows, max |q - q64| = %.3g (bar 1e-5)" % (j, len(rows), err))
            assert err <= 1e-5
            assert np.abs(v["tr_q"][j][rows] - sc["q"][np.arange(len(rows)), v["tr_pick"][j][rows]]).max() <= 1e-5
    # tr_head against the float64 stack: 4 x max(the same numpy chain in float32, one float32 ulp of the largest |head64|)
    bound = 4 * max(dev32, 2.0 ** -23 * top)
    print("head: max |tr_head - head64| = %.3g, float32 numpy chain %.3g, largest |head64| %.3g, bound %.3g" % (dev, dev32, top, bound))
    assert dev <= bound
    return v, alive


FLOAT64_SHAPES = {(17, 2, 100), (65, 7, 128)}


@pytest.mark.parametrize("kind,n,T,k,reset,mode", SC.nav_cases())
def test_rollout_navigation(kind, n, T, k, reset, mode):
    l = Launch(kind, n, T, k, reset, mode)
    out = l.run()
    v, alive = check_case(l, out, float64=(n, T, k) in FLOAT64_SHAPES)
    if (n, k, reset, mode, kind) == (65, 100, 0, "mixed", "navigation1"):       # the three branches of the pick, on step 0
        ns = v["tr_nsafe"][0]
        assert min((ns == 0).sum(), ((ns > 0) & (ns < k)).sum(), (ns == k).sum()) >= 8
    assert same_bits(out, Launch(kind, n, T, k, reset, mode).run())              # determinism


@pytest.mark.parametrize("n,T,k,horizon,reset,mode", SC.maze_cases())
def test_rollout_maze(n, T, k, horizon, reset, mode):
    l = Launch("maze", n, T, k, reset, mode, horizon=horizon)
    out = l.run()
    check_case(l, out, float64=(n, T, k) in FLOAT64_SHAPES)
    assert same_bits(out, Launch("maze", n, T, k, reset, mode, horizon=horizon).run())


def test_ties_and_nan():
    """Q_risk's last layers zero and eps_safe = 0: every q equals max sigmoid(b3) > 0, nothing is safe, every candidate ties and
    every row takes pick 0.  A NaN in one qW3 entry: q is NaN (it propagates through the max), nothing is safe (NaN <= eps is
    false), NaN counts as the smallest and the pick is 0."""
    kind, n, T, k = "navigation1", 17, 2, 100
    w = dev_weights(kind)
    bad = w["qW3"].clone()
    bad.view(-1)[5] = float("nan")
    for weights, eps_safe, nan in (({"qW3": torch.zeros_like(w["qW3"])}, 0.0, False), ({"qW3": bad}, 0.5, True)):
        l = Launch(kind, n, T, k, 0, eps_safe=eps_safe, weights=weights)
        v = views(l.run(), n, T)
        live = v["tr_flags"] != GUARD[torch.uint8]
        assert live[0].all()
        assert (v["tr_pick"][live] == 0).all() and (v["tr_nsafe"][live] == 0).all() and (v["tr_cstar"][live] == -1).all()
        assert (v["tr_pick"][~live] == GUARD[torch.int32]).all()
        q = v["tr_q"][live]
        assert np.isnan(q).all() if nan else (np.isfinite(q).all() and (q == q[0]).all() and q[0] > 0)
        # the executed action is candidate 0 of its row: the head on the regenerated eps of (row, step), through rrl_sqrl_act
        for j in range(T):
            a = live[j]
            obs32 = np.where(a[:, None], v["tr_pos"][j], 0.0).astype(np.float32)
            head = np.where(a[:, None], v["tr_head"][j], 0.0).astype(np.float32)
            got = sqrl_act(l.w, torch.tensor(obs32, device=DEV), torch.tensor(head, device=DEV), k, eps_safe,
                           torch.tensor(SC.noise(n, k, SC.TICK + j), device=DEV), torch.tensor(SC.uniforms(n, SC.TICK + j), device=DEV))
            assert v["tr_real"][j][a].tobytes() == got["cand"][a, 0].tobytes()


def test_outputs_do_not_depend_on_the_trace_nor_on_torchs_generators():
    full = Launch("navigation1", 65, 7, 100, 0)
    want = full.run()
    torch.manual_seed(12345)                                    # overwrite the global generators between two launches
    torch.cuda.manual_seed_all(999)
    cpu_state, dev_state = torch.get_rng_state(), torch.cuda.get_rng_state()
    bare = Launch("navigation1", 65, 7, 100, 0)
    for name in TRACES:
        setattr(bare.args.base, name, None)
    for name in SQ_TRACES:
        setattr(bare.args, name, None)
    got = bare.run()
    assert torch.equal(cpu_state, torch.get_rng_state()) and torch.equal(dev_state, torch.cuda.get_rng_state())
    for name in RESULTS:
        assert got[name].tobytes() == want[name].tobytes()
    for name, (dt, _) in list(TRACES.items()) + list(SQ_TRACES.items()):
        assert (got[name] == GUARD[dt]).all()
    assert got["tick"] == want["tick"]
    # ... nor on WHICH traces are asked for: the SQRL traces alone, the base's alone
    for drop in (TRACES, SQ_TRACES):
        part = Launch("navigation1", 65, 7, 100, 0)
        for name in drop:
            setattr(part.args.base if drop is TRACES else part.args, name, None)
        got = part.run()
        for name in list(RESULTS) + [t for t in list(TRACES) + list(SQ_TRACES) if t not in drop]:
            assert got[name].tobytes() == want[name].tobytes(), name
    assert same_bits(want, Launch("navigation1", 65, 7, 100, 0).run())


def test_draws_are_keyed_by_the_env_row_alone():
    """Rows 0 .. 15 of an n = 65 launch and an n = 16 launch with the same row seeds, start states and eps_safe: the same
    results and traces -- candidate c of row i is keyed by i k + c, the pick by i, whatever n is and whichever other rows live."""
    kind, T, k = "navigation2", 7, 65
    big = Launch(kind, 65, T, k, 0)
    small = Launch(kind, 16, T, k, 0, eps_safe=big.eps_safe, pos=SC.start_states(kind, 65)[:16])
    a, b = views(big.run(), 65, T), views(small.run(), 16, T)
    for name in RESULTS:
        assert a[name][:16].tobytes() == b[name].tobytes(), name
    for name in list(TRACES) + list(SQ_TRACES):
        x = a[name][:, :, :16] if name == "tr_z" else a[name][:, :16]
        assert np.ascontiguousarray(x).tobytes() == b[name].tobytes(), name
    assert (b["tr_flags"] != GUARD[torch.uint8]).sum() > 16 and (b["tr_flags"][-1] == GUARD[torch.uint8]).any()


@pytest.mark.parametrize("S", [2, 3])
def test_packed_launch_is_the_solo_launches(S):
    """S seeds that differ in n, T, k, kind within Navigation, reset and weights: each seed's outputs, traces and own tick
    equal its solo launch bit for bit."""
    other = {"qW3": (dev_weights("navigation2")["qW3"] * 0.5).contiguous()}
    cases = [(("navigation1", 65, 7, 100, 0), {}), (("navigation2", 17, 2, 17, 1), dict(weights=other)),
             (("navigation2", 1, 1, 128, 1), {})][:S]
    solo = [Launch(*c, **kw).run() for c, kw in cases]
    launches = [Launch(*c, **kw) for c, kw in cases]
    _lib.check(packed_call(launches), "rrl_eval_rollout_sqrl_packed")
    for (c, _), a, l in zip(cases, solo, launches):
        b = l.read()
        assert same_bits(a, b), c
        assert b["tick"] == [SC.TICK + c[2] + c[4], 0]
    plain = Launch("navigation2", 17, 2, 17, 1, eps_safe=launches[1].eps_safe).run()
    assert not same_bits(plain, solo[1])                                       # the other weights did change that seed


def test_packed_maze_launch_with_different_horizons():
    cases = [(65, 7, 65, 3, 0), (17, 2, 17, 100, 1)]
    mk = lambda n, T, k, h, reset: Launch("maze", n, T, k, reset, horizon=h)
    solo = [mk(*c).run() for c in cases]
    launches = [mk(*c) for c in cases]
    _lib.check(packed_call(launches), "rrl_eval_rollout_sqrl_packed")
    for c, a, l in zip(cases, solo, launches):
        assert same_bits(a, l.read()), c


def test_packed_mix_of_navigation_and_maze_is_refused_and_writes_nothing():
    launches = [Launch("navigation1", 17, 2, 17, 0), Launch("maze", 17, 2, 17, 0, horizon=100)]
    fresh = [l.read() for l in launches]
    assert packed_call(launches) == EINVAL
    torch.cuda.synchronize()
    for a, l in zip(fresh, launches):
        assert same_bits(a, l.read())
