"""rrl_eval_rollout_qs on the device, over the case table of eval_qsample_cases.py (which test_eval_qsample_cpu.py proves fair).

Env, results and tick: the trace-driven checks of test_eval_rollout_gpu.check_case, restated -- a second eager env stepped
with the traced executed actions agrees bit for bit, the results are the fold of the trace, the tick advances by T + reset,
dead rows' entries are untouched.  Task and gate: the bits of a one-step launch of the EXISTING rrl_eval_rollout[_maze] with
the Q_risk group only, at each step's traced states and tick.  Candidates, scores and pick: the bits of rrl_qsample_act at the
traced obs, the traced gate as its mask and the regenerated stream-13 candidates injected -- a kernel already pinned to float64
and to the reference's known answer; and against float64 directly at the bar of test_draws_scores_and_pick.  Then ties and
NaN, determinism and independence, and the packed launch against the solo ones."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import eval_cases as EC
import eval_maze_cases as MC
import eval_qsample_cases as QC
import test_eval_maze_gpu as TM
import test_eval_rollout_gpu as TG
from recovery_rl_amd import _lib
from recovery_rl_amd.env.maze import MazeVecEnv
from recovery_rl_amd.env.navigation import ENV_KIND, NavigationVecEnv
from test_eval_rollout_gpu import DEV, GUARD, RESULTS, TRACES, guarded
from test_qsample_act_cpu import BOXES, restate
from test_qsample_act_gpu import launch as qsample_act

pytestmark = pytest.mark.gpu
EINVAL = -1
QS_TRACES = {"tr_pick": torch.int32, "tr_q": torch.float32}
NETS = ("pW1", "pb1", "pW2p", "pb2", "pW3", "pb3", "scale", "bias")
QGROUP = ("qW1", "qb1", "qW2p", "qb2", "qW3", "qb3")
RGROUP = ("rW1", "rb1", "rW2p", "rb2", "rW3", "rb3", "rscale", "rbias", "rlog_std")


def dev_weights(kind):
    return TM.dev_weights() if kind == "maze" else TG.dev_weights(kind)


@functools.lru_cache(maxsize=None)
def box_dev(box):
    return tuple(torch.tensor(b, dtype=torch.float32, device=DEV) for b in BOXES[box])


def start_states(kind, n):
    return MC.start_states(n) if kind == "maze" else EC.start_states(kind, n)


class Launch:
    """Buffers and descriptor of one Q-sampling rollout: every output longer than needed, filled with its guard value."""

    def __init__(self, kind, n, T, k, reset, box, horizon=0, eps_safe=None, pos=None, tick=QC.TICK, seed=QC.SEED, weights=None):
        self.case = (kind, n, T, k, reset, box, horizon)
        self.kind, self.n, self.T, self.k, self.reset, self.box, self.horizon = kind, n, T, k, reset, box, horizon
        self.w = w = dict(dev_weights(kind), **(weights or {}))
        self.buf = {name: guarded(dt, n) for name, dt in RESULTS.items()}
        self.buf.update({name: guarded(dt, T * n * width) for name, (dt, width) in TRACES.items()})
        self.buf.update({name: guarded(dt, T * n) for name, dt in QS_TRACES.items()})
        self.tick = torch.tensor([tick, 0], dtype=torch.int64, device=DEV)
        if pos is None and not reset:
            pos = start_states(kind, n)
        self.pos = None if pos is None else torch.tensor(np.asarray(pos), dtype=torch.float64, device=DEV).contiguous()
        self.eps_safe = QC.eps_safe(kind, n, reset) if eps_safe is None else eps_safe
        p = _lib.ptr
        base = _lib.rrl_eval_rollout_t(n=n, T=T, H=256, d_obs=2, d_act=2, env_kind=2 if kind == "maze" else ENV_KIND[kind],
                                       reset=reset, pos=p(self.pos), seed=seed, counter=0, counter_dev=p(self.tick),
                                       eps_safe=self.eps_safe, **{name: p(w[name]) for name in NETS + QGROUP},
                                       **{name: p(t) for name, t in self.buf.items() if name not in QS_TRACES})
        lo, hi = box_dev(box)
        self.args = _lib.rrl_eval_rollout_qs_t(base=base, k=k, horizon=horizon, lo=p(lo), hi=p(hi),
                                               tr_pick=p(self.buf["tr_pick"]), tr_q=p(self.buf["tr_q"]))

    def run(self):
        _lib.check(_lib.load().rrl_eval_rollout_qs(C.byref(self.args), _lib.current_stream()), "rrl_eval_rollout_qs")
        return self.read()

    def read(self):
        out = {name: t.cpu().numpy() for name, t in self.buf.items()}
        out["tick"] = self.tick.cpu().tolist()
        return out


def packed_call(launches):
    args = (_lib.rrl_eval_rollout_qs_t * len(launches))(*[l.args for l in launches])
    return _lib.load().rrl_eval_rollout_qs_packed(len(launches), args, _lib.current_stream())


def same_bits(a, b):
    return all(a[name].tobytes() == b[name].tobytes() for name in a if name != "tick") and a["tick"] == b["tick"]


def views(out, n, T):
    """The used part of every buffer in its shape; asserts the guards behind it."""
    v = TG.views(out, n, T)
    for name, dt in QS_TRACES.items():
        assert (out[name][T * n:] == GUARD[dt]).all(), name
        v[name] = out[name][:T * n].reshape(T, n)
    return v


def gate_launch(kind, n, horizon, eps_safe, pos, tick):
    """One step of the EXISTING rollout entry with the Q_risk group only, at `pos` and `tick`: tr_task, tr_z and flags"""
    if kind == "maze":
        one = TM.Launch(n, 1, max(horizon, 1), True, 0, eps_safe=eps_safe, pos=pos, tick=tick)
    else:
        one = TG.Launch(kind, n, 1, True, 0, eps_safe=eps_safe, pos=pos, tick=tick)
    for name in RGROUP:
        setattr(one.args, name, None)
    return TG.views(one.run(), n, 1)


def check_case(l, out, float64=False):
    kind, n, T, k, reset, box, horizon = l.case
    v = views(out, n, T)
    flags = v["tr_flags"]
    # ---- alive from the trace itself; dead rows' entries untouched; tr_eps never written ----
    alive = np.ones((T, n), bool)
    for j in range(1, T):
        alive[j] = alive[j - 1] & ((flags[j - 1] >> 1) & 1 == 0)
    assert ((flags[alive] & 1) == 1).all() and (flags[~alive] == GUARD[torch.uint8]).all()
    for name, (dt, width) in TRACES.items():
        a = np.moveaxis(v[name], 1, 2) if name == "tr_z" else v[name]
        if name == "tr_eps":
            assert (a == GUARD[dt]).all()
            continue
        assert (a[~alive] == GUARD[dt]).all(), name
        assert np.isfinite(a[alive].astype(np.float64)).all() and (a[alive] != GUARD[dt]).all(), name
    assert out["tick"] == [QC.TICK + T + reset, 0]

    # ---- env, exact: a second env at the same seed and tick, stepped with the traced executed actions ----
    if kind == "maze":
        env = MazeVecEnv("maze", n, device=DEV, seed=QC.SEED, horizon=horizon, auto_reset=False)
    else:
        env = NavigationVecEnv(kind, n, device=DEV, seed=QC.SEED, auto_reset=False)
    env.tick[0] = QC.TICK
    if reset:
        env.reset()
    else:
        env.pos.copy_(torch.tensor(start_states(kind, n), device=DEV))
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

    # ---- per step: task and gate from the existing entry, candidates / scores / pick from rrl_qsample_act ----
    rec_bit = (flags >> 4) & 1 == 1
    gated = alive & rec_bit
    if n >= 17:          # the case's eps_safe splits its first-step q: rows of both kinds on step 0 already
        assert gated[0].any() and (alive[0] & ~gated[0]).any()
    W = {name[1:]: l.w[name] for name in QGROUP}
    W64 = QC.qrisk64(MC.weights32() if kind == "maze" else EC.weights32(kind))
    for j in range(T):
        ctr = QC.TICK + reset + j
        at = np.where(alive[j][:, None], v["tr_pos"][j], 0.0)
        w = gate_launch(kind, n, horizon, l.eps_safe, at, ctr)
        a = alive[j]
        assert v["tr_task"][j][a].tobytes() == w["tr_task"][0][a].tobytes(), j
        assert v["tr_z"][j][:, a].tobytes() == w["tr_z"][0][:, a].tobytes(), j
        assert np.array_equal(rec_bit[j][a], ((w["tr_flags"][0] >> 4) & 1 == 1)[a]), j
        g = gated[j]
        assert v["tr_real"][j][a & ~g].tobytes() == v["tr_task"][j][a & ~g].tobytes(), j
        assert (v["tr_pick"][j][~g] == GUARD[torch.int32]).all() and (v["tr_q"][j][~g] == GUARD[torch.float32]).all(), j
        if not g.any():
            continue
        cand = QC.candidates(g, n, k, box, ctr)
        obs32 = at.astype(np.float32)
        got = qsample_act(W, torch.tensor(obs32, device=DEV), k, box, mask=torch.tensor(g.astype(np.uint8), device=DEV),
                          cand_in=torch.tensor(cand, device=DEV))
        got = {name: t.cpu().numpy() for name, t in got.items()}
        rows = np.flatnonzero(g)
        assert got["cand"][rows].tobytes() == cand[rows].tobytes()
        assert v["tr_pick"][j][rows].tobytes() == got["pick"][rows].tobytes(), j
        assert v["tr_real"][j][rows].tobytes() == got["action"][rows].tobytes(), j
        assert v["tr_q"][j][rows].tobytes() == got["q"][rows, got["pick"][rows]].tobytes(), j
        assert v["tr_real"][j][rows].tobytes() == cand[rows, v["tr_pick"][j][rows]].tobytes(), j
        if float64:
            q64 = restate(W64, obs32[rows], cand[rows])["q"]
            gap = q64[np.arange(len(rows)), v["tr_pick"][j][rows]] - q64.min(1)
            print("step %d: %d gated rows, q64[pick] - min q64 <= %.3g (bar 2e-5)" % (j, len(rows), gap.max()))
            assert (gap <= 2e-5).all()
    return v, alive, gated


FLOAT64_SHAPES = {(17, 2, 1000), (65, 7, 130)}


@pytest.mark.parametrize("kind,n,T,k,reset,box", QC.nav_cases())
def test_rollout_navigation(kind, n, T, k, reset, box):
    l = Launch(kind, n, T, k, reset, box)
    out = l.run()
    check_case(l, out, float64=(n, T, k) in FLOAT64_SHAPES)
    assert same_bits(out, Launch(kind, n, T, k, reset, box).run())             # determinism


@pytest.mark.parametrize("n,T,k,horizon,reset", QC.maze_cases())
def test_rollout_maze(n, T, k, horizon, reset):
    l = Launch("maze", n, T, k, reset, "maze", horizon=horizon)
    out = l.run()
    check_case(l, out, float64=(n, T, k) in FLOAT64_SHAPES)
    assert same_bits(out, Launch("maze", n, T, k, reset, "maze", horizon=horizon).run())


def test_ties_and_nan():
    """Q_risk's last layers zero: every q equals sigmoid(b3)'s max, so every gated row picks candidate 0.  A NaN weight in one
    head: the gate drops the NaN head (fmaxf) and fires on the other, every candidate's q is NaN (it propagates through the
    max), the pick is 0 and tr_q holds the NaN."""
    kind, n, T, k = "navigation1", 17, 2, 130
    w = TG.dev_weights(kind)
    zero = {"qW3": torch.zeros_like(w["qW3"])}
    bad = w["qW3"].clone()
    bad.view(-1)[5] = float("nan")
    for weights, nan in ((zero, False), ({"qW3": bad}, True)):
        l = Launch(kind, n, T, k, 0, "unit", eps_safe=-1.0, weights=weights)
        v = views(l.run(), n, T)
        flags = v["tr_flags"]
        live = flags != GUARD[torch.uint8]
        assert live[0].all() and ((flags[live] >> 4) & 1 == 1).all()          # eps_safe = -1: every live row is gated
        assert (v["tr_pick"][live] == 0).all() and (v["tr_pick"][~live] == GUARD[torch.int32]).all()
        for j in range(T):
            for i in np.flatnonzero(live[j]):                                 # the executed action is candidate 0 of row i
                assert v["tr_real"][j][i].tobytes() == QC.candidates_row(int(i), k, "unit", QC.TICK + j)[0].tobytes()
        q = v["tr_q"][live]
        assert np.isnan(q).all() if nan else (np.isfinite(q).all() and (q == q[0]).all())


def test_outputs_do_not_depend_on_the_trace_nor_on_torchs_generator():
    full = Launch("navigation1", 65, 7, 130, 0, "unit")
    want = full.run()
    torch.manual_seed(12345)                                    # overwrite the global generators between two launches
    torch.cuda.manual_seed_all(999)
    state = torch.cuda.get_rng_state()
    bare = Launch("navigation1", 65, 7, 130, 0, "unit")
    for name in TRACES:
        setattr(bare.args.base, name, None)
    bare.args.tr_pick = bare.args.tr_q = None
    got = bare.run()
    assert torch.equal(state, torch.cuda.get_rng_state())       # ... and a launch draws nothing from them
    for name in RESULTS:
        assert got[name].tobytes() == want[name].tobytes()
    for name, dt in list((k, d) for k, (d, _) in TRACES.items()) + list(QS_TRACES.items()):
        assert (got[name] == GUARD[dt]).all()
    assert got["tick"] == want["tick"]
    assert same_bits(want, Launch("navigation1", 65, 7, 130, 0, "unit").run())


def test_draws_are_keyed_by_the_env_row_alone():
    """Rows 0 .. 15 of an n = 65 launch and an n = 16 launch with the same row seeds, start states and eps_safe: the same
    results and traces -- candidate c of row i is keyed by i k + c, whatever n is and whichever other rows are gated."""
    kind, T, k = "navigation2", 7, 65
    big = Launch(kind, 65, T, k, 0, "asym")
    small = Launch(kind, 16, T, k, 0, "asym", eps_safe=big.eps_safe, pos=EC.start_states(kind, 65)[:16])
    a, b = views(big.run(), 65, T), views(small.run(), 16, T)
    assert ((a["tr_flags"][:, :16] >> 4) & 1 == 1).any()
    for name in RESULTS:
        assert a[name][:16].tobytes() == b[name].tobytes(), name
    for name in list(TRACES) + list(QS_TRACES):
        x = a[name][:, :, :16] if name == "tr_z" else a[name][:, :16]
        assert np.ascontiguousarray(x).tobytes() == b[name].tobytes(), name


@pytest.mark.parametrize("S", [2, 3])
def test_packed_launch_is_the_solo_launches(S):
    """S seeds that differ in n, T, k, kind within Navigation, reset, box and weights: each seed's outputs, traces and own tick
    equal its solo launch bit for bit."""
    cases = [("navigation1", 65, 7, 130, 0, "unit"), ("navigation2", 17, 2, 17, 1, "asym"), ("navigation2", 3, 1, 1024, 1, "unit")][:S]
    solo = [Launch(*c).run() for c in cases]
    launches = [Launch(*c) for c in cases]
    _lib.check(packed_call(launches), "rrl_eval_rollout_qs_packed")
    for c, a, l in zip(cases, solo, launches):
        b = l.read()
        assert same_bits(a, b), c
        assert b["tick"] == [QC.TICK + c[2] + c[4], 0]
    assert any(((views(a, c[1], c[2])["tr_flags"] >> 4) & 1 == 1).any() for c, a in zip(cases, solo))


def test_packed_maze_launch_with_different_horizons():
    cases = [(65, 7, 65, 3, 0), (17, 2, 17, 100, 1)]
    mk = lambda n, T, k, h, reset: Launch("maze", n, T, k, reset, "maze", horizon=h)
    solo = [mk(*c).run() for c in cases]
    launches = [mk(*c) for c in cases]
    _lib.check(packed_call(launches), "rrl_eval_rollout_qs_packed")
    for c, a, l in zip(cases, solo, launches):
        assert same_bits(a, l.read()), c


def test_packed_mix_of_navigation_and_maze_is_refused_and_writes_nothing():
    launches = [Launch("navigation1", 17, 2, 17, 0, "unit"), Launch("maze", 17, 2, 17, 0, "maze", horizon=100)]
    fresh = [l.read() for l in launches]
    assert packed_call(launches) == EINVAL
    torch.cuda.synchronize()
    for a, l in zip(fresh, launches):
        assert same_bits(a, l.read())
