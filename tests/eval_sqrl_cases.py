"""Inputs of the rrl_eval_rollout_sqrl tests (SQRL constraint sampling inside the evaluation rollout) and the float64
restatement of the whole rollout they are judged by.

Built on eval_cases.py / eval_maze_cases.py: their agents, start states and env, with two changes.  The task policy's last
layer is the stacked four rows (mean_linear, then log_std_linear: the head rrl_sqrl_act_t.head describes), and the action
columns of Q_risk's first layers are multiplied by 10: with the unmodified agents q moves only 0.02 across the candidates of a
row, so almost no row has a mixed safe set; with the factor the per-row spread is 0.15 - 0.2.  The draws of streams 14 / 15 are
regenerated through `oracle.c_oracle` (`normals` = `normal2` row by row, `philox4x32`, `test_sqrl_act_cpu.unit_open`), keyed as
the kernel keys them: candidate row = env row * k + c, pick row = env row, counter = tick + reset + step.  Scores and pick in
float64 are `test_sqrl_act_cpu.restate_scores` / `restate_pick`.  tests/test_eval_sqrl_cpu.py proves that the cases are fair;
tests/test_eval_sqrl_gpu.py measures the kernels on them.  Computed once, shared, read-only."""
import copy
import functools

import numpy as np
import torch

import eval_cases as EC
import eval_maze_cases as MC
from oracle import c_oracle as co
from test_sqrl_act_cpu import restate_pick, restate_scores, unit_open

STREAM_EVAL_SQRL, STREAM_EVAL_SQRL_PICK = 14, 15
# The tick: the first one from eval_cases.TICK (37) on at which EVERY case's float64 restatement meets ambiguous_share_ok
# below.  No threshold can help a row on the argmin branch whose two smallest q lie within 1e-6 of each other (restate_pick
# calls that ambiguous): at tick 37 two such rows (35 and 53 of Navigation 2, n = 65, k = 128, step 0) leave 2 of the 65 pairs
# of the T = 1 case ambiguous against a cap of 1, at tick 38 Navigation 2 (17, 7, 64) reset 0 misses it; at 39 every case
# holds.  Found from the restatement alone, on the CPU.
SEED, TICK = EC.SEED, 39
ACTION_GAIN = 10.0                 # on qW1[:, :, 2:4]
NS, TS, KS = (1, 17, 65), (1, 2, 7), (1, 16, 17, 64, 65, 100, 128)
# (n, T, k): one row / one tile + 1 row / several tiles with a ragged last one; one candidate / one row tile / + 1 / one full
# pass / + 1 / the production count / the maximum; then one whole episode
SHAPES = [(n, T, k) for n in NS for T in TS for k in KS] + [(65, 101, 17)]
MODES = ("mixed", "none_safe", "all_safe")
EXTREME_SHAPES = [(17, 2, 100), (65, 7, 17)]          # the shapes of the eps_safe 0 / 1 cases (two per kind: one each)
# Maze: (n, T, k, horizon) -- a reduced subset at the env's own horizon and at one that ends rows
MAZE_SHAPES = [(1, 1, 1, 100), (17, 2, 17, 100), (17, 7, 64, 3), (65, 7, 65, 3), (65, 7, 100, 100), (17, 2, 128, 100)]


def nav_cases():
    """(kind, n, T, k, reset, mode): every shape x both env kinds x reset 0 / 1 at the mixed threshold, then per kind one
    case with nothing safe (eps_safe 0) and one with everything safe (eps_safe 1)"""
    out = [(kind, n, T, k, reset, "mixed") for kind in EC.KINDS for (n, T, k) in SHAPES for reset in (0, 1)]
    for kind in EC.KINDS:
        out += [(kind,) + EXTREME_SHAPES[0] + (0, "none_safe"), (kind,) + EXTREME_SHAPES[1] + (1, "all_safe")]
    return out


def maze_cases():
    """(n, T, k, horizon, reset, mode)"""
    out = [(n, T, k, h, reset, "mixed") for (n, T, k, h) in MAZE_SHAPES for reset in (0, 1)]
    return out + [(17, 2, 17, 100, 0, "none_safe"), (17, 7, 64, 3, 1, "all_safe")]


@functools.lru_cache(maxsize=None)
def agent(kind):
    """A copy of the kind's agent (eval_cases.agent / eval_maze_cases.agent; the shared one is left alone) with the action
    columns of Q_risk's first layers multiplied by ACTION_GAIN"""
    ag = copy.deepcopy(MC.agent() if kind == "maze" else EC.agent(kind))
    qr = ag.safety_critic.safety_critic
    with torch.no_grad():
        for lin in (qr.linear1, qr.linear4):
            lin.weight[:, 2:4].mul_(ACTION_GAIN)
    return ag


@functools.lru_cache(maxsize=None)
def weights32(kind):
    """The flat float32 arrays the kernel reads, by descriptor field: the kind's own with pW3 / pb3 the stacked four rows
    and the scaled qW1 (taken from the modified agent, so that the modules and the arrays hold the same bits)"""
    ag = agent(kind)
    w = dict(MC.weights32() if kind == "maze" else EC.weights32(kind))
    pol, qr = ag.policy, ag.safety_critic.safety_critic
    (mw, mb), (lw, lb) = EC._lin(pol.mean_linear), EC._lin(pol.log_std_linear)
    w["pW3"], w["pb3"] = np.concatenate([mw, lw]), np.concatenate([mb, lb])
    w["qW1"] = np.stack([EC._lin(qr.linear1)[0], EC._lin(qr.linear4)[0]])
    assert w["pW3"].shape == (4, 256) and w["qW1"].shape == (2, 256, 4)
    for v in w.values():
        v.setflags(write=False)
    return w


def qrisk64(kind):
    """restate_scores' weights: [(W1, b1, W2, b2, W3, b3)] * 2 in float64"""
    w = weights32(kind)
    return [tuple(w[name][h].astype(np.float64) for name in ("qW1", "qb1", "qW2", "qb2", "qW3", "qb3")) for h in range(2)]


def head_chain(kind, obs, dtype=np.float64):
    """The task policy's four last-layer outputs [m, 4] at float32 inputs, the numpy chain in `dtype`"""
    w = {k: v.astype(dtype) for k, v in weights32(kind).items() if k.startswith("p")}
    return EC._mlp64(np.asarray(obs, np.float32).astype(dtype), w["pW1"], w["pb1"], w["pW2"][0], w["pb2"], w["pW3"], w["pb3"])


@functools.lru_cache(maxsize=None)
def noise(n, k, tick, seed=SEED):
    """eps [n, k, 2] f32: the normal pair of Philox (seed, row i k + c, stream 14, tick), rounded to float32"""
    e = co.normals(seed, n * k, STREAM_EVAL_SQRL, tick).astype(np.float32).reshape(n, k, 2)
    e.setflags(write=False)
    return e


@functools.lru_cache(maxsize=None)
def uniforms(n, tick, seed=SEED, stream=STREAM_EVAL_SQRL_PICK):
    """u [n] f64: the open-unit double of the low 64 bits of Philox (seed, row i, stream 15, tick)"""
    u = np.empty(n, np.float64)
    for i in range(n):
        w = co.philox4x32((i, stream, tick & 0xFFFFFFFF, tick >> 32), (seed & 0xFFFFFFFF, seed >> 32))
        u[i] = unit_open((w[1] << 32) | w[0])
    u.setflags(write=False)
    return u


def start_states(kind, n):
    return MC.start_states(n) if kind == "maze" else EC.start_states(kind, n)


@functools.lru_cache(maxsize=None)
def first_states(kind, n, reset):
    """The case's states before step 0: the env's own reset at (SEED, TICK), or the start states of the kind's case file"""
    if not reset:
        return start_states(kind, n).copy()
    if kind == "maze":
        return co.maze_reset(n, mode=0, check_constraint=True, seed=SEED, counter=TICK)[0]
    return co.nav_reset(kind, n, seed=SEED, counter=TICK)[0]


def scores64(kind, obs32, k, ctr, n=None):
    """restate_scores at obs32 [n, 2] with the float64 head and the regenerated noise of counter `ctr`"""
    w = weights32(kind)
    n = len(obs32) if n is None else n
    return restate_scores(qrisk64(kind), head_chain(kind, obs32), obs32, noise(n, k, ctr),
                          scale=w["scale"].astype(np.float64), bias=w["bias"].astype(np.float64))


NEIGHBOURHOOD = 16                 # distinct values on either side of the median position whose gaps are the candidates
LEFT_OUT = 0.02                    # test_sqrl_act_cpu.left_out_cap: the share of rows a test may leave out as ambiguous


def thresholds(kind, n, k, reset):
    """The candidate thresholds of a mixed case, as float32, best first: the midpoints of the gaps between consecutive distinct
    step-0 q64 values among the NEIGHBOURHOOD values on either side of the median of the per-row medians, widest gap first
    (the plain rule -- the two values that bracket the median -- left rows within 1e-5 of the threshold; eval_cases.eps_safe
    has the reasons).  One distinct value (n = k = 1): half-way between it and 1, as test_sqrl_act_cpu.thresholds."""
    q = scores64(kind, first_states(kind, n, reset).astype(np.float32), k, TICK + reset)["q"]
    s = np.unique(q)
    if s.size == 1:
        return [float(np.float32(0.5 * (s[0] + 1.0)))]
    m = int(np.clip(np.searchsorted(s, np.median(np.median(q, 1))), 1, s.size - 1))
    lo, hi = max(1, m - NEIGHBOURHOOD), min(s.size - 1, m + NEIGHBOURHOOD)        # gaps s[i - 1] .. s[i] for i in [lo, hi]
    order = np.argsort(-(s[lo:hi + 1] - s[lo - 1:hi]), kind="stable")
    return [float(np.float32(0.5 * (s[lo + i - 1] + s[lo + i]))) for i in order]


def ambiguous_share_ok(r):
    """The condition a case's threshold has to meet, on the restatement alone: at most LEFT_OUT of the live (row, step) pairs
    of its float64 rollout are ambiguous by restate_pick's own definition"""
    return int((r["ambiguous"] & r["alive"]).sum()) <= int(LEFT_OUT * r["alive"].sum())


@functools.lru_cache(maxsize=None)
def _case(kind, n, T, k, reset, mode, horizon):
    """(eps_safe, float64 rollout) of a case.  The rollout goes on for T steps and a candidate's q drifts through any fixed
    value sooner or later (with every row mixed, about k * 2e-5 / 0.15 of the pairs fall within 1e-5 of a threshold: the cap
    itself at k = 128), so the widest step-0 gap alone does not keep a case inside the cap: the threshold is the first of
    thresholds() whose whole float64 rollout meets ambiguous_share_ok -- chosen from the restatement, never from a kernel."""
    if mode != "mixed":
        eps_s = {"none_safe": 0.0, "all_safe": 1.0}[mode]
        return eps_s, _rollout64(kind, n, T, k, reset, eps_s, horizon)
    tried = thresholds(kind, n, k, reset)
    for eps_s in tried:
        r = _rollout64(kind, n, T, k, reset, eps_s, horizon)
        if ambiguous_share_ok(r):
            return eps_s, r
    return tried[0], _rollout64(kind, n, T, k, reset, tried[0], horizon)      # (test_eval_sqrl_cpu.py fails on such a case)


def eps_safe(kind, n, T, k, reset, mode="mixed", horizon=None):
    """The case's threshold as float32 (mode none_safe: 0, all_safe: 1)"""
    return _case(kind, n, T, k, reset, mode, horizon)[0]


def rollout64(kind, n, T, k, reset, mode="mixed", horizon=None):
    """The case's float64 rollout (_rollout64 at its eps_safe)"""
    return _case(kind, n, T, k, reset, mode, horizon)[1]


def _rollout64(kind, n, T, k, reset, eps_s, horizon=None):
    """The whole rollout with the float64 networks, the regenerated draws and the oracle env (kind "maze": with `horizon`).
    Per step [T, n]: `alive`, `n_safe`, `cstar`, `pick`, `ambiguous` (restate_pick's own definition), the states `obs`
    [T, n, 2] f32 and the executed `real` [T, n, 2] f32 with their float64 `real64`; per row how it ended."""
    maze = kind == "maze"
    pos = first_states(kind, n, reset)
    alive = np.ones(n, bool)
    out = {"alive": np.zeros((T, n), bool), "n_safe": np.zeros((T, n), np.int64), "cstar": np.full((T, n), -1),
           "pick": np.zeros((T, n), np.int64), "ambiguous": np.zeros((T, n), bool), "obs": np.zeros((T, n, 2), np.float32),
           "real": np.zeros((T, n, 2), np.float32), "real64": np.zeros((T, n, 2)),
           "constraint": np.zeros(n, bool), "success": np.zeros(n, bool)}
    for j in range(T):
        ctr = TICK + reset + j
        obs = pos.astype(np.float32)
        sc = scores64(kind, obs, k, ctr)
        pk = restate_pick(sc["q"], sc["logp"], uniforms(n, ctr), eps_s)
        real64 = sc["cand"][np.arange(n), pk["pick"]]
        real = real64.astype(np.float32)
        out["alive"][j], out["obs"][j], out["real"][j], out["real64"][j] = alive, obs, real, real64
        for name in ("n_safe", "cstar", "pick", "ambiguous"):
            out[name][j] = pk[name]
        if maze:
            step = co.maze_step(pos, real, np.full(n, j, np.int32), seed=SEED, counter=ctr, horizon=horizon, auto_reset=False)
        else:
            step = co.nav_step(kind, pos, real, np.zeros(n, np.int32), seed=SEED, counter=ctr, horizon=1 << 30, auto_reset=False)
        out["constraint"] |= alive & step["constraint"].astype(bool)
        out["success"] |= alive & step["success"].astype(bool)
        pos = np.where(alive[:, None], step["pos"], pos)
        alive = alive & ~step["done"].astype(bool)
    out["survived"] = alive
    for v in out.values():
        v.setflags(write=False)
    return out
