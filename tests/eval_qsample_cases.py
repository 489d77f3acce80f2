"""Inputs of the rrl_eval_rollout_qs tests (Q-sampling recovery inside the evaluation rollout) and the float64 restatement of
the whole rollout they are judged by.

Built on eval_cases.py / eval_maze_cases.py: their agents (Q_risk and the task policy; the recovery policy is not used), start
states and eps_safe, which already give a mixed gate.  The candidates of stream 13 are regenerated through the C oracle's
Philox (`oracle.c_oracle.philox4x32`) and `test_qsample_act_cpu.unit_open`, keyed as the kernel keys them: row = env row * k + c,
counter = tick + reset + step.  Scores and pick in float64 are `test_qsample_act_cpu.restate`.  tests/test_eval_qsample_cpu.py
proves that the cases are fair; tests/test_eval_qsample_gpu.py measures the kernels on them.  Computed once, shared,
read-only."""
import functools

import numpy as np

import eval_cases as EC
import eval_maze_cases as MC
from oracle import c_oracle as co
from test_qsample_act_cpu import BOXES, restate, unit_open

STREAM_EVAL_QSAMPLE = 13
SEED, TICK = EC.SEED, EC.TICK
NS, TS, KS = (1, 17, 65), (1, 2, 7), (1, 17, 64, 65, 130)
# (n, T, k): one row / one tile + 1 row / several tiles with a ragged last one; one candidate / one row tile + 1 / one full pass
# / one pass + 1 / three passes with a tail; then the production count, the maximum, and one full episode
SHAPES = [(n, T, k) for n in NS for T in TS for k in KS] + [(17, 2, 1000), (3, 1, 1024), (65, 101, 17)]
NAV_BOXES = ("unit", "asym")
# Maze, the +-0.1 box: (n, T, k, horizon) -- a reduced subset of the shapes at the env's own horizon and at one that ends rows
MAZE_SHAPES = [(1, 1, 1, 100), (17, 2, 17, 100), (17, 7, 64, 3), (65, 7, 65, 3), (65, 7, 130, 100), (17, 2, 1000, 100)]


def nav_cases():
    """(kind, n, T, k, reset, box): every shape x both env kinds x reset 0 / 1 x both boxes"""
    return [(kind, n, T, k, reset, box) for kind in EC.KINDS for (n, T, k) in SHAPES for reset in (0, 1) for box in NAV_BOXES]


def maze_cases():
    """(n, T, k, horizon, reset), box "maze" """
    return [(n, T, k, h, reset) for (n, T, k, h) in MAZE_SHAPES for reset in (0, 1)]


@functools.lru_cache(maxsize=None)
def uniforms_row(row, k, stream, seed, tick):
    """u [k, 2] f64 of env row `row`: the open-unit doubles of the low and the high 64 bits of Philox (seed, row k + c, stream,
    tick) -- test_qsample_act_cpu.uniforms with the stream as a parameter, one env row at a time."""
    u = np.empty((k, 2), np.float64)
    for c in range(k):
        w = co.philox4x32(((row * k + c) & 0xFFFFFFFF, stream, tick & 0xFFFFFFFF, tick >> 32), (seed & 0xFFFFFFFF, seed >> 32))
        u[c] = unit_open((w[1] << 32) | w[0]), unit_open((w[3] << 32) | w[2])
    u.setflags(write=False)
    return u


def candidates_row(row, k, box, tick, seed=SEED, stream=STREAM_EVAL_QSAMPLE):
    """a_j = float(double(lo_j) + (double(hi_j) - double(lo_j)) u_j) [k, 2] f32: double arithmetic, one rounding"""
    lo, hi = (np.asarray(b, np.float32).astype(np.float64) for b in BOXES[box])
    return (lo + (hi - lo) * uniforms_row(row, k, stream, seed, tick)).astype(np.float32)


def candidates(rows, n, k, box, tick, seed=SEED):
    """[n, k, 2] f32 with the candidates of the env rows in `rows` (a bool mask [n]) and zeros elsewhere"""
    out = np.zeros((n, k, 2), np.float32)
    for i in np.flatnonzero(rows):
        out[i] = candidates_row(int(i), k, box, tick, seed)
    return out


def qrisk64(w):
    """test_qsample_act_cpu.restate's weights from a weights32 dict: [(W1, b1, W2, b2, W3, b3)] * 2 in float64"""
    return [tuple(w[name][h].astype(np.float64) for name in ("qW1", "qb1", "qW2", "qb2", "qW3", "qb3")) for h in range(2)]


def eps_safe(kind, n, reset):
    """The case's split of its own first-step q64 (eval_cases.eps_safe); too few rows to split (n < 4): the 130-row value"""
    if kind == "maze":
        return MC.eps_safe(n if n >= 4 else 130, reset)
    return EC.eps_safe(kind, n if n >= 4 else 130, reset)


def first_states(kind, n, reset):
    return MC.first_states(n, reset) if kind == "maze" else EC.first_states(kind, n, reset)


@functools.lru_cache(maxsize=None)
def rollout64(kind, n, T, k, reset, box, horizon=None):
    """The whole rollout with float64 networks, the regenerated candidates and the oracle env (kind "maze": with `horizon`).
    Per step `alive`, `gate` (of live rows) [T, n], the executed `real` [T, n, 2] f32, the `pick` [T, n] (-1 where none); per
    row how it ended."""
    maze = kind == "maze"
    nets = MC.networks64 if maze else functools.partial(EC.networks64, kind)
    W = qrisk64(MC.weights32() if maze else EC.weights32(kind))
    pos = first_states(kind, n, reset)
    alive = np.ones(n, bool)
    eps_s = eps_safe(kind, n, reset)
    out = {"alive": np.zeros((T, n), bool), "gate": np.zeros((T, n), bool), "real": np.zeros((T, n, 2), np.float32),
           "pick": np.full((T, n), -1), "constraint": np.zeros(n, bool), "success": np.zeros(n, bool)}
    for j in range(T):
        ctr = TICK + reset + j
        obs = pos.astype(np.float32)
        task = nets(obs)["task"].astype(np.float32)
        gate = (nets(obs, task=task)["q"] > eps_s) & alive
        real = task.copy()
        if gate.any():
            g = np.flatnonzero(gate)
            cand = candidates(gate, n, k, box, ctr)[g]
            pick = restate(W, obs[g], cand)["pick"]
            real[g] = cand[np.arange(len(g)), pick]
            out["pick"][j][g] = pick
        out["alive"][j], out["gate"][j], out["real"][j] = alive, gate, real
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
