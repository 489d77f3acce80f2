"""Case machinery of the f16x3 Q-sampling acting tests (test_qsample_f16x3_cpu.py, test_qsample_f16x3_gpu.py): the inputs of
tests/test_qsample_act_cpu.py (make_agent, observations, candidates, case, weights64, PHILOX_SEED, TICK), its float64 chain
`restate` as the reference, and the host restatement of the f16x3 score chain of tests/sqrl_f16x3_cases.py (emulate_z) on the
rows [obs | candidate].  No test functions here.

The case table -- the smallest shapes at which the kernel can go wrong:
    n in (1, 3, 65) x k in (1, 16, 17, 128, 129, 1000, 1024)   one row, one tile, tile + 1, one chunk, chunk + 1, the production
                                                                count (7 chunks + 104 rows), the maximum; all on the `unit` box
    (3, 129) and (3, 1000) on the `maze` box                    +-0.1: small activations, lo parts near the f16 subnormals
    (3, 129) and (3, 1000) on the `asym` box
subnormal_lo_flushed (sqrl_f16x3_cases.MUTATIONS) is seen by every case as drawn -- W2's lo parts are subnormal f16 values at
this width -- so no `maze` case had to be scaled (test_qsample_f16x3_cpu.py states which case sees which mutation).

Rule Z (the project's rule, sqrl_f16x3_cases.bound / deviation, FACTOR = 4): the kernel's largest |z - z64| over the gated rows
of a case is at most B = 4 x max(the f32 emulation's largest deviation on that case, 2^-23 x max |z64|); a non-finite value
where float64 is finite is an infinite deviation.
Rule Q, derived from rule Z: sigmoid is 1/4-Lipschitz, so |q - q64| <= B / 4 for every row; the kernel picks the argmin of its
own q, so in float64 the picked candidate is worse than the true minimum by at most 2 x B / 4:
    q64[e, pick[e]] <= q64[e].min() + B / 2."""
import functools

import numpy as np

import sqrl_f16x3_cases as SC
from test_qsample_act_cpu import (BOXES, KS, NS, PHILOX_SEED, TICK, argmin_first, candidates, case, make_agent,  # noqa: F401
                                  observations, restate, weights64)

CASES = tuple((n, k, "unit") for n in NS for k in KS) + tuple((3, k, box) for box in ("maze", "asym") for k in (129, 1000))
SAT_SHAPE = (3, 17, "unit")


@functools.lru_cache(maxsize=None)
def agent(box):
    return make_agent("cpu", box)


@functools.lru_cache(maxsize=None)
def weights(box):
    """The twin heads of the box's agent as float64 numpy (weights64 of the f32 tests)."""
    return weights64(agent(box).safety_critic.safety_critic)


def rows_of(obs, cand):
    """[n k, 4] float64 rows [obs | candidate]"""
    cand = np.asarray(cand, np.float64)
    obs = np.broadcast_to(np.asarray(obs, np.float64)[:, None, :], cand.shape)
    return np.concatenate([obs, cand], -1).reshape(-1, 4)


def emulate(W, obs, cand, dtype=np.float64, mutation=None):
    """{"z": [2, n, k], "q": [n, k]} of the emulated f16x3 chain (float64 values of `dtype` arithmetic)."""
    n, k = cand.shape[:2]
    z = SC.emulate_z(W, rows_of(obs, cand), dtype, mutation).astype(np.float64).reshape(2, n, k)
    return {"z": z, "q": SC.q_of(z)}


def bound_on(z64, z32, rows):
    """Rule Z's bound B over the env rows `rows` (bool [n] or index array) of a case."""
    return SC.bound(z64[:, rows], z32[:, rows])


def rule_q_holds(q64, pick, B):
    """Rule Q on the rows given: q64 [m, k], pick [m]."""
    return bool((q64[np.arange(len(pick)), pick] <= q64.min(1) + B / 2).all())


@functools.lru_cache(maxsize=None)
def table_case(n, k, box):
    """One case of the table: the f32 tests' case (obs, cand, float64 z / q / pick) plus both emulations' z.  Computed once and
    shared; nobody writes to it."""
    c = dict(case(n, k, box))
    W = weights(box)
    c["e64"] = emulate(W, c["obs"], c["cand"], np.float64)
    c["e32"] = emulate(W, c["obs"], c["cand"], np.float32)
    for e in (c["e64"], c["e32"]):
        for v in e.values():
            v.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def saturation_case():
    """The (3, 17) case with its observations scaled by sqrl_f16x3_cases.SAT_SCALE = 2^21: layer-1 activations beyond the f16
    range.  Its reference (z, q, pick) is the float64 EMULATION -- the clamp is part of the contract; the plain chain does not
    saturate.  `saturated`: the share of layer-1 activations above 65504."""
    n, k, box = SAT_SHAPE
    W = weights(box)
    obs = (observations(n, k) * np.float32(SC.SAT_SCALE)).astype(np.float32)
    cand = candidates(n, k, box)
    e64, e32 = emulate(W, obs, cand, np.float64), emulate(W, obs, cand, np.float32)
    h1 = np.maximum(rows_of(obs, cand) @ W[0][0].T + W[0][1], 0)
    c = {"obs": obs, "cand": cand, "z": e64["z"], "q": e64["q"], "pick": argmin_first(e64["q"]), "e64": e64, "e32": e32,
         "saturated": float((h1 > SC.F16_MAX).mean())}
    for v in (c["obs"], c["cand"], c["z"], c["q"], c["pick"]):
        v.setflags(write=False)
    return c
