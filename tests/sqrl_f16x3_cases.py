"""Case machinery of the f16x3 SQRL acting tests (test_sqrl_f16x3_cpu.py, test_sqrl_f16x3_gpu.py): the shapes and modes of
tests/test_sqrl_act_cpu.py, plus the restatement of the f16x3 score chain on the host.

The emulated chain is restate_scores' (float64, or the same text in f32) with layer 2's two operands replaced by their f16
splits -- v -> hi = f16(min(v, 65504)), lo = f16(v - hi), w -> hi = f16(w), lo = f16(w - hi) -- and the three products the
kernel forms, act_hi w_lo + act_hi w_hi + act_lo w_hi (lo lo dropped).  numpy's summation order is not the kernel's: the
emulation states the OPERAND error of the arithmetic, and the rule below leaves a factor 4 for the order.

The rule on z (the planner tests' rule 1, tests/plan_cases.py): the kernel's largest deviation from float64 is at most
FACTOR x max(the f32 emulation's largest deviation on that case, 2^-23 of the largest |z|).  `MUTATIONS` are the mistakes an
f16x3 kernel can make without failing to run; each is stated as a variant of the f32 emulation, and
test_sqrl_f16x3_cpu.py shows on which case the rule sees it."""
import numpy as np

from test_sqrl_act_cpu import KS, MODES, NS, case, restate_pick, restate_scores, thresholds, weights64  # noqa: F401

FACTOR = 4.0
F16_MAX = 65504.0
SHAPES = tuple((n, k) for n in NS for k in KS)
MUTATIONS = ("act_lo_w_hi_dropped", "act_hi_w_lo_dropped", "subnormal_lo_flushed", "no_clamp")
SAT_SCALE = 2.0 ** 21                 # the saturation case: observations times this put layer-1 activations far above 65504


def split16(v, dtype, clamp=True, flush=False):
    """hi, lo of the kernel's split16 (and of rrl_w2_pack_f16x3: |v| clamped), as `dtype` arrays holding f16 values."""
    v = np.asarray(v, dtype)
    if clamp:
        v = np.where(v > F16_MAX, dtype(F16_MAX), np.where(v < -F16_MAX, dtype(-F16_MAX), v))     # NaN compares false: kept
    with np.errstate(over="ignore", invalid="ignore"):
        hi = v.astype(np.float16)
        lo = (v - hi.astype(dtype)).astype(np.float16)
    if flush:
        lo = np.where(np.abs(lo) < 2.0 ** -14, np.float16(0), lo)
    return hi.astype(dtype), lo.astype(dtype)


def emulate_z(W, x, dtype=np.float64, mutation=None):
    """z [2, rows] of the twin heads on the input rows x [rows, 4] with layer 2 in f16x3, in `dtype` arithmetic."""
    assert mutation is None or mutation in MUTATIONS
    flush, clamp = mutation == "subnormal_lo_flushed", mutation != "no_clamp"
    x = np.asarray(x, dtype)
    out = []
    with np.errstate(over="ignore", invalid="ignore"):
        for W1, b1, W2, b2, W3, b3 in ([np.asarray(t, dtype) for t in head] for head in W):
            a_hi, a_lo = split16(np.maximum(x @ W1.T + b1, 0), dtype, clamp=clamp, flush=flush)
            w_hi, w_lo = split16(W2, dtype, flush=flush)
            h2 = a_hi @ w_hi.T
            if mutation != "act_hi_w_lo_dropped":
                h2 = h2 + a_hi @ w_lo.T
            if mutation != "act_lo_w_hi_dropped":
                h2 = h2 + a_lo @ w_hi.T
            out.append(np.maximum(h2 + b2, 0) @ W3.T[:, 0] + b3[0])
    return np.stack(out)


def inputs_of(c):
    """[n k, 4] float64 rows [obs | candidate] of a case (the float64 restatement's candidates)."""
    cand = c["scores"]["cand"]
    obs = c["obs"].cpu().numpy().astype(np.float64)
    return np.concatenate([np.broadcast_to(obs[:, None, :], cand.shape), cand], -1).reshape(-1, 4)


def q_of(z):
    with np.errstate(over="ignore"):
        return (1.0 / (1.0 + np.exp(-z.astype(np.float64)))).max(0)


def emulate(W, c, dtype=np.float64, mutation=None):
    """{"z": [2, n, k], "q": [n, k]} of case c on the emulated chain (float64 values of `dtype` arithmetic)."""
    n, k = c["scores"]["q"].shape
    z = emulate_z(W, inputs_of(c), dtype, mutation).astype(np.float64).reshape(2, n, k)
    return {"z": z, "q": q_of(z)}


def bound(z64, z32):
    """The rule's bound on max |z - z64| for a case whose f32 emulation is z32."""
    return FACTOR * max(float(np.abs(z32 - z64).max()), 2.0 ** -23 * float(np.abs(z64).max()))


def deviation(z, z64):
    d = np.abs(np.asarray(z, np.float64) - z64)
    return float("inf") if not np.isfinite(d).all() else float(d.max())


# ---- the case beside the 15 shapes ---- ---------------------------------------------------------------------------------
def saturation_case(agent, n=3, k=17, device="cpu"):
    """The (3, 17) case with its observations scaled by SAT_SCALE: layer-1 activations beyond the f16 range.  Its float64
    reference is the float64 EMULATION (the clamp is part of the contract; the plain chain does not saturate)."""
    c = dict(case(agent, n, k, device=device))
    c["obs"] = c["obs"] * SAT_SCALE
    W = weights64(agent)
    sc = restate_scores(W, c["head"].cpu().numpy(), c["obs"].cpu().numpy(), c["eps"])
    c["scores"] = sc
    x = inputs_of(c)
    h1 = np.maximum(x @ W[0][0].T + W[0][1], 0)
    c["saturated"] = float((h1 > F16_MAX).mean())
    return c

