"""Cases, NumPy restatements and launch helpers for the CEM bookkeeping kernels (csrc/cem_kernels.hip: cem_sample_kernel,
cem_update_kernel, cem_begin_kernel, cem_finish_kernel behind rrl_cem_sample / rrl_cem_update / rrl_cem_begin / rrl_cem_finish),
shared by test_cem_paths_cpu.py and test_cem_paths_gpu.py.

The kernels are written to reproduce the C oracle bit for bit, so there is no tolerance anywhere: the GPU tests compare with
np.array_equal / tobytes.  What this module adds to the oracle:

restate_update() is optimizers.py:104-117 of the reference in NumPy float64 -- NaN costs count as float32(1e6), the order is
(cost, index), the elite mean and the population variance are plain sequential float64 sums in sorted elite order without fused
multiply-add, blended with alpha.  It never calls the oracle: it pins the oracle where the two golden cases of mpc_golden.npz do
not reach (test_cem_paths_cpu.py compares the two bit for bit on every update case).

restate_begin() / restate_finish() are the host-count path of MPC.act: mask.nonzero(), the gather of the warm starts and the
observations, the scatter of the first action and of the solution shifted by one step.  Both work on copies of the WHOLE output
buffers, so an element the kernel must not write is compared as well.

Every launch helper allocates each output with guard elements behind it, filled with a sentinel no result can hold.  The samples
of an update launch carry `padded - pop` extra rows of 1e30 behind the last problem (padded = pop rounded up to a power of two, as
in rrl_cem_update): whatever key index the bitonic sort can produce, valid or padding, reads memory the test owns, and a padding
key chosen as an elite shows up as a huge mean instead of an out-of-bounds read.

The constants of the launches are literals here; test_cem_paths_cpu.py parses them out of the sources and proves that the tables
reach every edge they claim."""
import collections
import functools

import numpy as np

# ---- the launches' constants, as literals (test_cem_paths_cpu.py compares them with the sources) ------------------------------
CONSTANTS = dict(kBlock=256, kMaxGrid=2048, kBeginBlock=1024, max_pop=1024, max_dim=64)
K_BLOCK, K_MAX_GRID, K_BEGIN_BLOCK, MAX_POP, MAX_DIM = 256, 2048, 1024, 1024, 64
STRIDE_ELEMENTS = K_MAX_GRID * K_BLOCK          # above this many elements a grid_for() launch walks its grid-stride loop
WAVE = 64
STREAM_CEM = 5                                  # RRL_STREAM_CEM
EPSILON = 1e-3                                  # CEMOptimizer's default
SEED = 9
NAN_COST = np.float32(1e6)

# sentinels: what a buffer holds where nothing may write
S_SAMPLE = np.float32(1e30)                     # samples are bounded by the box and |z| <= 2
S_ACTIVE = 9                                    # the kernels write 0 or 1
S_F64 = -5e300                                  # mean, var, prev_sol
S_IDX = -7                                      # idx, count
S_OBS = np.float32(-3e30)
S_ACTION = np.float32(3e30)
POISON = 1e300                                  # rows of an INPUT nothing may read
GUARD = 256                                     # guard elements behind every buffer


def padded_pop(pop):
    """rrl_cem_update: pop rounded up to a power of two."""
    p = 1
    while p < pop:
        p <<= 1
    return p


def grid_for(n):
    """rrl_host.hpp: grid_for(n) workgroups of kBlock lanes."""
    return max(1, min(K_MAX_GRID, -(-n // K_BLOCK)))


def _stable_seed(key):
    """A seed from names and numbers that does not depend on the interpreter's string hashing."""
    s = 2166136261
    for k in key:
        for b in (k if isinstance(k, str) else repr(int(k))).encode():
            s = ((s ^ b) * 16777619) & 0xFFFFFFFF
    return s


def bounds(kind, dim):
    d = np.arange(dim, dtype=np.float64)
    if kind == "unit":
        return -np.ones(dim), np.ones(dim)
    if kind == "varied":                        # differs in every dimension: a wrong index into lb / ub changes the clamp
        return -1.0 - 0.1 * d, 0.5 + 0.05 * d
    if kind == "maze":                          # the maze's action box
        return np.full(dim, -0.1), np.full(dim, 0.1)
    raise KeyError(kind)


BOUNDS = ("unit", "varied", "maze")

# ---- sample cases -------------------------------------------------------------------------------------------------------------
# setup: how mean, var and the incoming `active` are made (sample_inputs()).  counter: the host's field; tick: the device tick's
# start (None: no counter_dev); inc: counter_inc; live: m_dev[0] (None: no m_dev, the launch bound M counts).
SampleCase = collections.namedtuple("SampleCase", "name M pop dim bounds setup sticky counter tick inc live what",
                                    defaults=("generic", 0, 4, None, 0, None, ""))

SHAPE_MEANS = (4, 50, 10)                       # mean / variance cases: four problems in the box that differs per dimension
SHAPE_FLAGS = (4, 20, 10)                       # activity and sticky cases
SHAPE_COUNT = (5, 400, 10)                      # counter cases: 79 workgroups take a ticket


def _sample_cases():
    S, out = SampleCase, []
    out += [
        S("prod-3x400x10", 3, 400, 10, "unit", what="the production shape of the navigation envs"),
        S("maze-3x400x30", 3, 400, 30, "maze", what="the production shape of the maze, its +-0.1 box"),
        S("pop1", 5, 1, 10, "varied", what="pop = 1: a problem is one row"),
        S("pop1024", 2, 1024, 3, "unit", what="pop at its limit"),
        S("dim1", 7, 33, 1, "varied", what="dim = 1: the max over the variances is the variance"),
        S("dim64", 3, 17, 64, "varied", what="dim at its limit; lb[d], ub[d] differ over 64 dimensions"),
        S("stride-140x400x10", 140, 400, 10, "maze", counter=1, tick=3, inc=1,
          what="560 000 elements: 2048 x 256 lanes walk the grid-stride loop, 2048 workgroups take a ticket"),
        S("manyM-5000x3x2", 5000, 3, 2, "varied", what="several thousand problems of a few elements: 42 problems per workgroup"),
    ]
    M, pop, dim = SHAPE_MEANS
    for mean, var, what in (
            ("interior", "below", "variance below the clamp: the variance is used"),
            ("interior", "at", "variance exactly the clamp"),
            ("interior", "above", "variance above the clamp: the squared half-distance is used"),
            ("on_ub", "above", "means exactly on ub: clamp 0, every sample there is float32(mean)"),
            ("on_lb", "above", "means exactly on lb: clamp 0, every sample there is float32(mean)"),
            ("outside", "above", "means outside the box: the squared half-distance still clamps"),
            ("outside", "below", "means outside the box, variance below that clamp")):
        out.append(S("mean-%s-var-%s" % (mean, var), M, pop, dim, "varied", "mean:%s:%s" % (mean, var), what=what))
    M, pop, dim = SHAPE_FLAGS
    out += [
        S("act-eps", M, pop, dim, "unit", "act:eps", what="max(var) == epsilon: inactive, the test is strict"),
        S("act-next", M, pop, dim, "unit", "act:next", what="max(var) == nextafter(epsilon, inf): active"),
        S("act-lastdim", M, pop, dim, "unit", "act:lastdim", what="only the last dimension above epsilon: active"),
        S("sticky-1", M, pop, dim, "unit", "sticky", sticky=1,
          what="sticky: active 0 on entry and a large variance stays 0, active 1 and a tiny variance becomes 0"),
        S("sticky-0", M, pop, dim, "unit", "sticky", sticky=0, what="the same inputs without sticky: the first problem re-activates"),
    ]
    M, pop, dim = SHAPE_COUNT
    out += [
        S("count-host", M, pop, dim, "unit", counter=11, what="the host's counter alone"),
        S("count-tick", M, pop, dim, "unit", counter=0, tick=11, inc=1, what="the device tick alone"),
        S("count-both-inc1", M, pop, dim, "unit", counter=4, tick=7, inc=1, what="host counter + device tick, counter_inc = 1"),
        S("count-both-inc3", M, pop, dim, "unit", counter=4, tick=7, inc=3, what="host counter + device tick, counter_inc = 3"),
        S("count-inc0", M, pop, dim, "unit", counter=4, tick=7, inc=0, what="counter_inc = 0 reads the tick and leaves it"),
        S("count-tick-2p40", M, pop, dim, "unit", counter=1, tick=2 ** 40, inc=1, what="a tick that needs more than 32 bits"),
        S("mdev-0", M, pop, dim, "unit", sticky=1, counter=0, tick=7, inc=1, live=0,
          what="an empty device-counted set: nothing written, the tick stays"),
        S("mdev-2of5", M, pop, dim, "unit", sticky=1, counter=1, tick=7, inc=3, live=2,
          what="m_dev < M: rows past it keep their sentinels"),
        S("mdev-5of5", M, pop, dim, "unit", sticky=1, counter=0, tick=7, inc=1, live=5, what="m_dev == M, the production flags"),
    ]
    return out


SAMPLE_CASES = _sample_cases()
SAMPLE_BY_NAME = {c.name: c for c in SAMPLE_CASES}
assert len(SAMPLE_BY_NAME) == len(SAMPLE_CASES)


def clamp_of(mean, lb, ub):
    """optimizers.py:95-98 without the variance: min(((mean - lb) / 2)^2, ((ub - mean) / 2)^2)."""
    lo, hi = (mean - lb) / 2.0, (ub - mean) / 2.0
    return np.minimum(lo * lo, hi * hi)


@functools.lru_cache(maxsize=None)
def sample_inputs(name):
    """dict(mean, var [M, dim] f64, lb, ub [dim] f64, active_in [M] u8, expect_active: None or the list the case is about).
    Computed once, shared, never modified."""
    c = SAMPLE_BY_NAME[name]
    # seeded by what the inputs depend on, not by the name: cases that differ in flags or counters alone share their inputs
    rng = np.random.RandomState(_stable_seed(("sample", c.setup, c.bounds, c.M, c.pop, c.dim)))
    M, dim = c.M, c.dim
    lb, ub = bounds(c.bounds, dim)
    w = ub - lb
    mean = lb + w * (0.05 + 0.9 * rng.rand(M, dim))
    var = rng.rand(M, dim) * (w * w) / 8.0 + 1e-6
    # a non-sticky launch does not read `active`: the sentinel proves that every live problem's flag is written
    active_in = np.full(M, S_ACTIVE if not c.sticky else 1, np.uint8)
    expect = None
    kind = c.setup.split(":")
    if kind[0] == "generic":
        var[2::5] = 1e-5                        # problems 2, 7, ...: inactive
    elif kind[0] == "mean":
        if kind[1] == "on_ub":
            mean[:, ::2] = ub[::2]
            mean[0] = ub
        elif kind[1] == "on_lb":
            mean[:, ::2] = lb[::2]
            mean[0] = lb
        elif kind[1] == "outside":
            mean[:, ::2] = ub[::2] + 0.3
            mean[:, 1::4] = lb[1::4] - 0.2
        cl = clamp_of(mean, lb, ub)
        var = dict(below=0.5 * cl, at=cl.copy(), above=2.0 * cl + 0.01)[kind[2]]
        expect = [1] * M
    elif kind[0] == "act":
        var[:] = 1e-5
        var[1] = 0.2
        if kind[1] == "eps":
            var[0] = EPSILON
            expect = [0, 1, 0, 0]
        elif kind[1] == "next":
            var[0] = EPSILON
            var[0, 3] = np.nextafter(EPSILON, np.inf)
            expect = [1, 1, 0, 0]
        else:
            var[0, dim - 1] = 0.01
            var[2, 0] = 0.01
            expect = [1, 1, 1, 0]
    elif kind[0] == "sticky":
        var[:] = 0.2
        var[1], var[3] = 1e-5, 1e-5
        active_in = np.array([0, 1, 7, 0], np.uint8)
        expect = [0, 0, 1, 0] if c.sticky else [1, 0, 1, 0]
    else:
        raise KeyError(c.setup)
    out = dict(mean=mean, var=var, lb=lb, ub=ub, active_in=active_in, expect_active=expect)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def oracle_counter(case):
    """The counter the kernel draws with: the host's field plus the device tick."""
    return case.counter + (case.tick or 0)


def tick_after(case):
    """The device tick after the launch: an empty device-counted set leaves it."""
    if case.tick is None:
        return None
    return case.tick + (0 if case.live == 0 else case.inc)


def live_of(case):
    return case.M if case.live is None else case.live


@functools.lru_cache(maxsize=None)
def sample_oracle(name):
    """The C oracle on the live problems of a table case -> (samples [live, pop, dim] f32 with zeros where a problem is
    inactive, active [live] u8).  Computed once, shared, never modified."""
    from oracle import c_oracle as co
    c, x = SAMPLE_BY_NAME[name], sample_inputs(name)
    n = live_of(c)
    if n == 0:
        return np.zeros((0, c.pop, c.dim), np.float32), np.zeros(0, np.uint8)
    s, a = co.cem_sample(x["mean"][:n], x["var"][:n], x["lb"], x["ub"], c.pop, epsilon=EPSILON, sticky=bool(c.sticky),
                         active=x["active_in"][:n], seed=SEED, counter=oracle_counter(c))
    s.setflags(write=False)
    a.setflags(write=False)
    return s, a


# ---- update cases -------------------------------------------------------------------------------------------------------------
# ne: "one", "tenth" (pop // 10 floored at 1) or "all".  The launch holds M + 2 problems: problem M is inactive, problem M + 1
# lies past the device count; both carry real samples and costs and must keep their mean and variance.
UpdateCase = collections.namedtuple("UpdateCase", "name M pop dim ne alpha costs what")
COST_PATTERNS = ("random", "ascending", "descending", "equal", "all_nan", "nan_1e6", "inf_plus", "inf_minus", "signed_zero",
                 "denormal", "dup_min")
UPDATE_POPS = (1, 2, 3, 63, 64, 65, 255, 256, 257, 400, 1023, 1024)
UPDATE_DIMS = (1, 10, 63, 64)
UPDATE_ALPHAS = (0.0, 0.1, 1.0)


def num_elites_of(case):
    return dict(one=1, tenth=max(1, case.pop // 10), all=case.pop)[case.ne]


def _update_cases():
    U = UpdateCase
    rows = [
        (1, 1, 10, "all", 0.1, "random", "pop = 1: no sort step runs, the one sample is the elite"),
        (3, 2, 1, "all", 0.0, "descending", "pop = 2, one compare-exchange; alpha = 0: the elites alone"),
        (3, 2, 10, "one", 1.0, "dup_min", "alpha = 1: mean and variance keep their values exactly"),
        (3, 3, 10, "all", 0.1, "inf_plus", "pop = 3 padded to 4: one padding key behind real +inf costs, every key an elite"),
        (2, 3, 63, "one", 0.1, "equal", "all costs equal: the elite is index 0; 63 lanes accumulate"),
        (2, 63, 64, "all", 0.1, "inf_plus", "pop = 63 padded to 64; 64 lanes accumulate"),
        (2, 63, 10, "tenth", 0.1, "random", "pop below a wave"),
        (2, 64, 10, "all", 0.1, "ascending", "pop = 64: no padding, already sorted"),
        (2, 64, 1, "tenth", 0.1, "signed_zero", "-0.0 and +0.0 compare equal: the index decides"),
        (3000, 65, 10, "tenth", 0.1, "random", "three thousand workgroups"),
        (2, 65, 10, "all", 0.0, "all_nan", "pop = 65 padded to 128; every cost NaN -> 1e6, index order"),
        (2, 255, 10, "all", 0.1, "nan_1e6", "pop = 255 padded to 256: one lane per key, one padding key"),
        (2, 255, 10, "one", 0.1, "inf_minus", "-inf costs sort first, by index"),
        (2, 256, 10, "tenth", 0.1, "dup_min", "pop = kBlock: one key per lane; the minimum twice, at a low and a high index"),
        (2, 256, 10, "all", 1.0, "descending", "pop = kBlock reversed, every key an elite"),
        (2, 257, 10, "all", 0.1, "inf_plus", "pop = 257 padded to 512: two keys per lane, 255 padding keys behind real +inf"),
        (2, 257, 63, "tenth", 0.1, "inf_minus", "pop just above kBlock"),
        (3, 400, 10, "tenth", 0.1, "random", "the production shape: 40 elites of 400"),
        (1, 400, 10, "all", 0.1, "denormal", "denormal costs must not be flushed to equal zeros; pop = 400 padded to 512"),
        (2, 400, 10, "tenth", 0.1, "equal", "all costs equal: the elites are indices 0 .. 39"),
        (2, 400, 10, "tenth", 0.1, "nan_1e6", "NaN -> 1e6 ties with costs of exactly 1e6f among the elites"),
        (2, 1023, 10, "all", 0.1, "signed_zero", "pop = 1023 padded to 1024: one padding key"),
        (2, 1023, 10, "tenth", 0.1, "inf_plus", "pop = 1023, +inf costs outside the elites"),
        (1, 1024, 64, "all", 0.1, "random", "pop and dim at their limits, 1024 elites"),
        (2, 1024, 10, "one", 0.0, "descending", "pop = 1024 reversed, one elite: the last index"),
        (2, 1024, 10, "tenth", 0.1, "all_nan", "pop = 1024, every cost NaN: the elites are indices 0 .. 101"),
    ]
    return [U("M%d-pop%d-dim%d-%s-a%g-%s" % r[:6], *r) for r in rows]


UPDATE_CASES = _update_cases()
UPDATE_BY_NAME = {c.name: c for c in UPDATE_CASES}
assert len(UPDATE_BY_NAME) == len(UPDATE_CASES)


def dup_low(pop):
    """The low index of the duplicated minimum of `dup_min` (the high one is pop - 1)."""
    return 1 if pop > 2 else 0


def costs_of(pattern, rng, pop):
    """One problem's costs [pop] f32."""
    f32 = np.float32
    c = rng.randn(pop).astype(f32)
    if pattern == "random":
        pass
    elif pattern == "ascending":
        c = np.arange(pop, dtype=f32)
    elif pattern == "descending":
        c = np.arange(pop, dtype=f32)[::-1].copy()
    elif pattern == "equal":
        c[:] = f32(0.25)
    elif pattern == "all_nan":
        c[:] = np.nan
    elif pattern == "nan_1e6":                  # a third NaN, a third exactly 1e6f, the rest dearer: the elites are the ties
        c = (f32(2e6) + np.abs(c) * f32(1e5)).astype(f32)
        kind = rng.randint(0, 3, pop)
        c[kind == 0] = np.nan
        c[kind == 1] = NAN_COST
        c[pop - 1] = np.nan
        c[0] = NAN_COST
    elif pattern == "inf_plus":                 # several +inf, the first and the last index among them
        c[rng.rand(pop) < 0.2] = np.inf
        c[0] = c[pop - 1] = np.inf
    elif pattern == "inf_minus":
        c[rng.rand(pop) < 0.1] = -np.inf
        c[pop - 1] = -np.inf
        c[pop // 2] = -np.inf
    elif pattern == "signed_zero":              # zeros of both signs are the cheapest costs
        c = (np.abs(c) + f32(1.0)).astype(f32)
        zero = rng.rand(pop) < 0.5
        c[zero] = np.where(rng.rand(int(zero.sum())) < 0.5, f32(-0.0), f32(0.0))
        c[pop - 1], c[0] = f32(-0.0), f32(0.0)
    elif pattern == "denormal":                 # bit patterns 1 .. 40 of either sign: denormals with many ties
        bits = rng.randint(1, 41, pop).astype(np.uint32) | (rng.randint(0, 2, pop).astype(np.uint32) << np.uint32(31))
        c = bits.view(f32).copy()
    elif pattern == "dup_min":                  # one duplicated minimum at a low and a high index
        c[dup_low(pop)] = c[pop - 1] = f32(c.min() - f32(1.0))
    else:
        raise KeyError(pattern)
    return c.astype(f32)


@functools.lru_cache(maxsize=None)
def update_inputs(name):
    """dict(samples [M + 2, pop, dim] f32, costs [M + 2, pop] f32, mean, var [M + 2, dim] f64, active [M + 2] u8 with problem M
    inactive).  Computed once, shared, never modified."""
    c = UPDATE_BY_NAME[name]
    rng = np.random.RandomState(_stable_seed(("update", name)))
    Mt = c.M + 2
    samples = rng.uniform(-1.0, 1.0, (Mt, c.pop, c.dim)).astype(np.float32)
    costs = np.stack([costs_of(c.costs, rng, c.pop) for _ in range(Mt)])
    mean = rng.uniform(-0.9, 0.9, (Mt, c.dim))
    var = rng.uniform(0.01, 0.3, (Mt, c.dim))
    active = np.ones(Mt, np.uint8)
    active[c.M] = 0
    out = dict(samples=samples, costs=costs, mean=mean, var=var, active=active)
    for v in out.values():
        v.setflags(write=False)
    return out


def restate_update(samples, costs, mean, var, num_elites, alpha, active=None):
    """optimizers.py:104-117 of the reference for every problem m with active[m] != 0, in float64 -> (mean, var) copies."""
    samples = np.asarray(samples, np.float32)
    M, pop, dim = samples.shape
    c = np.array(costs, np.float32)
    c[c != c] = NAN_COST                                          # MPC.py:415
    mean, var = np.array(mean, np.float64), np.array(var, np.float64)
    index, ne = np.arange(pop), int(num_elites)
    assert 0 < ne <= pop
    for m in range(M):
        if active is not None and not active[m]:
            continue
        order = np.lexsort((index, c[m]))[:ne]                    # by (cost, index)
        x = samples[m][order].astype(np.float64)                  # the elites [ne, dim], cheapest first
        s = np.zeros(dim)
        for e in range(ne):
            s = s + x[e]
        em = s / float(ne)
        sq = np.zeros(dim)
        for e in range(ne):
            dv = x[e] - em
            sq = sq + dv * dv
        ev = sq / float(ne)
        mean[m] = alpha * mean[m] + (1.0 - alpha) * em
        var[m] = alpha * var[m] + (1.0 - alpha) * ev
    return mean, var


@functools.lru_cache(maxsize=None)
def update_reference(name):
    """restate_update() of a table case over its M + 2 problems: computed once, shared, never modified."""
    c, x = UPDATE_BY_NAME[name], update_inputs(name)
    m, v = restate_update(x["samples"], x["costs"], x["mean"], x["var"], num_elites_of(c), c.alpha, x["active"])
    m.setflags(write=False)
    v.setflags(write=False)
    return m, v


# ---- begin and finish cases ---------------------------------------------------------------------------------------------------
SetCase = collections.namedtuple("SetCase", "name n dim du mask what")
MASK_PATTERNS = ("zeros", "ones", "alternating", "first_last", "last", "random30", "none_first_1024", "wave_gap", "bytes")
SET_NS = (1, 63, 64, 65, 1023, 1024, 1025, 2048, 2049, 4173)
SET_DIMS = ((10, 2), (1, 1), (64, 64), (7, 3), (64, 2))


def _set_cases():
    rows = [
        (1, 10, 2, "ones", "one env that plans"),
        (1, 1, 1, "zeros", "one env that does not; dim = du = 1"),
        (63, 7, 3, "alternating", "below a wave; du does not divide dim"),
        (64, 64, 64, "ones", "one full wave; du == dim: the shifted solution is all zeros"),
        (65, 10, 2, "random30", "one row into the second wave"),
        (1023, 10, 2, "first_last", "one short of the workgroup: the last lane idles"),
        (1024, 7, 3, "last", "exactly one pass, the set row in its last lane"),
        (1025, 10, 2, "last", "the second pass holds one row, the only set one: base_sh carries 0"),
        (1025, 10, 2, "zeros", "two passes, nothing set: finish writes zeros and leaves prev_sol"),
        (2048, 64, 2, "random30", "two full passes, base_sh carries the first pass's count"),
        (2049, 10, 2, "none_first_1024", "nothing set in the first pass"),
        (2049, 1, 1, "ones", "three passes, the first two full of set rows"),
        (4173, 10, 2, "wave_gap", "five passes; a whole wave of zeros between set rows"),
        (4173, 7, 3, "bytes", "set bytes of 2, 0x80 and 255"),
        (4173, 64, 64, "alternating", "du == dim over five passes"),
        (8200, 64, 2, "random30", "n * dim = 524 800: cem_finish_kernel walks its grid-stride loop"),
    ]
    return [SetCase("n%d-dim%d-du%d-%s" % r[:4], *r) for r in rows]


SET_CASES = _set_cases()
SET_BY_NAME = {c.name: c for c in SET_CASES}
assert len(SET_BY_NAME) == len(SET_CASES)


def mask_of(pattern, n, rng):
    m = np.zeros(n, np.uint8)
    if pattern == "zeros":
        pass
    elif pattern == "ones":
        m[:] = 1
    elif pattern == "alternating":
        m[::2] = 1
    elif pattern == "first_last":
        m[0] = m[n - 1] = 1
    elif pattern == "last":
        m[n - 1] = 1
    elif pattern == "random30":
        m[rng.rand(n) < 0.3] = 1
    elif pattern == "none_first_1024":
        m[K_BEGIN_BLOCK:] = rng.rand(n - K_BEGIN_BLOCK) < 0.5
        m[n - 1] = 1
    elif pattern == "wave_gap":                 # wave 0 set, wave 1 all zeros, wave 2 on: every third row
        m[:WAVE] = 1
        m[2 * WAVE::3] = 1
    elif pattern == "bytes":
        on = np.flatnonzero(rng.rand(n) < 0.5)
        m[on] = np.array([2, 0x80, 255, 1], np.uint8)[np.arange(on.size) % 4]
    else:
        raise KeyError(pattern)
    return m


@functools.lru_cache(maxsize=None)
def set_inputs(name):
    """dict(mask [n] u8, prev_sol [n, dim] f64, init_var [dim] f64, obs [n, 2] f32, mean [n, dim] f64: what the planner is taken
    to have left between begin and finish -- random rows for the problems, POISON behind them).  Shared, never modified."""
    c = SET_BY_NAME[name]
    rng = np.random.RandomState(_stable_seed(("set", name)))
    mask = mask_of(c.mask, c.n, rng)
    count = int((mask != 0).sum())
    mean = np.full((c.n, c.dim), POISON)
    mean[:count] = rng.uniform(-1.0, 1.0, (count, c.dim))
    out = dict(mask=mask, prev_sol=rng.uniform(-1.0, 1.0, (c.n, c.dim)), init_var=rng.uniform(0.1, 0.3, c.dim),
               obs=rng.randn(c.n, 2).astype(np.float32), mean=mean)
    for v in out.values():
        v.setflags(write=False)
    return out


def begin_buffers(n, dim):
    """The sentinel-filled outputs of rrl_cem_begin for n envs, on the host."""
    return dict(idx=np.full(n, S_IDX, np.int32), count=np.full(1, S_IDX, np.int32), mean=np.full((n, dim), S_F64),
                var=np.full((n, dim), S_F64), cur_obs=np.full((n, 2), S_OBS, np.float32), active=np.full(n, S_ACTIVE, np.uint8))


def restate_begin(mask, prev_sol, init_var, obs, out=None):
    """The host-count path of MPC.act up to the optimiser: idx = mask.nonzero(), the warm starts, the initial variance, the
    observations of the planning envs, all active.  -> copies of the whole buffers `out` (default: begin_buffers()) with the
    first `count` rows written."""
    mask, prev_sol, obs = np.asarray(mask), np.asarray(prev_sol, np.float64), np.asarray(obs, np.float32)
    n, dim = prev_sol.shape
    out = {k: v.copy() for k, v in (begin_buffers(n, dim) if out is None else out).items()}
    idx = np.flatnonzero(mask != 0)
    count = idx.size
    out["count"][0] = count
    out["idx"][:count] = idx
    for j in range(count):
        out["mean"][j] = prev_sol[idx[j]]
        out["var"][j] = init_var
        out["cur_obs"][j] = obs[idx[j]]
        out["active"][j] = 1
    return out


def restate_finish(mask, idx, count, mean, prev_sol, action, du):
    """The host-count path of MPC.act behind the optimiser on copies of the whole buffers -> (action, prev_sol):
    action[i] = float32(mean[j, :du]) for the planning env i = idx[j] and 0 for every other env,
    prev_sol[i] = concat(mean[j, du:], zeros(du)); every other env's row stays."""
    mask, mean = np.asarray(mask), np.asarray(mean, np.float64)
    action, prev_sol = np.array(action, np.float32), np.array(prev_sol, np.float64)
    dim = prev_sol.shape[1]
    action[mask == 0] = 0.0
    for j in range(int(count)):
        i = int(idx[j])
        action[i] = mean[j, :du].astype(np.float32)
        prev_sol[i] = np.concatenate([mean[j, du:], np.zeros(du)])
        assert prev_sol[i].shape == (dim,)
    return action, prev_sol


@functools.lru_cache(maxsize=None)
def set_reference(name):
    """dict(begin: restate_begin()'s buffers, action, prev_sol: restate_finish() on the case's `mean`) of a table case."""
    c, x = SET_BY_NAME[name], set_inputs(name)
    b = restate_begin(x["mask"], x["prev_sol"], x["init_var"], x["obs"])
    action, prev_sol = restate_finish(x["mask"], b["idx"], b["count"][0], x["mean"], x["prev_sol"],
                                      np.full((c.n, c.du), S_ACTION, np.float32), c.du)
    return dict(begin=b, action=action, prev_sol=prev_sol)


# ---- the production chain and the captured round ------------------------------------------------------------------------------
# (n, how the mask is made): pop = 400, dim = 10, du = 2
CHAIN = dict(pop=400, dim=10, du=2, num_elites=40, rounds=5, t0=12, cases=((65, "random30"), (1100, "spread")))
CAPTURE = dict(n=1100, pop=64, dim=10, du=2, num_elites=6, alpha=0.1, t0=5, replays=2)


def chain_mask(n, kind):
    rng = np.random.RandomState(_stable_seed(("chain", n, kind)))
    if kind == "random30":
        return mask_of("random30", n, rng)
    m = np.zeros(n, np.uint8)                   # "spread": set rows in both 1024-row passes
    m[5:K_BEGIN_BLOCK:40] = 1
    m[K_BEGIN_BLOCK - 1] = m[K_BEGIN_BLOCK] = 1
    m[K_BEGIN_BLOCK + 3::7] = 1
    return m


def quadratic_costs(samples, target):
    """The chain's fixed cost: |sample - target|^2 in float32, summed over the dimensions in index order -> [M, pop] f32."""
    diff = (np.asarray(samples, np.float32) - np.asarray(target, np.float32)[:, None, :]).astype(np.float32)
    sq = (diff * diff).astype(np.float32)
    out = np.zeros(sq.shape[:2], np.float32)
    for d in range(sq.shape[2]):
        out = (out + sq[:, :, d]).astype(np.float32)
    return out


# ---- device side (used by the GPU tests only) ---------------------------------------------------------------------------------
class Buf:
    """A device buffer holding `host` with `guard` elements of `fill` behind it."""

    def __init__(self, host, fill, dev, guard=GUARD):
        import torch
        host = np.ascontiguousarray(host)
        self.shape, self.n, self.fill = host.shape, host.size, fill
        self.flat = torch.empty(host.size + guard, dtype=torch.from_numpy(np.zeros(1, host.dtype)).dtype, device=dev)
        self.flat[:self.n] = torch.from_numpy(host.reshape(-1).copy()).to(dev)
        self.flat[self.n:] = torch.from_numpy(np.array([fill], host.dtype)).to(dev)

    @property
    def t(self):
        return self.flat[:self.n].view(self.shape)

    def host(self):
        return self.flat[:self.n].view(self.shape).cpu().numpy()

    def tail_intact(self):
        tail = self.flat[self.n:].cpu().numpy()
        return bool((tail == np.array(self.fill, tail.dtype)).all())

    def data_ptr(self):
        return self.flat.data_ptr()


def describe(struct, **fields):
    """A descriptor with the given fields set (a Buf or a tensor: its address); what is not given stays NULL / 0."""
    d = struct()
    for k, v in fields.items():
        if v is not None:
            setattr(d, k, v.data_ptr() if hasattr(v, "data_ptr") else v)
    return d


def _lib():
    from recovery_rl_amd import _lib as L
    return L, L.load(), L.current_stream()


def _sync():
    import torch
    torch.cuda.synchronize()


def run_sample(name, dev):
    """rrl_cem_sample on table case `name` -> dict(samples, active, mean, var, lb, ub (host arrays of the whole buffers),
    active_in: what `active` held before, tick: None or [tick, ticket], tails: every guard intact)."""
    import torch
    L, lib, st = _lib()
    c, x = SAMPLE_BY_NAME[name], sample_inputs(name)
    mean, var = Buf(x["mean"], S_F64, dev), Buf(x["var"], S_F64, dev)
    lb, ub = Buf(x["lb"], S_F64, dev), Buf(x["ub"], S_F64, dev)
    active_in = x["active_in"].copy()
    if c.live is not None:
        active_in[c.live:] = S_ACTIVE                               # past the device count nothing may write
    active = Buf(active_in, S_ACTIVE, dev)
    samples = Buf(np.full((c.M, c.pop, c.dim), S_SAMPLE, np.float32), S_SAMPLE, dev, guard=GUARD + c.pop * c.dim)
    m_dev = None if c.live is None else torch.tensor([c.live], dtype=torch.int32, device=dev)
    tick = None if c.tick is None else torch.tensor([c.tick, 0], dtype=torch.int64, device=dev)
    d = describe(L.rrl_cem_t, M=c.M, m_dev=m_dev, pop=c.pop, dim=c.dim, mean=mean, var=var, lb=lb, ub=ub, epsilon=EPSILON,
                 sticky=c.sticky, active=active, seed=SEED, counter=c.counter, counter_dev=tick, counter_inc=c.inc, samples=samples)
    rc = lib.rrl_cem_sample(d, st)
    assert rc == 0, rc
    _sync()
    bufs = (mean, var, lb, ub, active, samples)
    return dict(samples=samples.host(), active=active.host(), mean=mean.host(), var=var.host(), lb=lb.host(), ub=ub.host(),
                active_in=active_in, tick=None if tick is None else tick.tolist(), tails=all(b.tail_intact() for b in bufs))


def run_update(name, dev, device_count):
    """rrl_cem_update on table case `name` over its M + 2 problems.  device_count: m_dev[0] = M + 1 of a launch bound of M + 2
    (problem M + 1 lies past the count); else the bound is M + 1 and problem M + 1 is not part of the launch.
    -> dict(mean, var [M + 2, dim], tails)."""
    import torch
    L, lib, st = _lib()
    c, x = UPDATE_BY_NAME[name], update_inputs(name)
    extra = padded_pop(c.pop) - c.pop
    rows = np.full((extra, c.dim), S_SAMPLE, np.float32)           # behind the last problem: whatever a padding key reads
    samples = Buf(np.concatenate([x["samples"].reshape(-1, c.dim), rows]), S_SAMPLE, dev)
    costs = Buf(x["costs"], np.float32(S_SAMPLE), dev)
    mean, var, active = Buf(x["mean"], S_F64, dev), Buf(x["var"], S_F64, dev), Buf(x["active"], S_ACTIVE, dev)
    m_dev = torch.tensor([c.M + 1], dtype=torch.int32, device=dev) if device_count else None
    d = describe(L.rrl_cem_t, M=c.M + 2 if device_count else c.M + 1, m_dev=m_dev, pop=c.pop, dim=c.dim, mean=mean, var=var,
                 active=active, samples=samples, costs=costs, num_elites=num_elites_of(c), alpha=c.alpha)
    rc = lib.rrl_cem_update(d, st)
    assert rc == 0, rc
    _sync()
    unchanged = np.array_equal(samples.host()[:x["samples"].size // c.dim].reshape(x["samples"].shape), x["samples"]) and \
        costs.host().tobytes() == x["costs"].tobytes() and np.array_equal(active.host(), x["active"])
    return dict(mean=mean.host(), var=var.host(), inputs_unchanged=unchanged,
                tails=all(b.tail_intact() for b in (samples, costs, mean, var, active)))


def set_buffers(name, dev):
    """The device buffers of a begin / finish case: inputs and sentinel-filled outputs -> dict of Buf."""
    c, x = SET_BY_NAME[name], set_inputs(name)
    b = {k: Buf(v, dict(idx=S_IDX, count=S_IDX, mean=S_F64, var=S_F64, cur_obs=S_OBS, active=S_ACTIVE)[k], dev)
         for k, v in begin_buffers(c.n, c.dim).items()}
    b.update(mask=Buf(x["mask"], 0, dev), prev_sol=Buf(x["prev_sol"], S_F64, dev), init_var=Buf(x["init_var"], S_F64, dev),
             obs=Buf(x["obs"], S_OBS, dev), action=Buf(np.full((c.n, c.du), S_ACTION, np.float32), S_ACTION, dev))
    return b


def set_desc(c, b):
    L = _lib()[0]
    return describe(L.rrl_cem_set_t, n=c.n, dim=c.dim, du=c.du, **b)


def run_begin(name, dev):
    """rrl_cem_begin on table case `name` -> dict(the six outputs and prev_sol, obs, mask, init_var as host arrays, tails)."""
    L, lib, st = _lib()
    c = SET_BY_NAME[name]
    b = set_buffers(name, dev)
    rc = lib.rrl_cem_begin(set_desc(c, b), st)
    assert rc == 0, rc
    _sync()
    out = {k: v.host() for k, v in b.items()}
    out["tails"] = all(v.tail_intact() for v in b.values())
    return out


def run_finish(name, dev):
    """rrl_cem_finish on table case `name` with idx and count from the restatement and the case's own `mean` (values begin did
    not produce) -> dict(action, prev_sol, the inputs as host arrays, tails)."""
    L, lib, st = _lib()
    c, x, ref = SET_BY_NAME[name], set_inputs(name), set_reference(name)
    b = set_buffers(name, dev)
    b["idx"] = Buf(ref["begin"]["idx"], S_IDX, dev)
    b["count"] = Buf(ref["begin"]["count"], S_IDX, dev)
    b["mean"] = Buf(x["mean"], S_F64, dev)
    rc = lib.rrl_cem_finish(set_desc(c, b), st)
    assert rc == 0, rc
    _sync()
    out = {k: v.host() for k, v in b.items()}
    out["tails"] = all(v.tail_intact() for v in b.values())
    return out
