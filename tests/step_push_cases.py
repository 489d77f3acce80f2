"""Cases, inputs and the composite host reference shared by test_step_push_cpu.py and test_step_push_gpu.py.

The fused env step (rrl_nav_step_push_x / rrl_maze_step_push_x, csrc/step_push.hpp) against something that is not itself: one
reference step is put together here from the oracle's parts only -- c_oracle.nav_step / maze_step, two c_oracle.OracleReplay
rings (with `pin`), update_oracle.fixed_order_sum / recovery_select / stoch_head and the episode log of log_oracle (restated
vectorised below, checked against EpisodeLogOracle by the CPU file) -- and nothing from recovery_rl_amd.

Inputs are raw numpy arrays built from a seed: every option of rrl_step_push_t is a field of `Case`, initial_state() gives what
the device buffers hold before the first step, make_inputs() what step k reads, reference_step() advances the host state.
"""
import collections
import math

import numpy as np
import torch

import update_pieces as UP
from oracle import c_oracle as co
from oracle import update_oracle as O

K = 4                                   # steps per case
SMALL, MID = 16384, 262144              # the launch shapes' size limits (step_push.hpp: regime_of)
NEAR = 1e-5                             # no row's float64 risk lies this close to eps_safe
BASE_COUNTER = 1000                     # rrl_step_push_t.counter of the device-tick cases (the tick is added to it)
TICK0, TICK_INC = 7, 2
LOG_ITER0 = 5                           # the episode table's iteration count on entry
STATS0 = np.arange(1, 9, dtype=np.int64) * 11      # the counters are added to, not stored
STALE = 0xF000                          # flag bits the status words carry on entry


def regime_of(n):
    return 0 if n <= SMALL else (1 if n <= MID else 2)


_FIELDS = dict(
    name=None, env="navigation1", n=1,
    layout="arrays",            # "arrays": t + obs read; "status": u16 words, t NULL, stored state = float(pos)
    gate="off",                 # "off": real_action / recovery given; "action": sel_z + sel_rec_action; "head": sel_z + sel_rec_head
    sel_n_part=1, head_n_part=1, head_eps=True, log_std="above",
    ld_task=2, push_real_action=0,
    mem=None,                   # (cap, pinned) of the task ring
    rmem=None,                  # (cap, pinned) of the safety ring, None = recovery_memory NULL
    outputs="all",              # "all" six per-env outputs, "none", or "two" = reward + ep_done only
    log="off",                  # "off", "on", "small" = a table smaller than the episodes that end
    auto_reset=1, horizon=4,
    tick="dev",                 # "dev": counter_dev with counter_inc 2; "host": counter_dev NULL, the caller counts
    reward_penalty=0.0, eps_safe=0.3, seed=1)
Case = collections.namedtuple("Case", list(_FIELDS))


def span(n, pinned=0, free=None):
    """(cap, pinned) of a ring that n rows per step wrap in step 3 (n = 1: 2 free slots; else 2.5 n unless given)."""
    free = free if free is not None else (2 if n == 1 else 2 * n + n // 2)
    return pinned + free, pinned


def case(name, env, n, **kw):
    f = dict(_FIELDS, name=name, env=env, n=n, **kw)
    if f["mem"] is None:
        f["mem"] = span(n)
    f["seed"] = 1 + sum(ord(c) * (i + 1) for i, c in enumerate(name))
    return Case(**f)


# ---- the case table ----------------------------------------------------------------------------------------------------------
# Option values that occur in EVERY regime (0: n <= 16384, 1: n <= 262144, 2: above) and with BOTH env classes (nav, maze);
# test_step_push_cpu.py::test_the_table_covers_every_option_in_every_regime_and_env_class checks exactly this list:
#   layout arrays / status; gate off / action / head; sel_n_part 1 / 3 / 4; head n_part 1 / 4; head eps given / NULL;
#   log_std above / mixed; ld_task 2 / 4; push_real_action 0 / 1; recovery_memory given / NULL; a pinned ring / none;
#   outputs all / none / two; log off / on / small; auto_reset 0 / 1; tick dev / host; reward_penalty 0 / 2.5;
#   eps_safe 0.3 / 0.65.
# sel_n_part = 2 and head n_part = 2 occur in regimes 0 and 1 only (regime 2 has four cases: three of them gated).
# n edges: 1 (one lane), 63 (partial wave), 257 (second, partial workgroup), 16384 (last speculative size), 16385 (first
# 256-thread bandwidth size), 262144 / 262145 (the boundary to 1024 threads).
# Rings: every ring wraps in step 3 (span()).  Safety rings of the bandwidth regimes: "odd" = cap % 1024 != 0 and pinned % 1024
# != 0 (the workgroup that straddles the wrap sends its waves' nets straight to memory), "even" = both multiples of 1024 (the
# workgroup sums stay on): the two branches of block_sums.  The odd rings of r1_all_on and r2_all_on are sized so that the
# workgroup that straddles the wrap really touches three super-chunks (the last two and the one behind the pinned rows): it
# starts more slots before the ring's end than the last super-chunk holds, (free - 2 n) % workgroup size > cap % 1024 > 0.
# Those two cases run without auto-reset: an env inside an obstacle stays there, so step 3 still writes positives into those
# slots (with auto-reset the nav envs are back in the free start zone by then: under 1 % positives).
ALL_ON = dict(layout="status", gate="head", sel_n_part=3, head_n_part=4, ld_task=4, push_real_action=1, log="on",
              reward_penalty=2.5, outputs="none")


def _table():
    c = []
    # -- regime 0 (speculative, 256 threads, ticket) --
    # r0_all_on: everything on at once, nav; pinned safety ring that wraps
    c.append(case("r0_all_on", "navigation1", 16384, **ALL_ON, mem=span(16384, 500), rmem=span(16384, 777)))
    # r0_one_lane: n edge 1; nav x (arrays, gate action, sel 1, ld 2, push 0, rmem given, outputs all, log on, host tick)
    c.append(case("r0_one_lane", "navigation2", 1, gate="action", rmem=span(1, 3), log="on", tick="host", eps_safe=0.65))
    # r0_wave: n edge 63; nav x (gate off, rmem NULL, outputs two, auto_reset 0, log small)
    c.append(case("r0_wave", "navigation1", 63, outputs="two", auto_reset=0, log="small", reward_penalty=2.5))
    # r0_two_groups: n edge 257; nav x (head with eps NULL, sel 4, head n_part 1, log_std mixed, ld 4, eps_safe 0.65)
    c.append(case("r0_two_groups", "navigation2", 257, gate="head", sel_n_part=4, head_n_part=1, head_eps=False,
                  log_std="mixed", ld_task=4, rmem=span(257), eps_safe=0.65, outputs="two", tick="host"))
    # r0_maze_all_on: everything on, maze, n edge 16384
    c.append(case("r0_maze_all_on", "maze", 16384, **ALL_ON, mem=span(16384), rmem=span(16384, 1000)))
    # r0_maze_plain: maze x (arrays, gate off, ld 2, push 0, rmem NULL, outputs all, log off, auto_reset 0, host tick, penalty 0)
    c.append(case("r0_maze_plain", "maze", 1500, auto_reset=0, tick="host"))
    # r0_maze_action: maze x (gate action, sel 1, log small, outputs two, no pinned ring, eps_safe 0.65, status)
    c.append(case("r0_maze_action", "maze", 4097, layout="status", gate="action", sel_n_part=1, rmem=span(4097), log="small",
                  outputs="two", eps_safe=0.65, push_real_action=1))
    # r0_maze_head: maze x (head n_part 1, eps NULL, log_std mixed, sel 4); sel / head n_part 2 in r0_parts2
    c.append(case("r0_maze_head", "maze", 257, gate="head", sel_n_part=4, head_n_part=1, head_eps=False, log_std="mixed",
                  rmem=span(257, 100), eps_safe=0.65, ld_task=4))
    # r0_parts2: sel_n_part 2 and head n_part 2 (regime 0, nav) x (status, log on, no pinned ring, penalty 2.5)
    c.append(case("r0_parts2", "navigation1", 1500, gate="head", sel_n_part=2, head_n_part=2, rmem=span(1500), log="on",
                  layout="status", reward_penalty=2.5))
    # -- regime 1 (256 threads + the cursor launch) --
    # r1_all_on: everything on, nav, n edge 16385; odd pinned safety ring
    c.append(case("r1_all_on", "navigation2", 16385, **ALL_ON, mem=span(16385, 300), rmem=span(16385, 100, 41984), auto_reset=0))
    # r1_edge_hi: n edge 262144; nav x (gate action, sel 1, even safety ring, log small, outputs two, host tick, eps_safe 0.65)
    c.append(case("r1_edge_hi", "navigation1", 262144, gate="action", rmem=span(262144, 2048, 640 * 1024), log="small",
                  outputs="two", tick="host", eps_safe=0.65))
    # r1_plain: nav x (gate off, rmem NULL, outputs all, log off, auto_reset 0)
    c.append(case("r1_plain", "navigation1", 20000, auto_reset=0))
    # r1_head_noeps: nav x (head eps NULL, head n_part 1, sel 4, mixed, ld 4); status with horizon 4095
    c.append(case("r1_head_noeps", "navigation2", 40000, layout="status", gate="head", sel_n_part=4, head_n_part=1,
                  head_eps=False, log_std="mixed", ld_task=4, rmem=span(40000), horizon=4095, eps_safe=0.65, outputs="all"))
    # r1_maze_all_on: everything on, maze; even pinned safety ring (1024, 40 * 1024 free)
    c.append(case("r1_maze_all_on", "maze", 16385, **ALL_ON, mem=span(16385), rmem=span(16385, 1024, 40 * 1024)))
    # r1_maze_plain: maze x (gate off, rmem NULL, log off, auto_reset 0, host tick, outputs all)
    c.append(case("r1_maze_plain", "maze", 70001, auto_reset=0, tick="host"))
    # r1_maze_action: maze x (gate action, log small, outputs two, odd safety ring without pinned rows)
    c.append(case("r1_maze_action", "maze", 20000, gate="action", rmem=span(20000), log="small", outputs="two",
                  eps_safe=0.65, layout="status"))
    # r1_maze_head: maze x (head n_part 1, eps NULL, mixed, sel 4)
    c.append(case("r1_maze_head", "maze", 40000, gate="head", sel_n_part=4, head_n_part=1, head_eps=False, log_std="mixed",
                  rmem=span(40000, 333), eps_safe=0.65))
    # r1_parts2: sel_n_part 2 and head n_part 2 (regime 1, nav) x (arrays, ld 4, push 1, log on, pinned odd safety ring)
    c.append(case("r1_parts2", "navigation1", 70001, gate="head", sel_n_part=2, head_n_part=2, rmem=span(70001, 5), log="on",
                  push_real_action=1, ld_task=4))
    # -- regime 2 (1024 threads + the cursor launch): four cases --
    # r2_all_on: everything on, nav, n edge 262145; odd pinned safety ring
    c.append(case("r2_all_on", "navigation1", 262145, **ALL_ON, mem=span(262145, 300), rmem=span(262145, 1500, 656208), auto_reset=0))
    # r2_maze_plain: maze x regime 2 x (arrays, gate off, ld 2, push 0, rmem NULL, outputs all, log off, auto_reset 0, host tick)
    c.append(case("r2_maze_plain", "maze", 262145, auto_reset=0, tick="host"))
    # r2_action: nav x (gate action, sel 1, push 1, even pinned safety ring, outputs two, log small, eps_safe 0.65)
    c.append(case("r2_action", "navigation2", 300001, gate="action", sel_n_part=1, push_real_action=1,
                  rmem=span(300001, 2048, 733 * 1024), outputs="two", log="small", eps_safe=0.65))
    # r2_maze_head: maze x (status, head n_part 1, eps NULL, mixed, sel 4, ld 4, log on, outputs all, odd ring, no pinned rows)
    c.append(case("r2_maze_head", "maze", 270001, layout="status", gate="head", sel_n_part=4, head_n_part=1, head_eps=False,
                  log_std="mixed", ld_task=4, rmem=span(270001), log="on", eps_safe=0.65, reward_penalty=2.5))
    return c


CASES = _table()
assert len(set(c.name for c in CASES)) == len(CASES)

# the all-options-off case of test_nav_gpu.py::test_fused_step_push_matches_oracle_step_plus_pushes (n = 1500, cap = 4000,
# horizon 100, penalty 2.5, both rings): the composite reference must reproduce that test's inline computation
PLAIN = case("plain", "navigation1", 1500, mem=(4000, 0), rmem=(4000, 0), horizon=100, reward_penalty=2.5)


def packed_seeds(env_class, regime):
    """The S = 3 seeds of one packed launch: different n inside one regime, each with its own option set -- one gated from
    the head, one with the log on and status words, one plain with a pinned ring."""
    ns = (1, 257, 16384) if regime == 0 else (16385, 20000, 70001)
    env = ("maze",) * 3 if env_class == "maze" else ("navigation1",) * 3      # one env kind per packed call
    tag = "pk%d_%s_" % (regime, env_class)
    return [
        case(tag + "head", env[0], ns[0], gate="head", sel_n_part=3, head_n_part=4, ld_task=4, rmem=span(ns[0]),
             outputs="two", reward_penalty=2.5),
        case(tag + "log", env[1], ns[1], layout="status", log="on", rmem=span(ns[1]), outputs="none"),
        case(tag + "pinned", env[2], ns[2], mem=span(ns[2], 100), rmem=span(ns[2], 1029), push_real_action=1, eps_safe=0.65),
    ]


# ---- inputs ----------------------------------------------------------------------------------------------------------------
def is_maze(c):
    return c.env == "maze"


def act_scale(c):
    return 0.1 if is_maze(c) else 1.0


def head_consts(c):
    """scale, bias, log_std [2] f32 and min_log_std of the recovery policy's head: update_pieces' box (different per action
    dim), for the maze as well -- its step clips the action to +-0.1 like any other."""
    f = lambda x: np.asarray(x, np.float32)
    return f(UP.SCALE), f(UP.BIAS), f(UP.stoch_log_stds()[c.log_std]), UP.MIN_LOG_STD


def count_table_len(cap):
    """RRL_POS_CNT_LEN(cap) (include/rrl_hip.h): per-64-slot counts, padded to 4, per-1024-slot counts, padded to 2, one
    64-bit mask per chunk."""
    n_chunks, n_super = (cap + 63) // 64, (cap + 1023) // 1024
    return ((n_chunks + 3) // 4 * 4 + n_super + 1) // 2 * 2 + 2 * n_chunks


def count_tables(r, size, cap):
    """The three regions for a ring whose first `size` rows are filled: what the device table holds on entry."""
    n_chunks, n_super = (cap + 63) // 64, (cap + 1023) // 1024
    pos = np.zeros(n_super * 1024, bool)
    pos[:size] = r[:size] != 0
    out = np.zeros(count_table_len(cap), np.int32)
    out[:n_chunks] = pos[:n_chunks * 64].reshape(-1, 64).sum(1)
    base = (n_chunks + 3) // 4 * 4
    out[base:base + n_super] = pos.reshape(-1, 1024).sum(1)
    mbase = (base + n_super + 1) // 2 * 2
    out[mbase:] = np.packbits(pos[:n_chunks * 64].reshape(-1, 64), axis=1, bitorder="little").view(np.int32).ravel()
    return out


def _ring_rows(rng, rows, constraint):
    s, a, s2 = (rng.randn(rows, 2).astype(np.float32) for _ in range(3))
    r = (rng.uniform(size=rows) < 0.4).astype(np.float32) if constraint else rng.randn(rows).astype(np.float32)
    return s, a, r, s2, rng.randint(0, 2, rows).astype(np.float32)


def initial_state(c):
    """What the per-env arrays, the accumulators and the pinned ring rows hold before step 1 (numpy)."""
    n = c.n
    rng = np.random.RandomState(c.seed)
    st = {}
    if is_maze(c):
        pos, _, _ = co.maze_reset(n, seed=c.seed, counter=3)
        i = np.arange(n)
        wall = i % 5 == 1                         # next to the wall at x = -0.1 (contact from x >= -0.13), some inside it
        pos[wall, 0] = rng.uniform(-0.15, -0.128, n)[wall]
        pos[wall, 1] = (rng.uniform(0.14, 0.27, n) * rng.choice([-1.0, 1.0], n))[wall]
        goal = i % 5 == 3                         # around the goal (0.25, 0)
        pos[goal] = np.c_[rng.uniform(0.2, 0.27, n), rng.uniform(-0.04, 0.04, n)][goal]
    else:
        pos = np.c_[rng.uniform(-60, 10, n), rng.uniform(-12, 12, n)]
    st["pos"] = np.ascontiguousarray(pos, np.float64)
    if c.horizon == 4:
        t = rng.randint(0, 4, n)
    else:                                         # horizon 4095: a share of the envs reaches it in each of the K steps
        t = np.where(rng.uniform(size=n) < 0.4, c.horizon - 1 - rng.randint(0, K, n), rng.randint(0, 4000, n))
    st["t"] = t.astype(np.int32)
    # arrays layout: the observation is NOT float(pos) on entry -- the stored state must come from it there and from pos in
    # the status layout
    st["obs"] = rng.uniform(100.0, 200.0, (n, 2)).astype(np.float32)
    st["ep_reward"] = rng.uniform(-5.0, 5.0, n).astype(np.float32)
    st["log_len"] = rng.randint(0, 50, n).astype(np.int32)
    st["log_ret"] = rng.uniform(-100.0, 0.0, n)
    st["log_viol"] = rng.randint(0, 3, n).astype(np.int32)
    st["log_rec"] = rng.randint(0, 3, n).astype(np.int32)
    st["mem_rows"] = _ring_rows(rng, c.mem[1], False)
    st["rmem_rows"] = _ring_rows(rng, c.rmem[1], True) if c.rmem else None
    return st


BIG = np.float32(2.0 ** 27)      # a partial that absorbs every other one: BIG + x == BIG in f32 for |x| < 8


def _split(rng, target, n_part, order_rows=None, axis=0):
    """f32 partials [n_part, ...] of the float64 `target`: random ones, and the last makes up the difference.  In the rows
    `order_rows` (a mask over `axis` of the target; n_part >= 3) the first two partials are +BIG and -BIG: added in the
    documented order ((p0 + p1) + p2) + ... they cancel exactly and the sum is the target's; added in an order that puts a
    small partial next to one of them first, the small one is absorbed and the sum is not."""
    parts = [(rng.randn(*target.shape) * 0.7).astype(np.float32) for _ in range(n_part - 1)]
    if order_rows is not None and n_part >= 3:
        sel = (slice(None),) * axis + (order_rows,)
        parts[0][sel], parts[1][sel] = BIG, -BIG
    parts.append((target - sum(p.astype(np.float64) for p in parts)).astype(np.float32))
    return np.stack(parts)


def summed(parts):
    """The documented f32 sum of f32 partials [n_part, ...] (update_oracle.fixed_order_sum) as numpy."""
    return O.fixed_order_sum(torch.from_numpy(np.ascontiguousarray(parts))).numpy()


def risk64(parts):
    """float64 risk max sigmoid of the summed partials [n_part, 2, n]."""
    return O.risk(torch.from_numpy(summed(parts))).numpy()


def make_inputs(c, k):
    """What step k (0-based) reads: task [n,4] (the action in columns 2..3 when ld_task = 4, in 0..1 of a [n,2] view
    otherwise), real / recovery (gate off; with the gate on they hold values nobody may read), z partials, the recovery
    action or the head's partials and noise."""
    n, A = c.n, act_scale(c)
    rng = np.random.RandomState((c.seed * 7919 + k) % (2 ** 31))
    inp = {}
    task = rng.uniform(-A, A, (n, 4)).astype(np.float32)
    task[:, 0:2] += np.float32(50.0)                  # columns 0..1 of an ld_task = 4 row: somebody else's data
    inp["task4"] = task
    inp["task"] = np.ascontiguousarray(task[:, 2:4])
    inp["real"] = rng.uniform(-1.3 * A, 1.3 * A, (n, 2)).astype(np.float32)
    inp["recovery"] = (rng.uniform(size=n) < 0.3).astype(np.uint8)
    if c.gate == "off":
        return inp
    inp["recovery"][:] = 1                            # ignored with the gate on
    eps_safe = float(np.float32(c.eps_safe))

    def draw_z(m, first):
        z = rng.uniform(-4.0, 4.0, (2, m))
        b = first + np.arange(m)
        edge = b % 97 == 60                           # update_pieces.select_rows: risk exactly 0 or 1 in f32
        z[:, edge] = np.where((b // 97) % 2 == 0, 100.0, -100.0)[edge]
        return _split(rng, np.float32(z).astype(np.float64), c.sel_n_part, b % 97 == 30, axis=1)

    zp = draw_z(n, 0)
    for _ in range(100):                              # rows within NEAR of the threshold are drawn again
        near = np.nonzero(np.abs(risk64(zp) - eps_safe) < NEAR)[0]
        if not len(near):
            break
        zp[:, :, near] = draw_z(len(near), 1)         # (a handful of rows)
    inp["z_parts"] = zp
    if c.gate == "action":
        inp["rec"] = rng.uniform(-1.3 * A, 1.3 * A, (n, 2)).astype(np.float32)
        return inp
    b = np.arange(n)                                  # update_pieces.stoch_rows: saturated tanh and eps = 0 rows
    raw = rng.randn(n, 2) * 1.5
    raw[b % 6 == 4] = (np.where((b // 6) % 2 == 0, 1.0, -1.0)[:, None] * 25.0)[b % 6 == 4]
    eps = rng.randn(n, 2)
    eps[b % 6 == 5] = 0.0
    inp["head_parts"] = _split(rng, np.float32(raw).astype(np.float64), c.head_n_part, b % 97 == 30)
    inp["head_eps"] = eps.astype(np.float32)          # built either way; the case says whether the kernel gets it
    return inp


def head_action64(c, inp):
    """update_oracle.stoch_head in float64 on the summed f32 partials -> [n,2] float64 tensor."""
    scale, bias, log_std, floor = head_consts(c)
    t = torch.from_numpy
    return O.stoch_head(t(summed(inp["head_parts"])), t(inp["head_eps"]) if c.head_eps else None, t(log_std), floor,
                        t(scale), t(bias))[0]


# ---- the episode log, vectorised -----------------------------------------------------------------------------------------------
class VecLog:
    """log_oracle.EpisodeLogOracle over arrays: the same accumulators, the records of one step in env order."""

    def __init__(self, n, length=None, ret=None, viol=None, rec=None, iteration=0):
        z = lambda x, dt: np.zeros(n, dt) if x is None else np.array(x, dt)
        self.len, self.ret, self.viol, self.rec = z(length, np.int32), z(ret, np.float64), z(viol, np.int32), z(rec, np.int32)
        self.iteration = iteration
        self.rec_i32, self.rec_f64 = np.zeros((0, 6), np.int32), np.zeros((0, 2), np.float64)
        self.per_step = []                      # finished episodes of each step

    def append(self, reward, constraint, success, ep_done, recovery=None):
        r = np.asarray(reward, np.float32).astype(np.float64)
        c = (np.asarray(constraint) != 0).astype(np.int32)
        rc = np.zeros_like(c) if recovery is None else (np.asarray(recovery) != 0).astype(np.int32)
        self.len += 1
        self.ret = self.ret + r
        self.viol += c
        self.rec += rc
        e = np.nonzero(np.asarray(ep_done) != 0)[0]
        flags = (np.asarray(success)[e] != 0).astype(np.int32) | (c[e] << 1) | (rc[e] << 2)
        i32 = np.stack([e.astype(np.int32), np.full(len(e), self.iteration, np.int32), self.len[e], self.viol[e], self.rec[e],
                        flags], 1)
        self.rec_i32 = np.concatenate([self.rec_i32, i32])
        self.rec_f64 = np.concatenate([self.rec_f64, np.stack([self.ret[e], r[e]], 1)])
        self.per_step.append(len(e))
        self.len[e], self.ret[e], self.viol[e], self.rec[e] = 0, 0.0, 0, 0
        self.iteration += 1

    def records(self):
        return [tuple(int(x) for x in a) + (float(b[0]), float(b[1])) for a, b in zip(self.rec_i32, self.rec_f64)]


def log_cap(c):
    """Table size: room for every episode that can end ("on"), or a third of the envs ("small": with horizon 4 nearly every
    env ends an episode within the K steps, so the table overflows; the CPU file checks that it does)."""
    return K * c.n + 3 if c.log == "on" else max(1, c.n // 3)


# ---- the composite reference -------------------------------------------------------------------------------------------------
def ring_slots(cap, pinned, pos, n):
    """Slots of n consecutive pushes from cursor `pos` (replay_device.hpp: past the last slot the ring continues at `pinned`)."""
    s = pos + np.arange(n, dtype=np.int64)
    return np.where(s < cap, s, s - cap + pinned)


def _oracle_ring(spec, rows):
    cap, pinned = spec
    ring = co.OracleReplay(cap)
    for arr in (ring.s, ring.a, ring.r, ring.s2, ring.m):
        arr[...] = RING_FILL                    # rows nobody has written yet: recognisable, on the device as well
    if pinned:
        ring.push(*rows)
        ring.pin()
    return ring


RING_FILL = np.float32(-3.0)


def reference_state(c, init):
    ref = dict(pos=init["pos"].copy(), t=init["t"].copy(), obs=init["obs"].copy(), ep_reward=init["ep_reward"].copy(),
               stats=STATS0.copy(), tick=TICK0, step=0, terms=([], []), mem=_oracle_ring(c.mem, init["mem_rows"]),
               rmem=_oracle_ring(c.rmem, init["rmem_rows"]) if c.rmem else None, log=None, wraps={"mem": [], "rmem": []},
               positives_overwritten=0, events=collections.Counter())
    if c.layout == "status":
        ref["status"] = (init["t"].astype(np.uint16) | np.uint16(STALE)).astype(np.uint16)
    if c.log != "off":
        ref["log"] = VecLog(c.n, init["log_len"], init["log_ret"], init["log_viol"], init["log_rec"], LOG_ITER0)
    return ref


def reference_step(c, ref, inp):
    """One fused step on the host, from the oracle's parts.  `inp` is make_inputs(c, k), for gate = "head" with inp["rec"] set
    by the caller (the f32 recovery action the gate chooses from).  Advances `ref`, returns the step's per-env values."""
    n, k = c.n, ref["step"]
    task = inp["task"]
    # 1.-3. the gate
    if c.gate == "off":
        act, flag, risk = inp["real"], inp["recovery"] != 0, None
    else:
        z = torch.from_numpy(summed(inp["z_parts"]))
        real, fl, _, q = O.recovery_select(z, float(np.float32(c.eps_safe)), torch.from_numpy(task), torch.from_numpy(inp["rec"]))
        flag, risk = fl.numpy(), q.numpy()
        act = np.where(flag[:, None], inp["rec"], task).astype(np.float32)
        assert np.array_equal(act, real.numpy().astype(np.float32))
    # 4. the env step
    counter = BASE_COUNTER + ref["tick"] if c.tick == "dev" else BASE_COUNTER + 3 * k
    t_in = (ref["status"] & 0xFFF).astype(np.int32) if c.layout == "status" else ref["t"]
    if is_maze(c):
        o = co.maze_step(ref["pos"], act, t_in, seed=c.seed, counter=counter, horizon=c.horizon, auto_reset=bool(c.auto_reset))
    else:
        o = co.nav_step(c.env, ref["pos"], act, t_in, seed=c.seed, counter=counter, horizon=c.horizon,
                        auto_reset=bool(c.auto_reset))
    cons, dn, succ, epd = (o[key] != 0 for key in ("constraint", "done", "success", "ep_done"))
    rew = o["reward"]
    # 5. the replay rows
    prev = ref["pos"].astype(np.float32) if c.layout == "status" else ref["obs"]
    mask = np.where(dn, np.float32(0.0), np.float32(1.0))
    prew = np.where(cons, rew - np.float32(c.reward_penalty), rew).astype(np.float32)
    for key, spec, rows in (("mem", c.mem, (prev, act if c.push_real_action else task, prew, o["next_obs"], mask)),
                            ("rmem", c.rmem, (prev, act, cons.astype(np.float32), o["next_obs"], mask))):
        ring = ref[key]
        if ring is None:
            continue
        slots = ring_slots(spec[0], spec[1], ring.pos, n)
        if key == "rmem":
            old = slots < ring.size
            ref["positives_overwritten"] += int((ring.r[slots[old]] != 0).sum())
        if ring.pos + n >= spec[0]:
            ref["wraps"][key].append(k + 1)
        ring.push(*rows)
        assert ring.pos == int(ring_slots(spec[0], spec[1], slots[0], n + 1)[-1])
    # 6. the counters
    ref["stats"] += np.array([n, epd.sum(), (epd & cons).sum(), (epd & cons & flag).sum(), (epd & cons & ~flag).sum(),
                              (epd & succ).sum(), flag.sum(), cons.sum()], np.int64)
    # 7. the running return: one f32 add per env and step; the two f64 sums as their terms (math.fsum adds them exactly)
    er = ref["ep_reward"] + rew
    assert er.dtype == np.float32
    ref["terms"][0].append(rew.astype(np.float64))
    ref["terms"][1].append(er[epd].astype(np.float64))
    ref["ep_reward"] = np.where(epd, np.float32(0.0), er)
    # 8. env state and status words
    reset = epd & bool(c.auto_reset)
    ref["pos"], ref["t"], ref["obs"] = o["pos"], o["t"], o["obs"]
    if c.layout == "status":
        ref["status"] = (o["t"].astype(np.uint16) | (dn.astype(np.uint16) << 12) | (cons.astype(np.uint16) << 13) |
                         (succ.astype(np.uint16) << 14) | (epd.astype(np.uint16) << 15)).astype(np.uint16)
    # 9. the log
    if ref["log"] is not None:
        ref["log"].append(rew, cons, succ, epd, flag)
    if c.tick == "dev":
        ref["tick"] += TICK_INC
    ref["step"] = k + 1
    ev = ref["events"]
    ev["constraint"] += int(cons.sum())
    ev["done"] += int(dn.sum())
    ev["horizon"] += int((t_in + 1 == c.horizon).sum())
    ev["reset"] += int(reset.sum())
    ev["success"] += int(succ.sum())
    ev["flag"] += int(flag.sum())
    return dict(o, act=act, flag=flag.astype(np.uint8), risk=risk, prev=prev, counter=counter, at_horizon=t_in + 1 == c.horizon)


def reward_sums(ref):
    """(exact sums of the terms so far, the bound of an f64 sum of them in any order): the kernel adds its terms with f64
    atomics in arrival order, workgroup sums first.  A sum of N terms in any order is off by at most (N - 1) 2^-53 sum |term|;
    the device sums run over the steps, so N = n * (steps so far)."""
    out = []
    for terms in ref["terms"]:
        flat = np.concatenate(terms) if terms else np.zeros(0)
        n_terms = ref["step"] * len(ref["pos"])
        out.append((math.fsum(flat.tolist()), (n_terms - 1) * 2.0 ** -53 * math.fsum(np.abs(flat).tolist())))
    return out


def run_reference(c, steps=K):
    """The reference alone for `steps` steps (gate = "head": the recovery action is the float64 head rounded to f32).
    -> (ref, per-step outputs, per-step inputs)"""
    ref = reference_state(c, initial_state(c))
    outs, inps = [], []
    for k in range(steps):
        inp = make_inputs(c, k)
        if c.gate == "head":
            inp["rec"] = head_action64(c, inp).numpy().astype(np.float32)
        outs.append(reference_step(c, ref, inp))
        inps.append(inp)
    return ref, outs, inps
