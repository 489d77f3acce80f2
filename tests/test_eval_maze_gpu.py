"""rrl_eval_rollout_maze on the device, over the case table of eval_maze_cases.py (which test_eval_maze_cpu.py proves fair), in
the manner of test_eval_rollout_gpu.py.

Env: a second MazeVecEnv at the same seed, tick and horizon, driven by the traced executed actions, agrees with the trace bit
for bit (state, reward, flags; rows the horizon ended included), the tick advances by T + reset, and the per-env results are
the fold of the trace.  Networks: against float64 at the traced states, at the bounds the Navigation test uses for this
kernel, the gate against q64 > eps_safe outside the 1e-5 band.  Then determinism, independence of the trace, and the packed
launch against the solo ones.
Closest approaches to the bounds seen on an MI355X over the case table (each test prints its own): task action 1.4e-8 against
a bound of 1.2e-5, z 5.9e-7 against 5.9e-5, recovery action 1.9e-8 against 7.7e-6; no (row, step) pair inside the band."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import eval_cases as EC
import eval_maze_cases as MC
from recovery_rl_amd import _lib
from recovery_rl_amd.env.maze import MazeVecEnv
from test_eval_rollout_gpu import DEV, GUARD, RESULTS, TRACES, guarded, same_bits, views

pytestmark = pytest.mark.gpu
EINVAL = -1
NETS = ("pW1", "pb1", "pW2p", "pb2", "pW3", "pb3", "scale", "bias")
GROUPS = ("qW1", "qb1", "qW2p", "qb2", "qW3", "qb3", "rW1", "rb1", "rW2p", "rb2", "rW3", "rb3", "rscale", "rbias", "rlog_std")


@functools.lru_cache(maxsize=None)
def dev_weights():
    """The Maze agent's weights on the device by descriptor field, W2 in fragment order (rrl_w2_pack)."""
    lib, out = _lib.load(), {}
    for k, v in MC.weights32().items():
        t = torch.tensor(v, device=DEV).contiguous()
        if k.endswith("W2"):
            packed = torch.empty(t.numel(), dtype=torch.float32, device=DEV)
            _lib.check(lib.rrl_w2_pack(t.shape[0], t.shape[1], t.data_ptr(), packed.data_ptr(), _lib.current_stream()), "w2_pack")
            out[k + "p"] = packed
        else:
            out[k] = t
    return out


class Launch:
    """Buffers, descriptor and horizon of one Maze rollout: every output longer than needed, filled with its guard value."""

    def __init__(self, n, T, horizon, recovery, reset, eps_safe=None, pos=None, tick=MC.TICK, seed=MC.SEED):
        self.n, self.T, self.horizon, self.recovery, self.reset, self.seed, self.tick0 = n, T, horizon, recovery, reset, seed, tick
        w = dev_weights()
        self.buf = {k: guarded(dt, n) for k, dt in RESULTS.items()}
        self.buf.update({k: guarded(dt, T * n * width) for k, (dt, width) in TRACES.items()})
        self.tick = torch.tensor([tick, 0], dtype=torch.int64, device=DEV)
        if pos is None and not reset:
            pos = MC.start_states(n)
        self.pos = None if pos is None else torch.tensor(np.asarray(pos), dtype=torch.float64, device=DEV).contiguous()
        p = _lib.ptr
        a = _lib.rrl_eval_rollout_t(n=n, T=T, H=256, d_obs=2, d_act=2, env_kind=_lib.ENV_MAZE, reset=reset, pos=p(self.pos),
                                    seed=seed, counter=0, counter_dev=p(self.tick), **{k: p(w[k]) for k in NETS},
                                    **{k: p(t) for k, t in self.buf.items()})
        if recovery:
            for k in GROUPS:
                setattr(a, k, p(w[k]))
            a.eps_safe = MC.eps_safe(n, reset) if eps_safe is None else eps_safe
            a.min_log_std = MC.MIN_LOG_STD
        self.args = a

    def run(self):
        _lib.check(_lib.load().rrl_eval_rollout_maze(C.byref(self.args), self.horizon, _lib.current_stream()),
                   "rrl_eval_rollout_maze")
        return self.read()

    def read(self):
        out = {k: t.cpu().numpy() for k, t in self.buf.items()}
        out["tick"] = self.tick.cpu().tolist()
        return out


def packed_call(launches):
    args = (_lib.rrl_eval_rollout_t * len(launches))(*[l.args for l in launches])
    horizon = (C.c_int * len(launches))(*[l.horizon for l in launches])
    return _lib.load().rrl_eval_rollout_maze_packed(len(launches), args, horizon, _lib.current_stream())


def check_case(n, T, horizon, recovery, reset, out, seed=MC.SEED, tick=MC.TICK, networks=True):
    v = views(out, n, T)
    flags = v["tr_flags"]
    # ---- alive from the trace itself; dead rows' entries untouched ----
    alive = np.ones((T, n), bool)
    for j in range(1, T):
        alive[j] = alive[j - 1] & ((flags[j - 1] >> 1) & 1 == 0)
    assert ((flags[alive] & 1) == 1).all() and (flags[~alive] == GUARD[torch.uint8]).all()
    for k, (dt, width) in TRACES.items():
        written = recovery or k not in ("tr_z", "tr_eps")
        a = np.moveaxis(v[k], 1, 2) if k == "tr_z" else v[k]
        if written:
            assert (a[~alive] == GUARD[dt]).all(), k
            assert np.isfinite(a[alive].astype(np.float64)).all() and (a[alive] != GUARD[dt]).all(), k
        else:
            assert (a == GUARD[dt]).all(), k
    assert out["tick"] == [tick + T + reset, 0]

    # ---- env, exact: a second env at the same seed, tick and horizon, stepped with the traced executed actions ----
    env = MazeVecEnv("maze", n, device=DEV, seed=seed, horizon=horizon, auto_reset=False)
    env.tick[0] = tick
    if reset:
        env.reset()
    else:
        env.pos.copy_(torch.tensor(MC.start_states(n), device=DEV))
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

    # ---- results: the fold of the trace, f32 adds in step order; the env's horizon bounds every row ----
    ret = np.zeros(n, np.float32)
    for j in range(T):
        ret = np.where(alive[j], ret + v["tr_reward"][j], ret).astype(np.float32)
    assert v["ret"].tobytes() == ret.tobytes()
    assert np.array_equal(v["success"], (alive & ((flags >> 3) & 1 == 1)).any(0))
    assert np.array_equal(v["violation"], (alive & ((flags >> 2) & 1 == 1)).any(0))
    assert np.array_equal(v["steps"], alive.sum(0)) and (v["steps"] <= horizon).all()
    # a row that ran `horizon` steps is done at its last one, whatever its flags
    if horizon <= T:
        full = v["steps"] == horizon
        assert ((flags[horizon - 1][full] >> 1) & 1 == 1).all()
    if not networks:
        return v, alive

    # ---- networks, against float64 at the traced states ----
    obs = v["tr_pos"][alive].astype(np.float32)
    task = v["tr_task"][alive]
    eps = v["tr_eps"][alive] if recovery else None
    net = MC.networks64(obs, task=task if recovery else None, eps=eps)
    scale = float(MC.weights32()["scale"].max())
    m = np.abs(net["mean"]).max()
    err = np.abs(task - net["task"]).max()
    print("task action: max err %.3g, bound %.3g (m = %.3g)" % (err, scale * (1e-4 * m + 1e-6), m))
    assert err <= scale * (1e-4 * m + 1e-6)
    rec_bit = ((flags >> 4) & 1 == 1)
    if not recovery:
        assert not rec_bit[alive].any() and v["tr_real"][alive].tobytes() == task.tobytes()
        return v, alive
    z = np.moveaxis(v["tr_z"], 1, 2)[alive].T                                     # [2, pairs]
    zs = np.abs(net["z"]).max()
    zerr = np.abs(z - net["z"]).max()
    print("z: max err %.3g, bound %.3g (scale = %.3g)" % (zerr, 1e-4 * zs + 1e-9, zs))
    assert zerr <= 1e-4 * zs + 1e-9
    want_eps = np.stack([EC.eval_noise(n, tick + reset + j, seed) for j in range(T)])
    assert eps.tobytes() == want_eps[alive].tobytes()
    eps_s = MC.eps_safe(n, reset)
    clear = np.abs(net["q"] - eps_s) > MC.BAND
    print("gate: %d of %d pairs inside the band" % ((~clear).sum(), clear.size))
    assert (~clear).sum() <= 0.02 * clear.size
    gate = rec_bit[alive]
    assert np.array_equal(gate[clear], (net["q"] > eps_s)[clear])
    realv = v["tr_real"][alive]
    assert realv[~gate].tobytes() == task[~gate].tobytes()
    if gate.any():
        rscale = float(MC.weights32()["rscale"].max())
        mr = np.abs(net["mean_r"]).max()
        rerr = np.abs(realv[gate] - net["rec"][gate]).max()
        print("recovery action: max err %.3g, bound %.3g (m = %.3g)" % (rerr, rscale * (1e-4 * mr + 1e-6), mr))
        assert rerr <= rscale * (1e-4 * mr + 1e-6)
    # ... and bit for bit: the recovery action of EVERY row at the traced states of the first and the last step, from a
    # one-step launch whose gate always fires (eps_safe = -1) at that step's tick
    for j in sorted({0, T - 1}):
        one = Launch(n, 1, horizon, True, 0, eps_safe=-1.0, pos=np.where(alive[j][:, None], v["tr_pos"][j], 0.0),
                     tick=tick + reset + j, seed=seed)
        w = views(one.run(), n, 1)
        assert ((w["tr_flags"][0] >> 4) & 1 == 1).all()
        g = alive[j] & rec_bit[j]
        assert v["tr_real"][j][g].tobytes() == w["tr_real"][0][g].tobytes()
        assert v["tr_task"][j][alive[j]].tobytes() == w["tr_task"][0][alive[j]].tobytes()
    return v, alive


@pytest.mark.parametrize("n,T,horizon,recovery,reset", MC.all_cases())
def test_rollout_against_the_eager_env_and_float64(n, T, horizon, recovery, reset):
    out = Launch(n, T, horizon, recovery, reset).run()
    v, alive = check_case(n, T, horizon, recovery, reset, out)
    if horizon < MC.HORIZON and n >= 17:
        # the clause only Maze has: rows the horizon ended, done with neither flag, after exactly `horizon` steps
        last = v["tr_flags"][horizon - 1]
        timeout = alive[horizon - 1] & ((last & 0b1110) == 0b0010)
        assert timeout.any() and (v["steps"][timeout] == horizon).all()
        assert not v["success"][timeout].any() and not v["violation"][timeout].any()
        assert not alive[horizon:].any()
    # determinism: a second launch at the same tick agrees bit for bit
    assert same_bits(out, Launch(n, T, horizon, recovery, reset).run())


def test_outputs_do_not_depend_on_the_trace():
    """The trace is optional, pointer by pointer: without it the per-env results are the same bits."""
    want = Launch(65, 7, 3, True, 0).run()
    for keep in ((), ("tr_pos", "tr_flags"), ("tr_eps",)):
        bare = Launch(65, 7, 3, True, 0)
        for k in TRACES:
            if k not in keep:
                setattr(bare.args, k, None)
        got = bare.run()
        for k in RESULTS:
            assert got[k].tobytes() == want[k].tobytes(), (keep, k)
        for k, (dt, _) in TRACES.items():
            assert got[k].tobytes() == want[k].tobytes() if k in keep else (got[k] == GUARD[dt]).all(), (keep, k)
        assert got["tick"] == want["tick"]


PACKED = [dict(n=65, T=7, horizon=3, recovery=True, reset=0, seed=MC.SEED, tick=MC.TICK),
          dict(n=17, T=2, horizon=100, recovery=False, reset=1, seed=MC.SEED + 11, tick=5),
          dict(n=130, T=101, horizon=40, recovery=True, reset=1, seed=0xABCDEF987, tick=2 ** 33 + 3)]


@pytest.mark.parametrize("S", [2, 3])
def test_packed_launch_is_the_solo_launches(S):
    """S seeds that differ in n, T, horizon, groups, reset, env seed and tick: each seed's outputs and trace equal its solo
    launch bit for bit, and each seed's own tick advances by its own T + reset."""
    cases = PACKED[:S]
    solo = [Launch(**c).run() for c in cases]
    launches = [Launch(**c) for c in cases]
    _lib.check(packed_call(launches), "rrl_eval_rollout_maze_packed")
    for c, a, l in zip(cases, solo, launches):
        b = l.read()
        assert same_bits(a, b), c
        assert b["tick"] == [c["tick"] + c["T"] + c["reset"], 0]
        # every seed ran on ITS seed, tick and horizon: the env part of the case check, at the packed launch's outputs
        check_case(c["n"], c["T"], c["horizon"], c["recovery"], c["reset"], b, seed=c["seed"], tick=c["tick"], networks=False)
    # the horizon is part of the plan: the same descriptors with other horizons are another launch
    again = [Launch(**dict(c, horizon=c["horizon"] + 1)) for c in cases]
    _lib.check(packed_call(again), "rrl_eval_rollout_maze_packed")
    for c, l in zip(cases, again):
        assert same_bits(Launch(**dict(c, horizon=c["horizon"] + 1)).run(), l.read()), c


def test_a_mixed_array_is_refused():
    """One Navigation descriptor among Maze ones: RRL_EINVAL from the Maze entry, a Maze one among Navigation ones from the
    Navigation entry, and nothing was launched (every buffer still holds its guard, no tick moved)."""
    launches = [Launch(**c) for c in PACKED[:2]]
    launches[1].args.env_kind = 0
    assert packed_call(launches) == EINVAL
    args = (_lib.rrl_eval_rollout_t * 2)(*[l.args for l in launches])
    assert _lib.load().rrl_eval_rollout_packed(2, args, _lib.current_stream()) == EINVAL
    torch.cuda.synchronize()
    for l, c in zip(launches, PACKED):
        out = l.read()
        assert out["tick"] == [c["tick"], 0]
        for k, dt in list(RESULTS.items()) + [(k, dt) for k, (dt, _) in TRACES.items()]:
            assert (out[k] == GUARD[dt]).all(), k
