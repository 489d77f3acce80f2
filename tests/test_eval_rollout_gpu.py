"""rrl_eval_rollout on the device, over the case table of eval_cases.py (which test_eval_rollout_cpu.py proves fair).

Env: a second NavigationVecEnv at the same seed and tick, driven by the traced executed actions, agrees with the trace bit for
bit (state, reward, flags), the tick advances by T + reset, and the per-env results are the fold of the trace.  Networks:
against float64 at the traced states, at the project's bar (1e-4 relative to the case's largest magnitude),
the gate against q64 > eps_safe outside the 1e-5 band.  Then determinism, and the packed launch against the solo ones.
Largest errors seen on an MI355X over the case table (each test prints its own): task action 5.7e-7 against a bound of
1.6e-4, z 3.2e-6 against 1.4e-4, recovery action 4.8e-7 against 1.6e-4."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import eval_cases as EC
from recovery_rl_amd import _lib
from recovery_rl_amd.env.navigation import ENV_KIND, NavigationVecEnv

pytestmark = pytest.mark.gpu
DEV = "cuda"
PAD = 33                                  # guard elements behind every buffer
GUARD = {torch.float32: -7777.0, torch.float64: -7777.0, torch.uint8: 0xAB, torch.int32: -77}
TRACES = {"tr_pos": (torch.float64, 2), "tr_task": (torch.float32, 2), "tr_real": (torch.float32, 2), "tr_z": (torch.float32, 2),
          "tr_eps": (torch.float32, 2), "tr_reward": (torch.float32, 1), "tr_flags": (torch.uint8, 1)}
RESULTS = {"ret": torch.float32, "success": torch.uint8, "violation": torch.uint8, "steps": torch.int32}


@functools.lru_cache(maxsize=None)
def dev_weights(kind):
    """The kind's weights on the device by descriptor field, W2 in fragment order (rrl_w2_pack)."""
    lib, w = _lib.load(), EC.weights32(kind)
    out = {}
    for k, v in w.items():
        t = torch.tensor(v, device=DEV).contiguous()
        if k.endswith("W2"):
            packed = torch.empty(t.numel(), dtype=torch.float32, device=DEV)
            _lib.check(lib.rrl_w2_pack(t.shape[0], t.shape[1], t.data_ptr(), packed.data_ptr(), _lib.current_stream()), "w2_pack")
            out[k + "p"] = packed
        else:
            out[k] = t
    return out


def guarded(dtype, count):
    return torch.full((count + PAD,), GUARD[dtype], dtype=dtype, device=DEV)


class Launch:
    """Buffers and descriptor of one rollout: every output longer than needed, filled with its guard value."""

    def __init__(self, kind, n, T, recovery, reset, eps_safe=None, pos=None, tick=EC.TICK, counter=0):
        self.kind, self.n, self.T, self.recovery, self.reset = kind, n, T, recovery, reset
        w = dev_weights(kind)
        self.buf = {k: guarded(dt, n) for k, dt in RESULTS.items()}
        self.buf.update({k: guarded(dt, T * n * width) for k, (dt, width) in TRACES.items()})
        self.tick = torch.tensor([tick, 0], dtype=torch.int64, device=DEV)
        if pos is None and not reset:
            pos = EC.start_states(kind, n)
        self.pos = None if pos is None else torch.tensor(np.asarray(pos), dtype=torch.float64, device=DEV).contiguous()
        p = _lib.ptr
        a = _lib.rrl_eval_rollout_t(n=n, T=T, H=256, d_obs=2, d_act=2, env_kind=ENV_KIND[kind], reset=reset, pos=p(self.pos),
                                    seed=EC.SEED, counter=counter, counter_dev=p(self.tick),
                                    **{k: p(w[k]) for k in ("pW1", "pb1", "pW2p", "pb2", "pW3", "pb3", "scale", "bias")},
                                    **{k: p(t) for k, t in self.buf.items()})
        if recovery:
            for k in ("qW1", "qb1", "qW2p", "qb2", "qW3", "qb3", "rW1", "rb1", "rW2p", "rb2", "rW3", "rb3", "rscale", "rbias",
                      "rlog_std"):
                setattr(a, k, p(w[k]))
            a.eps_safe = EC.eps_safe(kind, n, reset) if eps_safe is None else eps_safe
            a.min_log_std = EC.MIN_LOG_STD
        self.args = a

    def run(self):
        _lib.check(_lib.load().rrl_eval_rollout(C.byref(self.args), _lib.current_stream()), "rrl_eval_rollout")
        return self.read()

    def read(self):
        out = {k: t.cpu().numpy() for k, t in self.buf.items()}
        out["tick"] = self.tick.cpu().tolist()
        return out


def launch_packed(launches):
    args = (_lib.rrl_eval_rollout_t * len(launches))(*[l.args for l in launches])
    _lib.check(_lib.load().rrl_eval_rollout_packed(len(launches), args, _lib.current_stream()), "rrl_eval_rollout_packed")
    return [l.read() for l in launches]


def same_bits(a, b):
    return all(a[k].tobytes() == b[k].tobytes() for k in list(RESULTS) + list(TRACES)) and a["tick"] == b["tick"]


def views(out, n, T):
    """The used part of every buffer in its shape; asserts the guards behind it."""
    v = {}
    for k, dt in RESULTS.items():
        assert (out[k][n:] == GUARD[dt]).all(), k
        v[k] = out[k][:n]
    for k, (dt, width) in TRACES.items():
        assert (out[k][T * n * width:] == GUARD[dt]).all(), k
        body = out[k][:T * n * width]
        v[k] = body.reshape(T, 2, n) if k == "tr_z" else body.reshape((T, n, 2) if width == 2 else (T, n))
    return v


def check_case(kind, n, T, recovery, reset, out):
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
    assert out["tick"] == [EC.TICK + T + reset, 0]

    # ---- env, exact: a second env at the same seed and tick, stepped with the traced executed actions ----
    env = NavigationVecEnv(kind, n, device=DEV, seed=EC.SEED, auto_reset=False)
    env.tick[0] = EC.TICK
    if reset:
        env.reset()
    else:
        env.pos.copy_(torch.tensor(EC.start_states(kind, n), device=DEV))
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

    # ---- networks, against float64 at the traced states ----
    obs = v["tr_pos"][alive].astype(np.float32)
    task = v["tr_task"][alive]
    eps = v["tr_eps"][alive] if recovery else None
    net = EC.networks64(kind, obs, task=task if recovery else None, eps=eps)
    scale = float(EC.weights32(kind)["scale"].max())
    m = np.abs(net["mean"]).max()
    err = np.abs(task - net["task"]).max()
    print("task action: max err %.3g, bound %.3g (m = %.3g)" % (err, scale * (1e-4 * m + 1e-6), m))
    assert err <= scale * (1e-4 * m + 1e-6)
    rec_bit = ((flags >> 4) & 1 == 1)
    if not recovery:
        assert not rec_bit[alive].any() and v["tr_real"][alive].tobytes() == task.tobytes()
        return
    z = np.moveaxis(v["tr_z"], 1, 2)[alive].T                                     # [2, pairs]
    zs = np.abs(net["z"]).max()
    zerr = np.abs(z - net["z"]).max()
    print("z: max err %.3g, bound %.3g (scale = %.3g)" % (zerr, 1e-4 * zs + 1e-9, zs))
    assert zerr <= 1e-4 * zs + 1e-9
    want_eps = np.stack([EC.eval_noise(n, EC.TICK + reset + j) for j in range(T)])
    assert eps.tobytes() == want_eps[alive].tobytes()
    eps_s = EC.eps_safe(kind, n, reset)
    clear = np.abs(net["q"] - eps_s) > EC.BAND
    assert (~clear).sum() <= 0.02 * clear.size
    gate = rec_bit[alive]
    assert np.array_equal(gate[clear], (net["q"] > eps_s)[clear])
    realv = v["tr_real"][alive]
    assert realv[~gate].tobytes() == task[~gate].tobytes()
    if gate.any():
        rscale = float(EC.weights32(kind)["rscale"].max())
        mr = np.abs(net["mean_r"]).max()
        rerr = np.abs(realv[gate] - net["rec"][gate]).max()
        print("recovery action: max err %.3g, bound %.3g (m = %.3g)" % (rerr, rscale * (1e-4 * mr + 1e-6), mr))
        assert rerr <= rscale * (1e-4 * mr + 1e-6)
    # ... and bit for bit: the recovery action of EVERY row at the traced states of the first and the last step, from a
    # one-step launch whose gate always fires (eps_safe = -1) at that step's tick
    for j in sorted({0, T - 1}):
        one = Launch(kind, n, 1, True, 0, eps_safe=-1.0, pos=np.where(alive[j][:, None], v["tr_pos"][j], 0.0),
                     tick=EC.TICK + reset + j)
        w = views(one.run(), n, 1)
        assert ((w["tr_flags"][0] >> 4) & 1 == 1).all()
        g = alive[j] & rec_bit[j]
        assert v["tr_real"][j][g].tobytes() == w["tr_real"][0][g].tobytes()
        assert v["tr_task"][j][alive[j]].tobytes() == w["tr_task"][0][alive[j]].tobytes()


@pytest.mark.parametrize("kind,n,T,recovery,reset", EC.all_cases())
def test_rollout_against_the_eager_env_and_float64(kind, n, T, recovery, reset):
    out = Launch(kind, n, T, recovery, reset).run()
    check_case(kind, n, T, recovery, reset, out)
    # determinism: a second launch at the same tick agrees bit for bit
    assert same_bits(out, Launch(kind, n, T, recovery, reset).run())


def test_outputs_do_not_depend_on_the_trace():
    """The trace is optional, pointer by pointer: without it the per-env results are the same bits."""
    full = Launch("navigation1", 65, 7, True, 0)
    want = full.run()
    bare = Launch("navigation1", 65, 7, True, 0)
    for k in TRACES:
        setattr(bare.args, k, None)
    got = bare.run()
    for k in RESULTS:
        assert got[k].tobytes() == want[k].tobytes()
    for k, (dt, _) in TRACES.items():
        assert (got[k] == GUARD[dt]).all()
    assert got["tick"] == want["tick"]


def test_gate_without_a_recovery_policy_selects_nothing():
    """The Q_risk group alone: the gate is evaluated and traced (the bits of the full launch's first step), the executed
    action stays the task action."""
    want = views(Launch("navigation2", 65, 1, True, 0).run(), 65, 1)
    alone = Launch("navigation2", 65, 1, True, 0)
    for k in ("rW1", "rb1", "rW2p", "rb2", "rW3", "rb3", "rscale", "rbias", "rlog_std"):
        setattr(alone.args, k, None)
    got = views(alone.run(), 65, 1)
    assert got["tr_z"].tobytes() == want["tr_z"].tobytes() and got["tr_task"].tobytes() == want["tr_task"].tobytes()
    assert np.array_equal(got["tr_flags"] & 17, want["tr_flags"] & 17) and ((got["tr_flags"] >> 4) & 1).any()
    assert got["tr_real"].tobytes() == got["tr_task"].tobytes()
    assert (got["tr_eps"] == GUARD[torch.float32]).all()


@pytest.mark.parametrize("S", [2, 3])
def test_packed_launch_is_the_solo_launches(S):
    """S seeds that differ in n, T, env kind, weights, groups and reset: each seed's outputs and trace equal its solo launch
    bit for bit, and each seed's own tick advances by its own T + reset."""
    cases = [("navigation1", 65, 7, True, 0), ("navigation2", 17, 2, False, 1), ("navigation2", 130, 101, True, 1)][:S]
    solo = [Launch(*c).run() for c in cases]
    packed = launch_packed([Launch(*c) for c in cases])
    for c, a, b in zip(cases, solo, packed):
        assert same_bits(a, b), c
        assert b["tick"] == [EC.TICK + c[2] + c[4], 0]
