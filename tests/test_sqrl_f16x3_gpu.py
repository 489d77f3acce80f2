"""SQRL acting with f16x3 scores on the GPU: rrl_w2_pack_f16x3 against numpy's float16 split bit for bit, rrl_sqrl_act_f16x3
against rrl_sqrl_act (candidates, log-probabilities and draws: the same bits), against the float64 restatement (decisions)
and against the rule of tests/sqrl_f16x3_cases.py (scores), its independence of the tiling, saturation, the tick protocol
inside a captured graph, and rrl_sqrl_act_f16x3_packed against the solo entry bit for bit."""
import ctypes as C
import functools
import types

import numpy as np
import pytest
import torch

import sqrl_f16x3_cases as SC
from recovery_rl_amd import _lib
from recovery_rl_amd.fast_update import FastActor
from test_sqrl_act_cpu import KS, MODES, NS, PHILOX_SEED, TICK, case, draws, left_out_cap, make_agent, weights64
from test_sqrl_act_gpu import DIAG, buffers, launch, same

pytestmark = pytest.mark.gpu
DEV = "cuda"
EINVAL = -1
GUARD = 64                               # floats behind a packed stream that the pack kernel must not touch


def pack_f16x3(W2):
    """The hi / lo stream of W2 [G, H, H], with GUARD poisoned floats behind it."""
    G, H, _ = W2.shape
    buf = torch.full((G * H * H + GUARD,), float("nan"), device=DEV)
    _lib.check(_lib.load().rrl_w2_pack_f16x3(G, H, W2.data_ptr(), buf.data_ptr(), _lib.current_stream()), "rrl_w2_pack_f16x3")
    return buf


def unpack_f16x3(stream, G, H):
    """(hi, lo) [G, H, H] float16 of a stream, by the layout rrl_hip.h documents: slot (n, 2 jp, lane) = hi[8] and slot
    (n, 2 jp + 1, lane) = lo[8] of W2[g][16 n + lane % 16][32 jp + 8 (lane / 16) + 0..7]."""
    halves = stream[:G * H * H].cpu().numpy().view(np.float16).reshape(G, H // 16, H // 16, 64, 8)     # [g][n][slot][lane][t]
    out = []
    for plane in (halves[:, :, 0::2], halves[:, :, 1::2]):                   # [g][n][jp][lane = 16 q + i][t]
        p = plane.reshape(G, H // 16, H // 32, 4, 16, 8)                     # [g][n][jp][q][i][t]
        out.append(p.transpose(0, 1, 4, 2, 3, 5).reshape(G, H, H))           # [g][16 n + i][32 jp + 8 q + t]
    return out


@pytest.fixture(scope="module")
def rig():
    """The weights of tests/test_sqrl_act_gpu.py with their hi / lo stream, and a second Q_risk (a seeded perturbation) with
    both of its streams."""
    agent = make_agent(DEV)
    fast = agent.enable_fast_path(256)
    fast.w2h = pack_f16x3(fast.qrisk.p["W2"])
    g = torch.Generator(device=DEV).manual_seed(77)
    p2 = {name: (t + 0.05 * torch.randn(t.shape, device=DEV, generator=g)).contiguous() for name, t in fast.qrisk.p.items()}
    w2p = torch.empty_like(fast.qrisk.w2_packed())
    _lib.check(_lib.load().rrl_w2_pack(2, 256, p2["W2"].data_ptr(), w2p.data_ptr(), _lib.current_stream()), "rrl_w2_pack")
    other = types.SimpleNamespace(qrisk=types.SimpleNamespace(p=p2, w2_packed=lambda: w2p), scale=fast.scale, bias=fast.bias,
                                  w2h=pack_f16x3(p2["W2"]))
    torch.cuda.synchronize()
    cases = functools.lru_cache(maxsize=None)(lambda n, k: case(agent, n, k, device=DEV))   # one restatement per shape, shared
    emu32 = functools.lru_cache(maxsize=None)(lambda n, k: SC.emulate(weights64(agent), cases(n, k), np.float32))
    return agent, fast, other, cases, emu32


def descriptor(net, obs, head, k, eps_safe, out, n_part=1, part_stride=0, eps=None, u=None, seed=PHILOX_SEED, counter=TICK,
               tick=None):
    p, P = _lib.ptr, net.qrisk.p
    return _lib.rrl_sqrl_act_t(n=obs.shape[0], k=k, H=256, d_obs=2, d_act=2, obs=p(obs), head=p(head), n_part=n_part,
                               part_stride=part_stride, scale=p(net.scale), bias=p(net.bias), W1=p(P["W1"]), b1=p(P["b1"]),
                               W2p=p(net.w2h), b2=p(P["b2"]), W3=p(P["W3"]), b3=p(P["b3"]), eps_safe=float(eps_safe),
                               seed=seed, counter=counter if tick is None else 0, counter_dev=p(tick),
                               counter_inc=0 if tick is None else 1, eps_in=p(eps), u_in=p(u),
                               **{name: p(t) for name, t in out.items()})


def launch16(net, obs, head, k, eps_safe, out=None, **kw):
    """One rrl_sqrl_act_f16x3 launch (the arguments of test_sqrl_act_gpu.launch) on net's hi / lo stream."""
    out = buffers(obs.shape[0], k) if out is None else out
    a = descriptor(net, obs, head, k, eps_safe, out, **kw)
    _lib.check(_lib.load().rrl_sqrl_act_f16x3(C.byref(a), _lib.current_stream()), "rrl_sqrl_act_f16x3")
    return out


# ---- the pack ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ("random", "integers", "tiny"))
def test_pack_is_numpys_float16_split_in_the_documented_layout(kind):
    g = torch.Generator(device=DEV).manual_seed(11)
    W2 = {"random": lambda: torch.randn(2, 256, 256, device=DEV, generator=g) * 0.02,
          "integers": lambda: torch.randint(-2048, 2049, (2, 256, 256), device=DEV, generator=g).float(),
          "tiny": lambda: torch.randn(2, 256, 256, device=DEV, generator=g) * 2.0 ** -20}[kind]()     # hi: f16 subnormals
    stream = pack_f16x3(W2)
    torch.cuda.synchronize()
    assert bool(torch.isnan(stream[-GUARD:]).all())                           # nothing behind the G H H floats was written
    hi, lo = unpack_f16x3(stream, 2, 256)
    w = W2.cpu().numpy()
    want_hi = w.astype(np.float16)
    want_lo = (w - want_hi.astype(np.float32)).astype(np.float16)
    assert np.array_equal(hi.view(np.uint16), want_hi.view(np.uint16))
    assert np.array_equal(lo.view(np.uint16), want_lo.view(np.uint16))
    if kind == "integers":
        assert not lo.any()                                                   # |w| <= 2048: exact in f16
    if kind == "random":                                                      # |w| < 1/8: every lo is an f16 subnormal, kept
        nz = lo[lo != 0]
        assert nz.size > 100000 and np.abs(nz.astype(np.float32)).max() < 2.0 ** -14
    if kind == "tiny":                                                        # hi itself is subnormal; nothing is flushed
        assert np.count_nonzero(hi) > 100000 and np.abs(hi.astype(np.float32)).max() < 2.0 ** -14


# ---- scores and decisions ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("k", KS)
def test_scores_and_decisions(rig, n, k):
    """Every shape and threshold: cand and logp are rrl_sqrl_act's bits for the same draws (own and injected), z obeys the
    rule against float64 and stays inside the project's bars, the decisions equal the float64 restatement's on every row that
    is not ambiguous, the action is the candidate at the pick."""
    agent, fast, _, cases, emu32 = rig
    c = cases(n, k)
    obs, head = c["obs"], c["head"]
    eps, u = torch.as_tensor(c["eps"], device=DEV), torch.as_tensor(c["u"], device=DEV)
    rows = torch.arange(n, device=DEV)
    z64, q64 = c["scores"]["z"], c["scores"]["q"]
    scale, bound = float(np.abs(z64).max()), SC.bound(z64, emu32(n, k)["z"])
    for mode in MODES:
        thr, want = c["thr"][mode], c["pick"][mode]
        own = launch16(fast, obs, head, k, thr)                       # the kernel's own draws at (PHILOX_SEED, TICK)
        inj = launch16(fast, obs, head, k, thr, eps=eps, u=u)         # the oracle's regeneration of them, injected
        assert same(own, inj), mode
        f32 = launch(fast, obs, head, k, thr)
        assert torch.equal(own["cand"], f32["cand"]) and torch.equal(own["logp"], f32["logp"]), mode
        assert not any(bool(torch.isnan(t).any()) for t in own.values() if t.is_floating_point())
        dev = SC.deviation(own["z"].double().cpu().numpy(), z64)
        dq = float(np.abs(own["q"].double().cpu().numpy() - q64).max())
        print("n=%d k=%d %s: z deviation %.3e (bound %.3e, f32 kernel %.3e, scale %.3e), q %.3e"
              % (n, k, mode, dev, bound, SC.deviation(f32["z"].double().cpu().numpy(), z64), scale, dq))
        assert dev <= bound, (dev, bound)
        assert dev <= 1e-4 * scale and dq <= 1e-5
        keep = ~want["ambiguous"]
        assert (~keep).sum() <= left_out_cap(n), (mode, int((~keep).sum()))
        for name in ("n_safe", "cstar", "pick"):
            got = own[name].cpu().numpy()
            assert np.array_equal(got[keep], want[name][keep]), (mode, name, np.flatnonzero(got != want[name]))
        assert torch.equal(own["action"], own["cand"][rows, own["pick"].long()]), mode


def test_a_candidates_z_does_not_depend_on_k_tile_or_pass(rig):
    """The first 100 candidates at k = 100 (two passes: 64 + 36 rows) and at k = 128 (64 + 64), candidates 0..15 at k = 16
    (one tile) and at k = 17 (two): the same obs, head and injected noise give the same z, bit for bit."""
    _, fast, _, cases, _ = rig
    n = 3
    c = cases(n, 128)
    eps = torch.as_tensor(c["eps"], device=DEV)                                 # [n, 128, 2]
    z = {}
    for k in (16, 17, 100, 128):
        out = launch16(fast, c["obs"], c["head"], k, 0.5, eps=eps[:, :k].contiguous())
        z[k] = out["z"]
        assert not bool(torch.isnan(out["z"]).any())
    assert torch.equal(z[100], z[128][:, :, :100]) and torch.equal(z[16], z[17][:, :, :16])
    assert torch.equal(z[16], z[128][:, :, :16])                                # ... and a one-pass launch against a two-pass one


def test_saturation(rig):
    """Observations scaled until almost half of the layer-1 activations exceed 65504: every output finite, z inside the rule
    against the emulation WITH the clamp (float64 reference and f32 basis both)."""
    agent, fast, _, _, _ = rig
    c = SC.saturation_case(agent, device=DEV)
    assert c["saturated"] > 0.1
    W = weights64(agent)
    z64, z32 = SC.emulate(W, c)["z"], SC.emulate(W, c, np.float32)["z"]
    n, k = c["scores"]["q"].shape
    out = launch16(fast, c["obs"].contiguous(), c["head"], k, 0.5, eps=torch.as_tensor(c["eps"], device=DEV),
                   u=torch.as_tensor(c["u"], device=DEV))
    assert all(bool(torch.isfinite(t).all()) for t in out.values() if t.is_floating_point())
    assert bool((out["pick"] >= 0).all()) and bool((out["pick"] < k).all())
    dev, bound = SC.deviation(out["z"].double().cpu().numpy(), z64), SC.bound(z64, z32)
    print("saturation: z deviation %.3e, bound %.3e, scale %.3e" % (dev, bound, float(np.abs(z64).max())))
    assert dev <= bound


# ---- tick and graph ------------------------------------------------------------------------------------------------------
def test_tick_and_graph(rig):
    """The protocol of the f32 test: two eager launches at ticks t and t + 1 equal the launches with the oracle's draws
    injected; a captured graph holding PACK + LAUNCH, replayed twice from tick t, gives those two results (from a stream the
    graph itself re-makes) and leaves the tick at t + 2."""
    _, fast, _, cases, _ = rig
    n, k, t0 = 65, 100, 1234567
    c = cases(n, k)
    thr = c["thr"]["mixed"]
    tick = torch.tensor([t0, 0], dtype=torch.int64, device=DEV)
    first = launch16(fast, c["obs"], c["head"], k, thr, tick=tick)
    second = launch16(fast, c["obs"], c["head"], k, thr, tick=tick)
    assert tick.tolist() == [t0 + 2, 0]
    assert not torch.equal(first["action"], second["action"]) and not torch.equal(first["cand"], second["cand"])
    for t, got in ((t0, first), (t0 + 1, second)):
        eps, u = draws(n, k, PHILOX_SEED, t)
        assert same(got, launch16(fast, c["obs"], c["head"], k, thr, eps=torch.as_tensor(eps, device=DEV),
                                  u=torch.as_tensor(u, device=DEV)))
    tick.copy_(torch.tensor([t0, 0]))
    out = buffers(n, k)
    W2 = fast.qrisk.p["W2"]
    net = types.SimpleNamespace(qrisk=fast.qrisk, scale=fast.scale, bias=fast.bias, w2h=torch.zeros_like(fast.w2h))
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        _lib.check(_lib.load().rrl_w2_pack_f16x3(2, 256, W2.data_ptr(), net.w2h.data_ptr(), _lib.current_stream()), "pack")
        launch16(net, c["obs"], c["head"], k, thr, tick=tick, out=out)
    assert tick.tolist() == [t0, 0] and not bool(net.w2h.any())        # the capture executed nothing
    for want in (first, second):
        g.replay()
        torch.cuda.synchronize()
        assert same(want, out)
    assert tick.tolist() == [t0 + 2, 0] and torch.equal(net.w2h[:-GUARD], fast.w2h[:-GUARD])


def test_fast_actor_act_sqrl_under_the_switch_is_pack_and_launch(rig):
    _, fast, _, cases, _ = rig
    n, k = 65, 100
    c = cases(n, k)
    actor = FastActor(fast, n)
    actor.sqrl_seed, actor.sqrl_f16x3 = PHILOX_SEED, True
    actor.sqrl_tick[0] = TICK
    diag = {name: t for name, t in buffers(n, k).items() if name != "action"}
    action = actor.act_sqrl(c["obs"], c["thr"]["mixed"], k=k, diag=diag)
    assert action is actor.task_action and actor.sqrl_tick.tolist() == [TICK + 1, 0]
    assert torch.equal(actor.sqrl_w2h, fast.w2h[:-GUARD])
    head, n_part, ps = actor.pol.parts
    direct = launch16(fast, c["obs"], head, k, c["thr"]["mixed"], n_part=n_part, part_stride=ps)
    assert torch.equal(action, direct["action"]) and all(torch.equal(diag[name], direct[name]) for name in diag)


# ---- packed ----------------------------------------------------------------------------------------------------------------
def seed_inputs(rig, s, k=100):
    _, fast, other, cases, _ = rig
    n = (3, 65, 3)[s]
    c = cases(n, k)
    return types.SimpleNamespace(n=n, k=k, net=(fast, other)[s % 2], obs=c["obs"], head=c["head"], thr=c["thr"][MODES[s % 3]],
                                 seed=PHILOX_SEED + 7919 * s, t0=1000 + 17 * s)


def tick_of(x):
    return torch.tensor([x.t0, 0], dtype=torch.int64, device=DEV)


@pytest.mark.parametrize("S", (1, 2, 3))
def test_packed_equals_the_solo_entry_bit_for_bit(rig, S):
    lib = _lib.load()
    xs = [seed_inputs(rig, s) for s in range(S)]
    want = []
    for x in xs:
        tick = tick_of(x)
        want.append([launch16(x.net, x.obs, x.head, x.k, x.thr, seed=x.seed, tick=tick) for _ in range(2)])
        assert tick.tolist() == [x.t0 + 2, 0]
    ticks = [tick_of(x) for x in xs]
    for turn in (0, 1):
        outs = [buffers(x.n, x.k) for x in xs]
        args = (_lib.rrl_sqrl_act_t * S)(*[descriptor(x.net, x.obs, x.head, x.k, x.thr, o, seed=x.seed, tick=t)
                                           for x, t, o in zip(xs, ticks, outs)])
        assert lib.rrl_sqrl_act_f16x3_packed(S, args, _lib.current_stream()) == 0
        torch.cuda.synchronize()
        for s in range(S):
            assert same(outs[s], want[s][turn]), (turn, s)
            assert not any(bool(torch.isnan(t).any()) for t in outs[s].values() if t.is_floating_point())
    assert all(t.tolist() == [x.t0 + 2, 0] for t, x in zip(ticks, xs))          # every seed's own tick
    if S > 1:
        assert not torch.equal(want[0][0]["z"], want[1][0]["z"][:, :3]) and xs[0].net is not xs[1].net
    lib.rrl_pack_clear()


def test_packed_seeds_with_different_k_are_refused_before_any_launch(rig):
    lib = _lib.load()
    xs = [seed_inputs(rig, 0, 100), seed_inputs(rig, 1, 128)]
    ticks, outs = [tick_of(x) for x in xs], [buffers(x.n, x.k) for x in xs]
    args = (_lib.rrl_sqrl_act_t * 2)(*[descriptor(x.net, x.obs, x.head, x.k, x.thr, o, seed=x.seed, tick=t)
                                       for x, t, o in zip(xs, ticks, outs)])
    lib.rrl_pack_clear()
    assert lib.rrl_sqrl_act_f16x3_packed(2, args, _lib.current_stream()) == EINVAL
    torch.cuda.synchronize()
    for x, t, o in zip(xs, ticks, outs):
        assert t.tolist() == [x.t0, 0]
        assert all(bool((torch.isnan(v) if v.is_floating_point() else v == -77).all()) for v in o.values())   # still poisoned
    assert lib.rrl_pack_clear() == 0                                            # nothing was stored either
