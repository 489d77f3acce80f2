"""Q-sampling recovery acting with f16x3 scores on the GPU: rrl_qsample_act_f16x3, rrl_qsample_act_gated_f16x3 and
rrl_qsample_act_f16x3_packed called through the C ABI, on the hi / lo stream rrl_w2_pack_f16x3 writes, against the float64
chain of tests/test_qsample_act_cpu.py under the rules of tests/qsample_f16x3_cases.py (rule Z on z, rule Q on the pick), and
bit for bit against the f32 entries wherever the arithmetic of layer 2 does not enter: draws, candidates, gate, fold, tick."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

import qsample_f16x3_cases as QC
import sqrl_f16x3_cases as SC
from recovery_rl_amd import _lib
from test_qsample_act_cpu import BOXES, EINVAL, ERANGE, PHILOX_SEED, TICK, argmin_first, candidates, make_agent
from test_qsample_act_gpu import POISON_I, buffers, check_ungated, gated_rows, launch, masks, same, weights_of

pytestmark = pytest.mark.gpu
DEV = "cuda"
ENTRY, GATED, PACKED = "rrl_qsample_act_f16x3", "rrl_qsample_act_gated_f16x3", "rrl_qsample_act_f16x3_packed"


def stream_of(W2):
    """The hi / lo fragment stream of the two heads' [256, 256] hidden weights, as rrl_sqrl_act_f16x3 reads it."""
    w2h = torch.empty(W2.numel(), dtype=torch.float32, device=DEV)
    _lib.check(_lib.load().rrl_w2_pack_f16x3(2, 256, W2.data_ptr(), w2h.data_ptr(), _lib.current_stream()), "rrl_w2_pack_f16x3")
    torch.cuda.synchronize()
    return w2h


@pytest.fixture(scope="module")
def rigs():
    """Per action box: Q_risk's weights as the f32 launch takes them (W), the same with W2p = the f16x3 stream (H), and the
    live W2."""
    out = {}
    for box in BOXES:
        fast = make_agent(DEV, box).enable_fast_path(256)
        W = weights_of(fast)
        out[box] = (W, dict(W, W2p=stream_of(fast.qrisk.p["W2"])), fast.qrisk.p["W2"])
    return out


def box_of(box):
    return tuple(torch.tensor(b, dtype=torch.float32, device=DEV) for b in BOXES[box])


def descriptor(W, obs, k, box, out, scratch, mask=None, cand_in=None, seed=PHILOX_SEED, counter=0, tick=None, inc=0):
    p = _lib.ptr
    lo, hi = box
    return _lib.rrl_qsample_act_t(n=obs.shape[0], k=k, H=256, d_obs=2, d_act=2, obs=p(obs), mask=p(mask), lo=p(lo), hi=p(hi),
                                  seed=seed, counter=counter, counter_dev=p(tick), counter_inc=inc, cand_in=p(cand_in),
                                  scratch=p(scratch), **{name: p(t) for name, t in W.items()},
                                  **{name: p(out[name]) for name in ("action", "q", "z", "cand", "pick")})


def scratch_for(n, k):
    return torch.full((int(_lib.load().rrl_qsample_scratch_floats(n, k)),), float("nan"), device=DEV)


def launch16(H, obs, k, box, mask=None, cand_in=None, seed=PHILOX_SEED, counter=TICK, tick=None, inc=1, out=None):
    """One rrl_qsample_act_f16x3 call, with the arguments of test_qsample_act_gpu.launch."""
    n = obs.shape[0]
    out = buffers(n, k) if out is None else out
    bx, scratch = box_of(box), scratch_for(n, k)
    a = descriptor(H, obs, k, bx, out, scratch, mask=mask, cand_in=cand_in, seed=seed, counter=counter if tick is None else 0,
                   tick=tick, inc=0 if tick is None else inc)
    _lib.check(getattr(_lib.load(), ENTRY)(C.byref(a), _lib.current_stream()), ENTRY)
    torch.cuda.synchronize()
    return out


# ---- draws, scores, pick ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,k,box", QC.CASES)
def test_draws_scores_and_pick(rigs, n, k, box):
    """Every case and mask: the candidates are the f32 entry's and the float64 restatement's bits, the kernel's own draws and
    their injection give the same output bits, rule Z holds on z and rule Q on the pick, the pick is the lowest-index argmin
    of the kernel's own q, the action is the candidate at the pick, nothing of an ungated env is written."""
    W, H, _ = rigs[box]
    c = QC.table_case(n, k, box)
    obs, cand32 = torch.tensor(c["obs"], device=DEV), torch.tensor(c["cand"], device=DEV)
    B = SC.bound(c["z"], c["e32"]["z"])                                   # the case's rule-Z bound
    fresh = buffers(n, k)
    for name, mask in masks(n).items():
        own = launch16(H, obs, k, box, mask=mask)                        # the kernel's own draws at (PHILOX_SEED, TICK)
        inj = launch16(H, obs, k, box, mask=mask, cand_in=cand32)        # the oracle's regeneration of them, injected
        f32 = launch(W, obs, k, box, mask=mask)
        assert same(own, inj), name
        assert torch.equal(own["cand"].view(torch.int32), f32["cand"].view(torch.int32)), name
        gated = gated_rows(mask, n)
        check_ungated(own, fresh, gated)
        if not gated.any():
            continue
        g = np.flatnonzero(gated)
        got = {key: t.cpu().numpy() for key, t in own.items()}
        assert got["cand"][g].tobytes() == c["cand"][g].tobytes(), name                 # bit for bit
        z64 = c["z"][:, g]
        dev, dev32 = SC.deviation(got["z"][:, g], z64), SC.deviation(f32["z"].cpu().numpy()[:, g], z64)
        qerr = float(np.abs(got["q"][g].astype(np.float64) - c["q"][g]).max())
        print("n=%d k=%d %s %s: z deviation %.3e, bound %.3e, f32 kernel %.3e, scale %.3e; q error %.3e"
              % (n, k, box, name, dev, B, dev32, float(np.abs(z64).max()), qerr))
        assert dev <= B, (name, dev, B)                                                  # rule Z
        pick = got["pick"][g]
        assert np.array_equal(pick, argmin_first(got["q"][g])), name
        assert got["action"][g].tobytes() == got["cand"][g, pick].tobytes(), name
        assert QC.rule_q_holds(c["q"][g], pick, B), (name, float((c["q"][g][np.arange(len(g)), pick] - c["q"][g].min(1)).max()), B)


def test_saturation_case(rigs):
    """Observations times 2^21: layer-1 activations above 65504 are clamped, as the float64 emulation clamps them."""
    _, H, _ = rigs["unit"]
    c = QC.saturation_case()
    n, k, box = QC.SAT_SHAPE
    print("share of layer-1 activations above 65504: %.3f" % c["saturated"])
    assert c["saturated"] > 0 and np.isfinite(c["z"]).all()
    out = launch16(H, torch.tensor(c["obs"], device=DEV), k, box)
    got = {key: t.cpu().numpy() for key, t in out.items()}
    assert got["cand"].tobytes() == c["cand"].tobytes()
    assert np.isfinite(got["z"]).all() and np.isfinite(got["q"]).all() and np.isfinite(got["action"]).all()
    B = SC.bound(c["z"], c["e32"]["z"])
    dev = SC.deviation(got["z"], c["z"])
    print("saturation: z deviation %.3e, bound %.3e, scale %.3e" % (dev, B, float(np.abs(c["z"]).max())))
    assert dev <= B
    assert np.array_equal(got["pick"], argmin_first(got["q"])) and QC.rule_q_holds(c["q"], got["pick"], B)


def test_ties_and_nan(rigs):
    """All candidates identical: pick 0.  The best candidate copied into an earlier and a later chunk: the earliest copy.  A NaN
    candidate is picked and its q is NaN; of two NaNs the first."""
    _, H, _ = rigs["unit"]
    n, k = 3, 1000
    c = QC.table_case(n, k, "unit")
    obs, rows = torch.tensor(c["obs"], device=DEV), torch.arange(n, device=DEV)
    flat = torch.tensor(c["cand"][:, :1], device=DEV).expand(n, k, 2).contiguous()
    out = launch16(H, obs, k, "unit", cand_in=flat)
    assert out["pick"].tolist() == [0] * n and bool((out["q"] == out["q"][:, :1]).all())
    assert torch.equal(out["action"], flat[:, 0])

    base = launch16(H, obs, k, "unit", cand_in=torch.tensor(c["cand"], device=DEV))
    best = base["pick"].long()
    dup = torch.tensor(c["cand"], device=DEV)
    for at in (5, 100, 640, 900, 999):                                    # chunks 0, 0, 5, 7, 7 (the last: 104 rows)
        dup[rows, at] = dup[rows, best]
    out = launch16(H, obs, k, "unit", cand_in=dup)
    assert torch.equal(out["pick"].long(), best.clamp(max=5))             # the earliest copy, whichever chunk holds the original
    assert torch.equal(out["action"], dup[rows, best]) and torch.equal(out["q"][rows, 5], base["q"][rows, best])
    for at in (0, 127, 128, 900, 999):                                    # one copy: the lower index of the two
        one = torch.tensor(c["cand"], device=DEV)
        one[rows, at] = one[rows, best]
        assert torch.equal(launch16(H, obs, k, "unit", cand_in=one)["pick"].long(), best.clamp(max=at)), at

    for at in (0, 130, 700, 999):
        bad = torch.tensor(c["cand"], device=DEV)
        bad[:, at, 1] = float("nan")
        out = launch16(H, obs, k, "unit", cand_in=bad)
        assert out["pick"].tolist() == [at] * n
        assert bool(torch.isnan(out["action"][:, 1]).all()) and torch.equal(out["action"][:, 0], bad[:, at, 0])
        assert bool(torch.isnan(out["q"][:, at]).all()) and int(torch.isnan(out["q"]).sum()) == n
    two = torch.tensor(c["cand"], device=DEV)
    two[:, 300, 0] = float("nan")
    two[:, 40, 0] = float("nan")
    assert launch16(H, obs, k, "unit", cand_in=two)["pick"].tolist() == [40] * n       # the first NaN


def test_tick_and_graph(rigs):
    """The host counter gives what the device tick gives; the device tick advances by exactly counter_inc per call whatever the
    mask holds; a captured graph holding the call, replayed, equals the eager calls bit for bit; tick and draws are the f32
    entry's at the same tick."""
    W, H, _ = rigs["asym"]
    n, k, t0, inc = 3, 129, 1234567, 3
    obs = torch.tensor(QC.table_case(n, k, "asym")["obs"], device=DEV)
    m = masks(n)
    tick = torch.tensor([t0, 0], dtype=torch.int64, device=DEV)
    fresh = buffers(n, k)
    none = launch16(H, obs, k, "asym", mask=m["zeros"], tick=tick, inc=inc)
    assert tick.tolist() == [t0 + inc, 0] and same(none, fresh)             # honoured once, by env 0's fold thread
    tick.copy_(torch.tensor([t0, 0]))
    first = launch16(H, obs, k, "asym", mask=m["alternating"], tick=tick, inc=inc)
    second = launch16(H, obs, k, "asym", mask=m["alternating"], tick=tick, inc=inc)
    assert tick.tolist() == [t0 + 2 * inc, 0]
    assert not torch.equal(first["cand"][0], second["cand"][0]) and not torch.equal(first["action"][0], second["action"][0])
    tick32 = torch.tensor([t0, 0], dtype=torch.int64, device=DEV)
    for t, got in ((t0, first), (t0 + inc, second)):
        assert same(got, launch16(H, obs, k, "asym", mask=m["alternating"], counter=t))        # host counter = device tick
        want = torch.tensor(candidates(n, k, "asym", PHILOX_SEED, t), device=DEV)
        assert torch.equal(got["cand"][0], want[0]) and torch.equal(got["cand"][2], want[2])
        f32 = launch(W, obs, k, "asym", mask=m["alternating"], tick=tick32, inc=inc)            # the f32 entry at the same tick
        assert torch.equal(got["cand"].view(torch.int32), f32["cand"].view(torch.int32))
    assert tick32.tolist() == tick.tolist()
    tick.copy_(torch.tensor([t0, 0]))
    out = buffers(n, k)
    bx, scratch = box_of("asym"), scratch_for(n, k)
    a = descriptor(H, obs, k, bx, out, scratch, mask=m["alternating"], tick=tick, inc=inc)
    lib = _lib.load()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        _lib.check(lib.rrl_qsample_act_f16x3(C.byref(a), _lib.current_stream()), ENTRY)
    assert tick.tolist() == [t0, 0]                                    # the capture executed nothing
    for want in (first, second):
        g.replay()
        torch.cuda.synchronize()
        assert same(want, out)
    assert tick.tolist() == [t0 + 2 * inc, 0]


# ---- the gate in the launch ------------------------------------------------------------------------------------------------
def outputs(n, k):
    """The poisoned buffers plus what a gate in the launch writes: recovery (poison 9) and task_out (NaN)."""
    out = buffers(n, k)
    out["recovery"] = torch.full((n,), 9, dtype=torch.uint8, device=DEV)
    out["task_out"] = torch.full((n, 2), float("nan"), device=DEV)
    return out


def differing(a, b):
    bits = lambda t: t if t.dtype == torch.uint8 else t.view(torch.int32)
    return [name for name in a if not torch.equal(bits(a[name]), bits(b[name]))]


def gate_of(parts, eps, xa, out):
    p = _lib.ptr
    return _lib.rrl_qsample_gate_t(z=p(parts), n_part=parts.shape[0], part_stride=parts.stride(0), eps_safe=float(eps),
                                   task_action=p(xa[:, 2:4]), ld_task=xa.stride(0), task_out=p(out["task_out"]),
                                   recovery_out=p(out["recovery"]))


def partials(n, n_part, seed):
    """Partial last-layer sums [n_part, 2, n] of z = Q_risk(s, a_task) around 0, and their in-order f32 sum [2, n]."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    parts = 0.8 * torch.randn(n_part, 2, n, device=DEV, generator=g)
    z = parts[0].clone()
    for i in range(1, n_part):
        z = z + parts[i]
    return parts.contiguous(), z.contiguous()


@pytest.mark.parametrize("n_part", (1, 4))
def test_gated_call_equals_recovery_select_then_the_masked_call(rigs, n_part):
    lib, st = _lib.load(), _lib.current_stream()
    _, H, _ = rigs["unit"]
    n, k, eps, t0, inc = 65, 129, 0.5, 4321, 2                         # z around 0: sigmoid around 1/2, a mixed gate
    obs = torch.tensor(QC.table_case(n, k, "unit")["obs"], device=DEV)
    g = torch.Generator(device=DEV).manual_seed(7 + n_part)
    xa = torch.randn(n, 4, device=DEV, generator=g)                    # [s | a_task]: the task action at stride 4
    parts, zsum = partials(n, n_part, 100 + n_part)
    bx = box_of("unit")
    want, tick = outputs(n, k), torch.tensor([t0, 0], dtype=torch.int64, device=DEV)
    dummy = torch.zeros(n, 2, device=DEV)
    _lib.check(lib.rrl_recovery_select(n, zsum.data_ptr(), eps, xa[:, 2:4].data_ptr(), 4, dummy.data_ptr(),
                                       want["action"].data_ptr(), want["recovery"].data_ptr(), want["task_out"].data_ptr(), st),
               "rrl_recovery_select")
    scratch = scratch_for(n, k)
    a = descriptor(H, obs, k, bx, want, scratch, mask=want["recovery"], tick=tick, inc=inc)
    _lib.check(lib.rrl_qsample_act_f16x3(C.byref(a), st), ENTRY)
    got, tick2, scratch2 = outputs(n, k), torch.tensor([t0, 0], dtype=torch.int64, device=DEV), scratch_for(n, k)
    a2, g2 = descriptor(H, obs, k, bx, got, scratch2, tick=tick2, inc=inc), gate_of(parts, eps, xa, got)
    _lib.check(lib.rrl_qsample_act_gated_f16x3(C.byref(a2), C.byref(g2), st), GATED)
    torch.cuda.synchronize()
    assert not differing(got, want), differing(got, want)
    assert tick.tolist() == tick2.tolist() == [t0 + inc, 0]
    rec = got["recovery"].bool()
    assert 0 < int(rec.sum()) < n                                      # the mask is mixed
    assert torch.equal(got["task_out"], xa[:, 2:4]) and torch.equal(got["action"][~rec], xa[:, 2:4][~rec])
    assert bool(torch.isnan(got["q"][~rec]).all()) and bool((got["pick"][~rec] == POISON_I).all())
    assert not bool(torch.isnan(got["q"][rec]).any()) and bool((got["pick"][rec] >= 0).all())


# ---- packed ----------------------------------------------------------------------------------------------------------------
def seed_inputs(rigs, s, k):
    """Seed s of a packed call: its own env count (3, 65, 3), box and weights, mask family, gate, Philox seed, tick."""
    n = (3, 65, 3)[s]
    box = ("unit", "asym", "maze")[s]
    _, H, _ = rigs[box]
    mask = masks(n)[("alternating", "ends", "ones")[s]]
    z = torch.where(mask.bool(), 5.0, -5.0)
    parts = torch.stack([z, z]).unsqueeze(0).repeat(1 + s, 1, 1).contiguous() / (1 + s)       # [n_part, 2, n]
    g = torch.Generator(device=DEV).manual_seed(300 + s)
    return types.SimpleNamespace(n=n, k=k, box=box_of(box), H=H, obs=torch.tensor(QC.observations(n, 11 + s), device=DEV), mask=mask,
                                 eps=0.3 + 0.05 * s, parts=parts, xa=torch.randn(n, 4, device=DEV, generator=g),
                                 seed=PHILOX_SEED + 7919 * s, t0=1000 + 17 * s, inc=1 + s, scratch=scratch_for(n, k))


def pair_of(x, tick, out, gated):
    a = descriptor(x.H, x.obs, x.k, x.box, out, x.scratch, mask=None if gated else x.mask, seed=x.seed, tick=tick, inc=x.inc)
    return a, (gate_of(x.parts, x.eps, x.xa, out) if gated else None)


def solo_call(x, tick, out, gated):
    lib, st = _lib.load(), _lib.current_stream()
    a, g = pair_of(x, tick, out, gated)
    if gated:
        _lib.check(lib.rrl_qsample_act_gated_f16x3(C.byref(a), C.byref(g), st), GATED)
    else:
        _lib.check(lib.rrl_qsample_act_f16x3(C.byref(a), st), ENTRY)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("S", (1, 2, 3))
@pytest.mark.parametrize("gated", (True, False))
def test_packed_equals_stand_alone_bit_for_bit(rigs, S, gated):
    """Every seed's outputs and tick equal its solo launch's bit for bit, with and without gates; S = 1 is the solo entry."""
    lib, st, k = _lib.load(), _lib.current_stream(), 129
    xs = [seed_inputs(rigs, s, k) for s in range(S)]
    tick_of = lambda x: torch.tensor([x.t0, 0], dtype=torch.int64, device=DEV)
    want = []
    for x in xs:                                     # every seed alone, twice
        tick = tick_of(x)
        want.append((solo_call(x, tick, outputs(x.n, k), gated), solo_call(x, tick, outputs(x.n, k), gated)))
        assert tick.tolist() == [x.t0 + 2 * x.inc, 0]
    ticks = [tick_of(x) for x in xs]                 # the pack, twice
    got = [outputs(x.n, k) for x in xs], [outputs(x.n, k) for x in xs]
    for outs in got:
        pairs = [pair_of(x, t, o, gated) for x, t, o in zip(xs, ticks, outs)]
        args = (_lib.rrl_qsample_act_t * S)(*[p[0] for p in pairs])
        gates = (_lib.rrl_qsample_gate_t * S)(*[p[1] for p in pairs]) if gated else None
        assert lib.rrl_qsample_act_f16x3_packed(S, args, gates, st) == 0
    torch.cuda.synchronize()
    for s, x in enumerate(xs):
        assert not differing(got[0][s], want[s][0]) and not differing(got[1][s], want[s][1]), (gated, s)
        assert ticks[s].tolist() == [x.t0 + 2 * x.inc, 0], (gated, s)
        on = x.mask.bool()
        assert not torch.equal(got[0][s]["action"][on], got[1][s]["action"][on])       # the second call drew at the next tick
        assert not bool(torch.isnan(got[0][s]["q"][on]).any()) and bool(torch.isnan(got[0][s]["q"][~on]).all())
        if gated:
            assert torch.equal(got[0][s]["recovery"], x.mask)
    lib.rrl_pack_clear()


def test_packed_refusals_are_the_solo_entrys_and_leave_the_device_untouched(rigs):
    lib, st, S, k = _lib.load(), _lib.current_stream(), 3, 129
    xs = [seed_inputs(rigs, s, k) for s in range(S)]
    ticks = [torch.tensor([x.t0, 0], dtype=torch.int64, device=DEV) for x in xs]
    outs = [outputs(x.n, k) for x in xs]
    lib.rrl_pack_clear()
    for gated in (True, False):
        for fields, code in ((dict(k=1025), ERANGE), (dict(k=0), ERANGE), (dict(H=128), EINVAL), (dict(obs=None), EINVAL),
                             (dict(W2p=xs[2].H["W2p"].data_ptr() + 8), EINVAL)):
            pairs = [pair_of(x, t, o, gated) for x, t, o in zip(xs, ticks, outs)]
            for name, v in fields.items():
                setattr(pairs[2][0], name, v)
            args = (_lib.rrl_qsample_act_t * S)(*[p[0] for p in pairs])
            gates = (_lib.rrl_qsample_gate_t * S)(*[p[1] for p in pairs]) if gated else None
            solo = (lib.rrl_qsample_act_gated_f16x3(C.byref(pairs[2][0]), C.byref(pairs[2][1]), st) if gated
                    else lib.rrl_qsample_act_f16x3(C.byref(pairs[2][0]), st))
            assert solo == code == lib.rrl_qsample_act_f16x3_packed(S, args, gates, st), (gated, fields)
    torch.cuda.synchronize()
    for s, x in enumerate(xs):
        assert ticks[s].tolist() == [x.t0, 0] and not differing(outs[s], outputs(x.n, k)), s       # no output byte changed
        assert bool(torch.isnan(x.scratch).all())
    assert lib.rrl_pack_clear() == 0                                    # nothing was stored either


# ---- the stream is the caller's to keep current -----------------------------------------------------------------------------
def test_scores_follow_the_stream_until_it_is_packed_again(rigs):
    """W2 changed without a new rrl_w2_pack_f16x3: the scores are the old stream's (the contract: nothing but the caller keeps
    the stream current -- FastActor.act_qsample packs in front of every launch).  Packed again: they follow W2."""
    _, H, W2 = rigs["unit"]
    n, k = 3, 129
    c = QC.table_case(n, k, "unit")
    obs = torch.tensor(c["obs"], device=DEV)
    before = launch16(H, obs, k, "unit")
    live, mine = W2.clone(), dict(H, W2p=H["W2p"].clone())
    live.mul_(2.0)
    stale = launch16(mine, obs, k, "unit")
    assert same(before, stale)
    _lib.check(_lib.load().rrl_w2_pack_f16x3(2, 256, live.data_ptr(), mine["W2p"].data_ptr(), _lib.current_stream()), "rrl_w2_pack_f16x3")
    fresh = launch16(mine, obs, k, "unit")
    assert torch.equal(fresh["cand"], before["cand"]) and not torch.equal(fresh["z"], before["z"])
    Wq = [tuple(w * 2.0 if i == 2 else w for i, w in enumerate(head)) for head in QC.weights("unit")]
    z64 = QC.restate(Wq, c["obs"], c["cand"])["z"]
    z32 = QC.emulate(Wq, c["obs"], c["cand"], np.float32)["z"]
    assert SC.deviation(fresh["z"].cpu().numpy(), z64) <= SC.bound(z64, z32)
    assert SC.deviation(stale["z"].cpu().numpy(), z64) > SC.bound(z64, z32)
