"""The solo Adam launches take their two bias corrections from a device-side memo that the launch before filled
(csrc/update_kernels.hip: adam_memo) instead of two double pow() chains.  RRL_ADAM_MEMO=0 switches the memo off: every
segment then takes the pow() path that test_update_pieces_gpu.py holds against float64.

Every test here runs the same launches twice, on identical copies of the inputs: once with the memo, once with the off
switch.  After EVERY step each parameter, moment, target, fragment-order copy of W2 and step counter of the two must be the
same bits (torch.equal) -- there is no tolerance in this file.

The memo side's step counters come from one small pool, so that the whole file claims a handful of memo slots; the last
test then claims more than there are."""
import contextlib
import os

import pytest
import torch

from recovery_rl_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
p = _lib.ptr
LR, BETAS, ADAM_EPS = 3e-4, (0.9, 0.999), 1e-8
W2 = 256 * 256                                  # floats of one [256, 256] matrix
_POOL = {}


def counters(k):
    """The memo side's k-th step counter {t, ticket}: the same address in every test."""
    if "t" not in _POOL:
        _POOL["t"] = torch.zeros(16, 2, dtype=torch.int64, device=DEV)
    return _POOL["t"][k]


@contextlib.contextmanager
def memo(on):
    old = os.environ.pop("RRL_ADAM_MEMO", None)
    if not on:
        os.environ["RRL_ADAM_MEMO"] = "0"        # the launcher reads it at every call
    try:
        yield
    finally:
        os.environ.pop("RRL_ADAM_MEMO", None)
        if old is not None:
            os.environ["RRL_ADAM_MEMO"] = old


class Seg:
    """One segment's tensors on the device and its descriptor.  The two sides of a test build it from the same seed."""

    def __init__(self, n, step, t0=0, seed=1, target=False, g2=False, wd=0.0, parts=None, w2=None):
        gen = torch.Generator().manual_seed(seed)
        rnd = lambda *shape: torch.randn(*shape, generator=gen).to(DEV)
        self.t = dict(p=rnd(n), g=rnd(n) * 0.1, m=rnd(n) * 0.01, v=rnd(n).square() * 1e-3)
        self.step = step
        step.copy_(torch.tensor([t0, 0]))
        tau = 0.0
        if target:
            self.t["target"], tau = rnd(n), 0.005
        g2_t = rnd(n) * 0.1 if g2 else None
        gp, n_part, stride, pe = None, 0, 0, 0
        if parts:                                # (n_part, part_elems): the first part_elems gradients are the partials' sum
            n_part, pe = parts
            stride = pe + 8
            gp = rnd(n_part, stride) * 0.03
        w2_off, heads = 0, 0
        if w2:                                   # (w2_off, heads): fragment-order copies of the matrices and of the target's
            w2_off, heads = w2
            self.t["w2p"], self.t["target_w2p"] = torch.zeros(heads * W2, device=DEV), torch.zeros(heads * W2, device=DEV)
        self.keep = (g2_t, gp)
        t = self.t
        self.seg = _lib.rrl_adam_seg_t(n, p(t["p"]), p(t["g"]), p(t["m"]), p(t["v"]), p(step), p(t.get("target")), tau, wd,
                                       p(g2_t), p(gp), n_part, stride, pe, p(t.get("w2p")), p(t.get("target_w2p")), w2_off, heads)

    def state(self):
        return dict(self.t, step=self.step)


class Dual:
    def __init__(self, stat):
        one = lambda x: torch.tensor([x], dtype=torch.float32, device=DEV)
        self.stat = one(stat)
        self.t = dict(log_p=one(-1.2), exp_avg=one(0.01), exp_avg_sq=one(4e-4), step=one(0.0), value=one(0.0))
        t = self.t
        self.desc = _lib.rrl_dual_t(p(t["log_p"]), p(t["exp_avg"]), p(t["exp_avg_sq"]), p(t["step"]), p(t["value"]),
                                    p(self.stat), 0.3, 1e-3, None, None, 0.0)

    def state(self):
        return self.t


def launch(on, segs, betas=BETAS, dual=None):
    lib, arr = _lib.load(), (_lib.rrl_adam_seg_t * len(segs))(*[s.seg for s in segs])
    with memo(on):
        if dual is None:
            rc = lib.rrl_adam_step_multi(len(segs), arr, LR, betas[0], betas[1], ADAM_EPS, _lib.current_stream())
        else:
            darr = (_lib.rrl_dual_t * 1)(dual.desc)
            rc = lib.rrl_adam_step_multi_duals(len(segs), arr, 1, darr, LR, betas[0], betas[1], ADAM_EPS, _lib.current_stream())
    _lib.check(rc, "rrl_adam_step_multi")


def same(a, b, where):
    torch.cuda.synchronize()
    for x, y in zip(a, b):
        sx, sy = x.state(), y.state()
        assert sx.keys() == sy.keys()
        for name in sx:
            assert torch.equal(sx[name], sy[name]), (where, name)


def both(make):
    """The memo side (step counters from the pool) and the off-switch side (counters of its own) of one list of segments."""
    off = torch.zeros(16, 2, dtype=torch.int64, device=DEV)
    return make(counters), make(lambda k: off[k])


def steps(a, b, n, where, betas=BETAS, dual=None):
    for i in range(n):
        launch(True, a, betas, dual and dual[0])
        launch(False, b, betas, dual and dual[1])
        same(a + ([dual[0]] if dual else []), b + ([dual[1]] if dual else []), "%s, step %d" % (where, i))


SHAPES = {
    "one float4": lambda c: [Seg(4, c(0))],
    "scalar tail": lambda c: [Seg(1023, c(0), seed=2)],                                  # 255 float4, then three floats
    # 320 float4 of partial sums: workgroup 0 and the first wave of workgroup 1
    "partials": lambda c: [Seg(1280 + 4096, c(0), seed=3, parts=(16, 1280))],
    "twin heads": lambda c: [Seg(2 * W2 + 2048, c(0), seed=4, target=True, w2=(1024, 2))],
    "g2": lambda c: [Seg(4100, c(0), seed=5, g2=True, wd=1e-2)],
    "two segments": lambda c: [Seg(1023, c(0), seed=6, target=True), Seg(70000, c(1), seed=7, parts=(3, 516))],
}


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_eight_steps_with_the_memo_are_the_steps_without(shape):
    a, b = both(SHAPES[shape])
    steps(a, b, 8, shape)
    assert all(s.step.tolist() == [8, 0] for s in a)                      # advanced once per launch, the ticket back at 0


def test_eight_steps_of_the_dual_row_launch():
    a, b = both(lambda c: [Seg(1280 + 4096, c(0), seed=8, parts=(16, 1280), target=True)])
    duals = (Dual(0.4), Dual(0.4))
    steps(a, b, 8, "dual row", dual=duals)
    assert a[0].step.tolist() == [8, 0] and duals[0].t["step"].item() == 8.0


def test_a_step_counter_set_from_the_host_misses_and_is_picked_up_again():
    a, b = both(lambda c: [Seg(1280 + 4096, c(0), seed=9, parts=(16, 1280), target=True)])
    steps(a, b, 3, "from 0")
    for t in (1000, 7):
        for side in (a, b):
            side[0].step.copy_(torch.tensor([t, 0]))
        steps(a, b, 3, "from %d" % t)
        assert a[0].step.tolist() == [t + 3, 0]


def test_other_betas_miss():
    a, b = both(lambda c: [Seg(4100, c(0), seed=10)])
    steps(a, b, 2, "default betas")
    steps(a, b, 1, "other betas", betas=(0.8, 0.9))                       # the entry is there for this t, under another tag
    steps(a, b, 2, "default betas again")
    steps(a, b, 3, "other betas for good", betas=(0.8, 0.9))


def test_counters_one_apart_in_one_launch():
    """Segment 1 reads the parity that segment 0's writer fills (in its own slot)."""
    a, b = both(lambda c: [Seg(1023, c(0), t0=5, seed=11), Seg(4100, c(1), t0=6, seed=12)])
    steps(a, b, 4, "one apart")
    assert [s.step.tolist() for s in a] == [[9, 0], [10, 0]]


def test_beta1_power_underflows():
    a, b = both(lambda c: [Seg(1023, c(0), t0=200000, seed=13, target=True)])
    steps(a, b, 3, "t = 200000")


def test_captured_launches_replay_like_eager_ones_without_the_memo():
    a, b = both(lambda c: [Seg(1280 + 4096, c(0), seed=14, parts=(16, 1280), target=True)])
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(4):
            launch(True, a)
    assert a[0].step.tolist() == [0, 0]                                   # the capture executed nothing
    for turn in range(3):
        g.replay()
        for _ in range(4):
            launch(False, b)
        same(a, b, "replay %d" % turn)
    assert a[0].step.tolist() == [12, 0]


def test_more_step_counters_than_memo_slots():
    """300 segments on 300 step counters, twelve to a launch, two steps each: those that find the map full take pow().  (Last
    in this file: no slot is left afterwards.)"""
    n_seg = 300
    step_a, step_b = (torch.zeros(n_seg, 2, dtype=torch.int64, device=DEV) for _ in range(2))
    a = [Seg(4 + 4 * (k % 3), step_a[k], t0=k, seed=100 + k) for k in range(n_seg)]
    b = [Seg(4 + 4 * (k % 3), step_b[k], t0=k, seed=100 + k) for k in range(n_seg)]
    for i in range(2):
        for k in range(0, n_seg, _lib.ADAM_MAX_SEGS):
            launch(True, a[k:k + _lib.ADAM_MAX_SEGS])
            launch(False, b[k:k + _lib.ADAM_MAX_SEGS])
        same(a, b, "step %d" % i)
    assert step_a[:, 0].tolist() == [k + 2 for k in range(n_seg)]
