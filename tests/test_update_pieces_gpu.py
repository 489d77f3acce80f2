"""Every element-wise entry point of the updates alone, through its descriptor, against the float64 restatements of
oracle/update_oracle.py at the edges of its formulas and of its loops (clamp bounds, saturated tanh / sigmoid, ties, masked
targets, ragged rows, second passes, unaligned and ragged Adam segments, more than 16 gradient partials).

Tolerance, per quantity and pooled over all shapes of a test (test_sqrl_act_gpu.py's rule): the kernel's largest error
against float64 is at most twice that of the f32 module path (the torch modules, autograd and torch.optim.Adam on the same
device and inputs) and at most 1e-4 of the tensor's scale.  One line per quantity is printed; DESIGN.md section 5 records
them.  Whatever the header states as exact -- gates, ties, sentinels, copies, partials against pre-summed tensors, the fused
forms against the stand-alone ones -- is torch.equal."""
import ctypes as C
import functools
import itertools

import pytest
import torch

import update_pieces as UP
from oracle import update_oracle as O
from recovery_rl_amd import _lib
from recovery_rl_amd.fast_update import heads_multi, loss_dout

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENT = 7.0
ALPHA, GAMMA, GAMMA_SAFE, NU = 0.2, 0.99, 0.65, 3.5
p = _lib.ptr


def dev(x):
    return None if x is None else x.to(DEV).contiguous()


def full(*shape):
    return torch.full(shape, SENT, dtype=torch.float32, device=DEV)


@functools.lru_cache(maxsize=None)
def consts():
    return dev(torch.tensor(UP.SCALE)), dev(torch.tensor(UP.BIAS)), dev(torch.tensor([ALPHA]))


class Pool:
    """Largest error against float64 per quantity: [kernel, module path, scale]."""

    def __init__(self):
        self.worst = {}

    def add(self, name, ker, mod, want, where=""):
        ek, scale = UP.scaled_err(ker, want)
        em, _ = UP.scaled_err(mod, want)
        w = self.worst.setdefault(name, [0.0, 0.0, 0.0, ""])
        self.worst[name] = [max(w[0], ek), max(w[1], em), max(w[2], scale), where if ek > w[0] else w[3]]

    def check(self, factors=None):
        for name, (ker, mod, scale, where) in self.worst.items():
            print("%s: largest error against float64: kernel %.3e, module path %.3e (scale %.3e)%s"
                  % (name, ker, mod, scale, where and " at " + where))
        for name, (ker, mod, scale, _) in self.worst.items():
            assert ker <= (factors or {}).get(name, 2) * mod, (name, ker, mod)
            assert ker <= 1e-4 * scale, (name, ker, scale)


# ---- a. rrl_policy_heads_fwd_multi ------------------------------------------------------------------------------------------------
def head_desc(kind, B, head, eps, action, ld, logp=None, mean_out=None, obs_in=None, obs_out=None, log_std=None, n_part=1,
              stride=0):
    scale, bias, _ = consts()
    return _lib.rrl_policy_head_t(kind, B, p(head), n_part, stride, p(eps), p(scale), p(bias), p(action), ld, p(logp),
                                  p(mean_out), p(obs_in), p(obs_out), p(log_std), UP.MIN_LOG_STD)


def run_head(kind, B, head, eps, ld, log_std=None, obs=None, want_logp=True, want_mean=True, n_part=1, stride=0):
    """One lone head launch into sentinel-filled buffers -> (row buffer [B,ld], logp [B], mean_out [B,2])."""
    buf, logp, mean = full(B, ld), full(B), full(B, 2)
    action = buf if ld == 2 else buf[:, 2:]
    heads_multi([head_desc(kind, B, head, eps, action, ld, logp if want_logp else None, mean if want_mean else None,
                           obs, buf if obs is not None else None, log_std, n_part, stride)])
    torch.cuda.synchronize()
    return buf, logp, mean


def test_gauss_head_forward_against_float64():
    pool = Pool()
    scale, bias, _ = consts()
    for B in UP.BATCHES:
        rows = UP.gauss_rows(B)
        head, eps = dev(rows["head"]), dev(rows["eps"])
        o_act, o_logp, o_mean = O.gauss_head(rows["head"], rows["eps"], scale, bias)
        m_act, m_logp, m_mean = UP.module_gauss(head, eps)
        obs = torch.randn(B, 2, device=DEV)
        got = {}
        for ld, with_obs in ((2, False), (4, False), (4, True)):
            buf, logp, mean = got[ld, with_obs] = run_head(_lib.HEAD_GAUSS, B, head, eps, ld, obs=obs if with_obs else None)
            act = buf if ld == 2 else buf[:, 2:]
            pool.add("gauss action", act, m_act, o_act)
            pool.add("gauss logp", logp, m_logp, o_logp)
            pool.add("gauss mean_out", mean, m_mean, o_mean)
            if ld == 4:         # columns 0..1: the observation bit for bit, or untouched
                assert torch.equal(buf[:, 0:2], obs if with_obs else torch.full_like(obs, SENT))
        for key in ((4, False), (4, True)):     # the row stride changes where the action lands, nothing else
            assert torch.equal(got[key][0][:, 2:], got[2, False][0]) and torch.equal(got[key][1], got[2, False][1])
        buf, logp, mean = run_head(_lib.HEAD_GAUSS, B, head, eps, 2, want_logp=False, want_mean=False)
        assert torch.equal(buf, got[2, False][0]) and bool((logp == SENT).all()) and bool((mean == SENT).all())
        sat = rows["cls"] == 4
        if bool(sat.any()):         # a saturated tanh is +-1: the action sits on the box's edge
            edge = torch.sign(dev(rows["pre"][sat]).float()) * scale + bias
            assert torch.equal(got[2, False][0][dev(sat)], edge)
    pool.check()


def test_stoch_head_forward_against_float64():
    pool = Pool()
    scale, bias, _ = consts()
    for B in UP.BATCHES:
        rows = UP.stoch_rows(B)
        raw, eps = dev(rows["raw"]), dev(rows["eps"])
        for which, ls in sorted(UP.stoch_log_stds().items()):
            log_std = dev(torch.tensor(ls, dtype=torch.float32))
            for ld, noise in ((2, True), (4, True), (2, False)):
                e = eps if noise else None
                o_act, _, o_mean = O.stoch_head(rows["raw"], rows["eps"] if noise else None, log_std, UP.MIN_LOG_STD, scale, bias)
                m_act, m_mean = UP.module_stoch(raw, e, log_std)
                buf, logp, mean = run_head(_lib.HEAD_STOCH, B, raw, e, ld, log_std=log_std)
                act = buf if ld == 2 else buf[:, 2:]
                pool.add("stoch action", act, m_act, o_act)
                pool.add("stoch mean_out", mean, m_mean, o_mean)
                assert bool((logp == SENT).all())                       # the stochastic head has no log-probability
                if ld == 4:
                    assert bool((buf[:, 0:2] == SENT).all())            # ... and copies no observation
                if not noise:
                    assert torch.equal(act, mean)                       # eps = NULL: action = mean
            if which == "below":    # both dims below the floor: the noise has the floor's std, whatever log_std says
                lower = dev(torch.tensor([UP.MIN_LOG_STD - 9.0, UP.MIN_LOG_STD - 0.5], dtype=torch.float32))
                assert torch.equal(run_head(_lib.HEAD_STOCH, B, raw, eps, 2, log_std=lower)[0],
                                   run_head(_lib.HEAD_STOCH, B, raw, eps, 2, log_std=log_std)[0])
    pool.check()


@pytest.mark.parametrize("n_part", (1, 2, 4))
def test_heads_on_partial_sums_equal_the_heads_on_the_summed_tensor(n_part):
    B = 257
    g = torch.Generator(device=DEV).manual_seed(11)
    eps = torch.randn(B, 2, device=DEV, generator=g)
    for kind, width, log_std in ((_lib.HEAD_GAUSS, 4, None), (_lib.HEAD_STOCH, 2, dev(torch.tensor([-1.0, -2.0])))):
        parts = torch.randn(4, B, width, device=DEV, generator=g) * 0.7
        summed = O.fixed_order_sum(parts[:n_part]).contiguous()
        a = run_head(kind, B, parts, eps, 2, log_std=log_std, n_part=n_part, stride=parts.stride(0))
        b = run_head(kind, B, summed, eps, 2, log_std=log_std)
        assert all(torch.equal(x, y) for x, y in zip(a, b))
        if n_part > 1:
            assert not torch.equal(a[0], run_head(kind, B, parts, eps, 2, log_std=log_std)[0])


def test_four_mixed_heads_of_different_sizes_in_one_launch():
    scale, bias, _ = consts()
    members = ((_lib.HEAD_GAUSS, 600), (_lib.HEAD_STOCH, 17), (_lib.HEAD_GAUSS, 1), (_lib.HEAD_STOCH, 257))
    log_std = dev(torch.tensor(UP.stoch_log_stds()["mixed"], dtype=torch.float32))
    descs, outs, want, lone = [], [], [], []
    for kind, B in members:
        rows = UP.gauss_rows(B) if kind == _lib.HEAD_GAUSS else UP.stoch_rows(B)
        head, eps = dev(rows["head" if kind == _lib.HEAD_GAUSS else "raw"]), dev(rows["eps"])
        act, logp, mean = full(B, 2), full(B), full(B, 2)
        descs.append(head_desc(kind, B, head, eps, act, 2, logp, mean, log_std=log_std))
        outs.append((act, logp, mean, head, eps))
        want.append(O.gauss_head(head, eps, scale, bias) if kind == _lib.HEAD_GAUSS else
                    O.stoch_head(head, eps, log_std, UP.MIN_LOG_STD, scale, bias))
        lone.append(run_head(kind, B, head, eps, 2, log_std=log_std))
    heads_multi(descs)
    torch.cuda.synchronize()
    for (kind, B), (act, logp, mean, _, _), (o_act, o_logp, o_mean), alone in zip(members, outs, want, lone):
        for got, ref in ((act, o_act), (mean, o_mean)) + (((logp, o_logp),) if kind == _lib.HEAD_GAUSS else ()):
            err, sc = UP.scaled_err(got, ref)
            assert err <= 1e-4 * sc, (kind, B, err, sc)
        assert torch.equal(act, alone[0]) and torch.equal(logp, alone[1]) and torch.equal(mean, alone[2])


# ---- b - d. the seven loss kinds: stand-alone, inside the head backward, inside the paired launch -----------------------------------
LABEL = {_lib.LOSS_SAC_CRITIC: "sac critic", _lib.LOSS_SAC_POLICY: "sac policy", _lib.LOSS_QRISK_CRITIC: "qrisk critic",
         _lib.LOSS_QRISK_POLICY: "qrisk policy", _lib.LOSS_DGD_QRISK: "dgd qrisk", _lib.LOSS_GAUSS_HEAD: "gauss head",
         _lib.LOSS_STOCH_HEAD: "stoch head"}
KINDS = ("sac_critic", "sac_critic_penalty", "sac_policy", "qrisk_critic", "qrisk_policy", "dgd_qrisk",
         "gauss_head_1", "gauss_head_2", "stoch_above_1", "stoch_at_2", "stoch_below_2", "stoch_mixed_1")
CRITIC_KINDS = KINDS[:6]


class Case:
    """One loss kind on one batch: device operands, the descriptor, the float64 answer and the f32 module path's."""

    def __init__(self, name, B):
        self.name, self.B = name, B
        scale, bias, alpha = self.consts = consts()
        self.n_loss = 2
        self.da_dev = None
        if name.startswith("sac") or name.startswith("qrisk") or name.startswith("dgd"):
            self.G, self.dout = 2, 1
            r = UP.critic_rows(B, wide=not name.startswith("sac"))
            self.rows = r
            t = self.t = {k: dev(v) for k, v in r.items() if k != "cls"}
            if name.startswith("sac_critic"):
                pen, pen_d = (r["penalty"], t["penalty"]) if name.endswith("penalty") else (None, None)
                self.kind = _lib.LOSS_SAC_CRITIC
                self.fields = dict(out=t["a"], out_t=t["at"], v0=t["logp2"], v1=t["r"], v2=t["m"], v3=pen_d, alpha=alpha, f0=GAMMA)
                self.oracle = O.sac_critic(r["a"], r["at"], r["logp2"], r["r"], r["m"], ALPHA, GAMMA, pen)
                self.module = UP.module_sac_critic(t["a"], t["at"], t["logp2"], t["r"], t["m"], alpha, GAMMA, pen_d)
            elif name == "sac_policy":
                self.kind, self.n_loss = _lib.LOSS_SAC_POLICY, 1
                self.fields = dict(out=t["a"], v0=t["logp"], alpha=alpha)
                self.oracle = O.sac_policy(r["a"], r["logp"], ALPHA)
                self.module = UP.module_sac_policy(t["a"], t["logp"], alpha)
            elif name == "qrisk_critic":
                self.kind = _lib.LOSS_QRISK_CRITIC
                self.fields = dict(out=t["a"], out_t=t["at"], v0=t["c"], v1=t["m"], f0=GAMMA_SAFE)
                self.oracle = O.qrisk_critic(r["a"], r["at"], r["c"], r["m"], GAMMA_SAFE)
                self.module = UP.module_qrisk_critic(t["a"], t["at"], t["c"], t["m"], GAMMA_SAFE)
            else:
                nu = NU if name == "dgd_qrisk" else None
                self.kind, self.n_loss = (_lib.LOSS_DGD_QRISK if nu else _lib.LOSS_QRISK_POLICY), 1
                self.fields = dict(out=t["a"], f0=NU if nu else 0.0)
                self.oracle = O.dgd_qrisk(r["a"], NU) if nu else O.qrisk_policy(r["a"])
                self.module = UP.module_qrisk_policy(t["a"], nu)
            self.module = (self.module[0].unsqueeze(-1), self.module[1])
            return
        self.G, n_heads = 1, int(name[-1])
        ld = 2 if n_heads == 1 else 4
        da = UP.d_action(B, n_heads, ld)                       # [n_heads, B, ld]; ld = 4: the action's gradient in columns 2..3
        self.da_dev = dev(da)
        act = da[..., ld - 2:]
        self.da_sum = O.fixed_order_sum(act)                   # f32, head by head
        self.da_view = self.da_dev[0, :, ld - 2:]
        self.head_fields = dict(ld=ld, n_heads=n_heads, head_stride=self.da_dev.stride(0), d_action=self.da_view)
        da_sum_d = dev(self.da_sum)
        if name.startswith("gauss"):
            self.kind, self.dout, self.n_loss = _lib.LOSS_GAUSS_HEAD, 4, 0
            r = self.rows = UP.gauss_rows(B)
            head, eps = dev(r["head"]), dev(r["eps"])
            self.dlogp = ALPHA / B
            self.fields = dict(out=head, v0=eps, v1=scale, f0=self.dlogp, **self.head_fields)
            self.oracle = O.gauss_head_bwd(r["head"], r["eps"], scale, self.da_sum, self.dlogp)
            self.module = (UP.module_gauss(head, eps, da_sum_d, self.dlogp)[3].unsqueeze(0), torch.zeros(0))
        else:
            self.kind, self.dout = _lib.LOSS_STOCH_HEAD, 2
            r = self.rows = UP.stoch_rows(B)
            raw, eps = dev(r["raw"]), dev(r["eps"])
            self.log_std = torch.tensor(UP.stoch_log_stds()[name.split("_")[1]], dtype=torch.float32)
            ls = dev(self.log_std)
            self.fields = dict(out=raw, v0=eps, v1=ls, v2=scale, f0=UP.MIN_LOG_STD, **self.head_fields)
            self.oracle = O.stoch_head_bwd(r["raw"], r["eps"], self.log_std, UP.MIN_LOG_STD, scale, self.da_sum)
            m = UP.module_stoch(raw, eps, ls, da_sum_d)
            self.module = (m[2].unsqueeze(0), m[3])

    def loss(self, loss_buf, **over):
        f = dict(n_part=1, part_stride=0, out_t=None, v0=None, v1=None, v2=None, v3=None, alpha=None, f0=0.0, ld=0, n_heads=0,
                 head_stride=0, d_action=None, da_parts=0, da_part_stride=0, da_group=0)
        f.update(self.fields)
        f.update(over)
        self.keep = f
        return _lib.rrl_loss_t(self.kind, f["n_part"], f["part_stride"], p(f["out"]), p(f["out_t"]), p(f["v0"]), p(f["v1"]),
                               p(f["v2"]), p(f["v3"]), p(f["alpha"]), f["f0"], f["ld"], f["n_heads"], f["head_stride"],
                               p(f["d_action"]), p(loss_buf), f["da_parts"], f["da_part_stride"], f["da_group"])

    def alone(self, **over):
        """rrl_loss_dout -> dOut [G,B,dout], loss[2] (sentinels where the kind writes none)."""
        dout, loss = full(self.G, self.B, self.dout), full(2)
        loss_dout(self.loss(loss, **over), self.B, dout)
        torch.cuda.synchronize()
        return dout, loss

    def pool(self, pool, what, dout, loss):
        kind = LABEL[self.kind]
        where = "%s, B = %d" % (self.name, self.B)
        pool.add("%s %s dOut" % (what, kind), dout, self.module[0], self.oracle[0], where)
        if self.n_loss:
            pool.add("%s %s loss" % (what, kind), loss[:self.n_loss], self.module[1], self.oracle[1], where)
        assert bool((loss[self.n_loss:] == SENT).all())

    def exact(self, dout):
        """What the header states exactly, whichever launch produced dOut [G,B,dout]."""
        B, name = self.B, self.name
        if B < 6:
            return
        if name.startswith("gauss"):
            cls, ds = dev(self.rows["cls"]), dout[0][:, 2:4]
            assert bool((ds[cls == 3] == 0.0).all())                            # raw outside the clamp: no gradient
            assert bool((ds[(cls == 1) | (cls == 2)] != 0.0).all())             # at a bound: it passes
            # a saturated row: tanh' = 0, so nothing reaches the mean and only -dlogp the log-std
            assert bool((dout[0][cls == 4][:, 0:2] == 0.0).all())
            assert torch.equal(ds[cls == 4], torch.full_like(ds[cls == 4], -self.dlogp))
        elif name.startswith("stoch"):
            sat = (dev(self.rows["raw"]).abs() == 25.0)
            assert bool((dout[0][sat] == 0.0).all())
        else:
            tie = dev(self.rows["cls"] == 3)
            if name == "sac_policy":            # min splits a tie: -0.5 / B on both heads
                assert torch.equal(dout[:, tie, 0], torch.full_like(dout[:, tie, 0], -0.5 / B))
                assert bool(((dout[:, ~tie, 0] == 0.0) | (dout[:, ~tie, 0] == -1.0 / B)).all())
            if name in ("qrisk_policy", "dgd_qrisk"):   # max splits a tie: 0.5 / B q (1 - q) on both heads, q the same
                assert torch.equal(dout[0, tie], dout[1, tie]) and bool((dout[0, tie] > 0).all())
                q, s = torch.sigmoid(self.t["a"][0, tie].double()), (NU if name == "dgd_qrisk" else 1.0)
                # f32 rounds q to 6e-8, and q (1 - q) <= 1/4: the product is within 1e-5 of that scale with room to spare
                assert float((dout[0, tie, 0].double() - s * 0.5 / B * q * (1 - q)).abs().max()) <= 1e-5 * s * 0.125 / B


def test_loss_dout_of_every_kind_against_float64():
    pool = Pool()
    for B in UP.BATCHES:
        for name in KINDS:
            c = Case(name, B)
            dout, loss = c.alone()
            c.pool(pool, "alone", dout, loss)
            c.exact(dout)
            if name.startswith("stoch"):
                below = dev(c.log_std < torch.tensor(UP.MIN_LOG_STD, dtype=torch.float32))
                assert bool((loss[below] == 0.0).all()) and (B < 6 or bool((loss[~below] != 0.0).all()))
            if name == "qrisk_policy":          # DGD with nu = 1 is QRISK_POLICY, bit for bit
                c.kind = _lib.LOSS_DGD_QRISK
                one = c.alone(f0=1.0)
                c.kind = _lib.LOSS_QRISK_POLICY
                assert torch.equal(one[0], dout) and torch.equal(one[1], loss)
    pool.check()


@pytest.mark.parametrize("n_part", (2, 4))
def test_loss_dout_on_partial_sums_equals_the_summed_operands(n_part):
    B = 257
    for name in ("sac_critic_penalty", "qrisk_critic", "sac_policy", "dgd_qrisk", "gauss_head_1", "stoch_above_1"):
        c = Case(name, B)
        g = torch.Generator(device=DEV).manual_seed(5)
        out = c.fields["out"]
        parts = torch.randn(4, *out.shape, device=DEV, generator=g)
        over = dict(n_part=n_part, part_stride=parts.stride(0), out=parts)
        summed = dict(out=O.fixed_order_sum(parts[:n_part]).contiguous())
        if "out_t" in c.fields:
            parts_t = torch.randn(4, *out.shape, device=DEV, generator=g)
            over["out_t"], summed["out_t"] = parts_t, O.fixed_order_sum(parts_t[:n_part]).contiguous()
        a, b = c.alone(**over), c.alone(**summed)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), name


def head_backward(c, H=16, **over):
    """rrl_mlp_head_backward_multi on a stack whose last layer makes dOut observable: h2 = 1 and W3 = 1 (one output) or the
    identity's first rows (dh2[b, o] = dOut[b, o]); dW3 and db3 then carry the batch sums.  -> dh2, dW3, db3, loss."""
    G, B, dout = c.G, c.B, c.dout
    h2 = torch.ones(G, B, H, device=DEV)
    W3 = torch.ones(G, 1, H, device=DEV) if dout == 1 else torch.eye(H, device=DEV)[:dout].unsqueeze(0).contiguous()
    dW3, db3, dh2, loss = full(G, dout, H), full(G, dout), full(G, B, H), full(2)
    desc = _lib.rrl_head_bwd_t(c.loss(loss, **over), G, B, H, dout, p(h2), p(W3), p(dW3), p(db3), p(dh2))
    _lib.check(_lib.load().rrl_mlp_head_backward_multi(1, C.byref(desc), _lib.current_stream()), "rrl_mlp_head_backward_multi")
    torch.cuda.synchronize()
    return dh2, dW3, db3, loss


# Quantities whose kernel error is more than twice the module path's, with the cause and the measured ratio rounded up to the
# next integer (DESIGN.md section 5 has the figures).  All of them are sums over the batch, and the cause is the order of the
# additions: the head backward adds a thread's rows (256 apart) first, then DPP sums inside the 16-lane rows, then the 16 row
# sums one after the other, and dW3 is an fmaf chain over the B / 8 rows of a slice followed by the 8 slice sums; torch's
# mean / sum is a pairwise tree.  The stand-alone kernels' 8-step tree stays inside the factor 2.  Every one is a single
# number (or one per output), a few roundings of 6e-8 of the scale each: 2.5 against 1 rounding, not a formula.
FUSED_FACTORS = {"fused sac policy loss": 3,        # 1.871e-07 against 7.549e-08: 2.48
                 "fused qrisk policy loss": 3,      # 1.122e-07 against 5.264e-08: 2.13
                 "fused dgd qrisk loss": 3,         # the same launch body and operands: 2.13
                 "fused stoch dW3": 3}              # 5.189e-06 against 1.814e-06: 2.86
PAIRED_FACTORS = {"paired sac policy loss": 3}      # 1.871e-07 against 8.671e-08: 2.16


def test_loss_kinds_inside_the_head_backward_against_float64_and_the_stand_alone_launch():
    pool = Pool()
    for B in UP.BATCHES:
        for name in KINDS:
            c = Case(name, B)
            dh2, dW3, db3, loss = head_backward(c)
            dout = dh2[..., :c.dout].contiguous()
            alone, _ = c.alone()
            assert torch.equal(dout, alone), (name, B)                        # the stand-alone launch's dOut, bit for bit
            if c.dout == 1:
                assert torch.equal(dh2, dout.expand_as(dh2))
            else:
                assert bool((dh2[..., c.dout:] == 0.0).all())
            c.pool(pool, "fused", dout, loss)
            c.exact(dout)
            sums, m_sums = c.oracle[0].sum(1), c.module[0].sum(1)             # [G, dout]
            kind = "critic" if c.dout == 1 else name.split("_")[0]
            where = "%s, B = %d" % (name, B)
            pool.add("fused %s db3" % kind, db3, m_sums, sums, where)
            pool.add("fused %s dW3" % kind, dW3, m_sums.unsqueeze(-1).expand_as(dW3), sums.unsqueeze(-1).expand_as(dW3), where)
    pool.check(FUSED_FACTORS)


@pytest.mark.parametrize("da_parts,da_group", ((4, 1), (16, 4)))
@pytest.mark.parametrize("name", ("gauss_head_1", "gauss_head_2", "stoch_above_1", "stoch_at_2"))
def test_head_backward_on_d_action_partials_equals_the_presummed_tensor(name, da_parts, da_group):
    """One critic head: random partials, so the documented order is what makes the bits equal.  Two heads: the kernel adds
    head 1's partials on top of head 0's running sum, so the partials are multiples of 1/8 (every order gives the same sum)."""
    for B in (17, 600):
        c = Case(name, B)
        n_heads, ld = c.head_fields["n_heads"], c.head_fields["ld"]
        g = torch.Generator(device=DEV).manual_seed(da_parts)
        if n_heads == 1:
            parts = torch.randn(da_parts, n_heads, B, ld, device=DEV, generator=g)
        else:
            parts = torch.randint(-8, 9, (da_parts, n_heads, B, ld), device=DEV, generator=g).float() / 8.0
        summed = O.fixed_order_sum(parts, da_group).contiguous()
        a = head_backward(c, d_action=parts[0, 0, :, ld - 2:], head_stride=parts.stride(1), da_parts=da_parts,
                          da_part_stride=parts.stride(0), da_group=da_group)
        b = head_backward(c, d_action=summed[0, :, ld - 2:], head_stride=summed.stride(0))
        assert all(torch.equal(x, y) for x, y in zip(a, b)), (name, B)
        assert not torch.equal(a[0], head_backward(c)[0])


def test_critic_loss_kinds_inside_the_paired_launch_against_float64_and_the_stand_alone_launch():
    """rrl_mlp_backward_pair_multi, one launch, at (B, H) = (128, 128) and (256, 256): h2 = 1, W3 = 1 and h1 = I make
    dW2[g] = dh2[g]^T, every row of it the dOut the tiles derived themselves; db2 is its batch sum; dh2 itself is not written."""
    pool = Pool()
    lib = _lib.load()
    for B, name in itertools.product((128, 256), CRITIC_KINDS):
        H = B
        c = Case(name, B)
        h2, W3 = torch.ones(2, B, H, device=DEV), torch.ones(2, 1, H, device=DEV)
        h1 = torch.eye(H, device=DEV).unsqueeze(0).repeat(2, 1, 1)
        W2 = torch.ones(2, H, H, device=DEV)
        dW3, db3, dh2, loss = full(2, 1, H), full(2, 1), full(2, B, H), full(2)
        dW2, db2, dh1 = full(2, H, H), full(2, H), full(2, B, H)
        head = _lib.rrl_head_bwd_t(c.loss(loss), 2, B, H, 1, p(h2), p(W3), p(dW3), p(db3), p(dh2))
        hidden = _lib.rrl_hidden_bwd_t(2, B, H, p(dh2), p(h1), p(W2), p(dW2), p(db2), p(dh1), _lib.rrl_first_layer_t())
        _lib.check(lib.rrl_mlp_backward_pair_multi(1, C.byref(head), C.byref(hidden), _lib.current_stream()),
                   "rrl_mlp_backward_pair_multi")
        torch.cuda.synchronize()
        assert bool((dh2 == SENT).all())                                       # one launch: the link is not written
        dout = dW2[:, 0, :].unsqueeze(-1).contiguous()                         # [2, B, 1]
        assert torch.equal(dW2, dout.transpose(1, 2).expand_as(dW2))
        alone, _ = c.alone()
        assert torch.equal(dout, alone), name
        c.pool(pool, "paired", dout, loss)
        c.exact(dout)
        sums, m_sums = c.oracle[0].sum(1), c.module[0].sum(1)
        where = "%s, B = %d" % (name, B)
        pool.add("paired db2", db2, m_sums.expand_as(db2), sums.expand_as(db2), where)
        pool.add("paired db3", db3, m_sums, sums, where)
        pool.add("paired dW3", dW3, m_sums.unsqueeze(-1).expand_as(dW3), sums.unsqueeze(-1).expand_as(dW3), where)
    pool.check(PAIRED_FACTORS)


# ---- e. rrl_rcpo_penalty and rrl_recovery_select -------------------------------------------------------------------------------
def penalty(B, z, lam, want_penalty=True, n_part=1, stride=0):
    pen, mean = full(B), full(1)
    args = _lib.rrl_penalty_args_t(B, p(z), n_part, stride, p(lam), p(pen) if want_penalty else None, p(mean))
    _lib.check(_lib.load().rrl_rcpo_penalty(C.byref(args), _lib.current_stream()), "rrl_rcpo_penalty")
    torch.cuda.synchronize()
    return pen, mean


def test_rcpo_penalty_against_float64():
    pool = Pool()
    lam = dev(torch.tensor([0.7]))
    for B in UP.BATCHES:
        z = UP.critic_rows(B)["a"]
        zd = dev(z)
        o_pen, o_mean = O.rcpo_penalty(z, float(lam))
        m_q = torch.max(torch.sigmoid(zd[0]), torch.sigmoid(zd[1]))
        pen, mean = penalty(B, zd, lam)
        pool.add("penalty", pen, lam * m_q, o_pen)
        pool.add("penalty mean", mean, m_q.mean().reshape(1), o_mean.reshape(1))
        only_pen, only_mean = penalty(B, zd, None, want_penalty=False)        # the mean alone: lambda is not read
        assert bool((only_pen == SENT).all()) and torch.equal(only_mean, mean)
        lam2 = dev(torch.tensor([0.7]))
        first = penalty(B, zd, lam2)[0]
        lam2.fill_(1.9)                                                       # lambda lives on the device: the next launch sees it
        second = penalty(B, zd, lam2)[0]
        assert torch.equal(first, pen) and not torch.equal(second, first)
        pool.add("penalty", second, 1.9 * m_q, O.rcpo_penalty(z, float(lam2))[0])
        parts = torch.randn(4, 2, B, device=DEV, generator=torch.Generator(device=DEV).manual_seed(B))
        a = penalty(B, parts, lam, n_part=4, stride=parts.stride(0))
        b = penalty(B, O.fixed_order_sum(parts).contiguous(), lam)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    pool.check()


@pytest.mark.parametrize("eps_safe", (0.0, 0.3, 1.0))
def test_recovery_select_decides_as_float64_does(eps_safe):
    lib = _lib.load()
    for N in UP.BATCHES:
        r = UP.select_rows(N)
        z, task, rec = dev(r["z"]), dev(r["task"]), dev(r["rec"])
        real, flag, task_out = full(N, 2), torch.full((N,), 9, dtype=torch.uint8, device=DEV), full(N, 2)
        _lib.check(lib.rrl_recovery_select(N, p(z), eps_safe, p(task[:, 2:]), 4, p(rec), p(real), p(flag), p(task_out),
                                           _lib.current_stream()), "rrl_recovery_select")
        torch.cuda.synchronize()
        _, o_flag, _, risk = O.recovery_select(r["z"], eps_safe, r["task"][:, 2:], r["rec"])
        decided = (risk - eps_safe).abs() > 1e-6            # float64 risk within 1e-6 of the threshold: either answer
        exempt = int((~decided).sum())
        assert exempt <= 0.02 * N, (N, exempt)              # (test_update_pieces_cpu.py: the generator stays under it)
        print("N = %d, eps_safe = %g: %d of %d rows exempt" % (N, eps_safe, exempt, N))
        got = flag.cpu().bool()
        assert torch.equal(got[decided], o_flag[decided]) and bool((flag <= 1).all())
        sel = flag.bool().unsqueeze(1)
        assert torch.equal(real, torch.where(sel, rec, task[:, 2:])) and torch.equal(task_out, task[:, 2:])


# ---- f. rrl_adam_step_multi ---------------------------------------------------------------------------------------------------
BETAS, ADAM_EPS = UP.BETAS, UP.ADAM_EPS         # f32 numbers: what the entry point's float arguments carry


def shifted(x, off):
    """x on the device, `off` floats behind a 16-byte boundary."""
    if x is None:
        return None
    buf = torch.empty(x.numel() + 4, dtype=x.dtype, device=DEV)
    view = buf[off:off + x.numel()]
    view.copy_(x)
    assert view.data_ptr() % 16 == 4 * off
    return view


class Seg:
    """One Adam segment built from raw tensors, with its float64 answer and the f32 torch.optim.Adam path."""

    def __init__(self, n, t, lr, full_opts=False, off=0, parts=None, part_elems=0, seed=6):
        lr = UP.as_f32(lr)
        self.n, self.t, self.lr = n, t, lr
        s = self.host = UP.adam_state(n, seed)
        self.wd, self.tau = (UP.as_f32(1e-2), UP.as_f32(0.005)) if full_opts else (0.0, 0.0)
        g2, target = (s["g2"], s["target"]) if full_opts else (None, None)
        grad = s["g"]
        self.gp = None
        if parts is not None:           # [n_part, stride] small integers: the first part_elems gradients are their sum
            self.gp = dev(parts)
            grad = grad.clone()
            grad[:part_elems] = parts[:, :part_elems].double().sum(0).float()
            s["g"][:part_elems] = 1e3   # what the segment's g holds there is not read
        self.d = {k: shifted(s[k], off) for k in ("p", "g", "m", "v")}
        self.d["g2"], self.d["target"] = shifted(g2, off), shifted(target, off)
        self.step = torch.tensor([t, 0], dtype=torch.int64, device=DEV)
        self.want = O.adam_step(s["p"], grad, s["m"], s["v"], t, lr, BETAS, ADAM_EPS, self.wd, g2, target, self.tau)
        gd = dev(grad)
        self.module = UP.module_adam(dev(s["p"]), gd, dev(s["m"]), dev(s["v"]), t, lr, self.wd, dev(g2), dev(target), self.tau,
                                     BETAS, ADAM_EPS)
        d = self.d
        self.seg = _lib.rrl_adam_seg_t(n, p(d["p"]), p(d["g"]), p(d["m"]), p(d["v"]), p(self.step), p(d["target"]), self.tau,
                                       self.wd, p(d["g2"]), p(self.gp), 0 if parts is None else parts.shape[0],
                                       0 if parts is None else parts.shape[1], part_elems, None, None, 0, 0)

    def pool(self, pool):
        d, s = self.d, self.host
        assert self.step.tolist() == [self.t + 1, 0]                    # advanced by exactly one, the ticket back at 0
        where = "n = %d, t = %d, lr = %g" % (self.n, self.t, self.lr)
        pool.add("adam p", d["p"], self.module[0], self.want[0], where)
        pool.add("adam m", d["m"], self.module[1], self.want[1], where)
        pool.add("adam v", d["v"], self.module[2], self.want[2], where)
        p0 = s["p"].double()
        pool.add("adam update", d["p"].double().cpu() - p0, self.module[0].double().cpu() - p0, self.want[0] - p0, where)
        if self.want[3] is not None:
            pool.add("adam target", d["target"], self.module[3], self.want[3], where)


def adam_launch(segs, lr, duals=None):
    lib, arr = _lib.load(), (_lib.rrl_adam_seg_t * max(len(segs), 1))(*[s.seg for s in segs])
    if duals is None:
        _lib.check(lib.rrl_adam_step_multi(len(segs), arr, lr, BETAS[0], BETAS[1], ADAM_EPS, _lib.current_stream()),
                   "rrl_adam_step_multi")
    else:
        darr = (_lib.rrl_dual_t * len(duals))(*duals)
        _lib.check(lib.rrl_adam_step_multi_duals(len(segs), arr, len(duals), darr, lr, BETAS[0], BETAS[1], ADAM_EPS,
                                                 _lib.current_stream()), "rrl_adam_step_multi_duals")
    torch.cuda.synchronize()


ADAM_SIZES = (1, 3, 4, 5, 1023, 65540, 200004)      # 200 004: 50 001 float4 over 96 workgroups, some threads get a third slot


@pytest.mark.parametrize("n", ADAM_SIZES)
def test_adam_step_against_float64(n):
    """Step counts x learning rates, cycling through (plain | weight decay + g2 + Polyak target) x (aligned | one float off
    a 16-byte boundary: the scalar path): every size sees every variant twice."""
    pool = Pool()
    for i, (t, lr) in enumerate(itertools.product((0, 1, 999, 99999), (3e-4, 0.1))):
        variant = (3 * i + i // 4) % 4              # 0 3 2 1 1 0 3 2: each variant meets both learning rates and two step counts
        s = Seg(n, t, lr, full_opts=bool(variant & 1), off=variant >> 1, seed=6 + i)
        adam_launch([s], s.lr)
        s.pool(pool)
    pool.check()


@pytest.mark.parametrize("off", (0, 1))
@pytest.mark.parametrize("n_part", (1, 2, 16, 17, 33, 64))
def test_adam_gradient_partials_are_added_once_each(n_part, off):
    """g_part with n_part partials on the vector path (off = 0) and the scalar path (p, g, m, v one float off): part_elems
    below n (a ragged tail of plain gradients behind them) and equal to n.  The partials are small multiples of 1/64: their sum
    is exact in any order, so the oracle's gradient is unambiguous, and a partial added twice or left out moves m by 1e-3 or
    more of its scale."""
    pool = Pool()
    for n, pe in ((1030, 516), (1028, 1028), (65540, 65536)):
        stride = pe + 8
        parts = torch.randint(-3, 4, (n_part, stride), generator=torch.Generator().manual_seed(n_part)).float() / 64.0
        s = Seg(n, 999, 0.1, full_opts=(n == 1030), off=off, parts=parts, part_elems=pe)
        adam_launch([s], s.lr)
        s.pool(pool)
    pool.check()


def test_twelve_adam_segments_in_one_launch():
    pool = Pool()
    sizes = (1, 3, 4, 5, 1023, 65540, 200004, 17, 256, 4096, 1030, 2)
    parts = torch.randint(-3, 4, (17, 520), generator=torch.Generator().manual_seed(3)).float() / 64.0
    segs = [Seg(n, (0, 1, 999, 99999)[k % 4], 0.1, full_opts=bool(k & 1), off=(k >> 1) & 1, seed=20 + k,
                parts=parts if n == 1030 else None, part_elems=516 if n == 1030 else 0) for k, n in enumerate(sizes)]
    assert len(segs) == _lib.ADAM_MAX_SEGS
    adam_launch(segs, segs[0].lr)
    for s in segs:
        s.pool(pool)
    pool.check()


# ---- g. rrl_adam_step_multi_duals ------------------------------------------------------------------------------------------------
class Dual:
    def __init__(self, stat, eps_safe, lr, step, with_step=True, with_loss=True, log_p=-1.2, m=0.01, v=4e-4, loss_in=0.8,
                 f_loss=2.5):
        one = lambda x: torch.tensor([x], dtype=torch.float32, device=DEV)
        self.stat, self.eps_safe = stat, eps_safe                       # stat: a device tensor an earlier launch writes
        self.t = dict(log_p=one(log_p), exp_avg=one(m), exp_avg_sq=one(v), step=one(float(step)), value=full(1),
                      loss_in=one(loss_in), loss_out=full(1))
        t = self.t
        self.with_step, self.with_loss = with_step, with_loss
        self.args = (log_p, m, v, step, eps_safe, lr, loss_in, f_loss)
        self.desc = _lib.rrl_dual_t(p(t["log_p"]) if with_step else None, p(t["exp_avg"]), p(t["exp_avg_sq"]), p(t["step"]),
                                    p(t["value"]), p(stat), eps_safe, lr, p(t["loss_in"]) if with_loss else None,
                                    p(t["loss_out"]) if with_loss else None, f_loss)

    def pool(self, pool):
        log_p, m, v, step, eps_safe, lr, loss_in, f_loss = self.args
        f32 = lambda x: float(torch.tensor(x, dtype=torch.float32))
        one = lambda x: torch.tensor([x], dtype=torch.float32, device=DEV)
        stat = float(self.stat)
        want = O.dual_step(f32(log_p) if self.with_step else None, f32(m), f32(v), step, stat, f32(eps_safe), f32(lr), BETAS,
                           ADAM_EPS, f32(loss_in) if self.with_loss else None, f32(f_loss))
        t = self.t
        if not self.with_step:
            for k, x in (("log_p", log_p), ("exp_avg", m), ("exp_avg_sq", v), ("step", float(step))):
                assert float(t[k]) == f32(x)
            assert float(t["value"]) == SENT
        else:
            mp, mm, mv, _ = UP.module_adam(one(log_p), one(eps_safe) - self.stat.reshape(1), one(m), one(v), step, f32(lr),
                                           betas=BETAS, eps=ADAM_EPS)
            pool.add("dual log_p", t["log_p"], mp, want["log_p"].reshape(1))
            pool.add("dual update", t["log_p"].double().cpu() - f32(log_p), mp.double().cpu() - f32(log_p),
                     want["log_p"].reshape(1) - f32(log_p))
            pool.add("dual exp_avg", t["exp_avg"], mm, want["exp_avg"].reshape(1))
            pool.add("dual exp_avg_sq", t["exp_avg_sq"], mv, want["exp_avg_sq"].reshape(1))
            pool.add("dual value", t["value"], mp.exp(), want["value"].reshape(1))
            assert float(t["step"]) == step + 1
        if self.with_loss:
            pool.add("dual loss_out", t["loss_out"], one(loss_in) + f_loss * (self.stat.reshape(1) - eps_safe),
                     want["loss_out"].reshape(1))
        else:
            assert float(t["loss_out"]) == SENT


@pytest.mark.parametrize("n_seg", (0, 2))
def test_dual_steps_against_float64(n_seg):
    pool = Pool()
    lam = dev(torch.tensor([0.7]))
    for i, B in enumerate(UP.BATCHES):
        z = dev(UP.critic_rows(B, seed=30 + i)["a"] * 0.2)
        mean = full(1)
        args = _lib.rrl_penalty_args_t(B, p(z), 1, 0, p(lam), None, p(mean))
        step = (0, 999)[i % 2]
        duals = [Dual(mean, 0.3, 3e-5, step, with_loss=bool(i % 2)), Dual(mean, 0.1, 0.1, step, with_loss=not i % 2),
                 Dual(mean, 0.2, 3e-5, step, with_step=False)]
        segs = [Seg(1023, step, 3e-4, full_opts=True, off=1), Seg(4096, 1, 3e-4)][:n_seg]
        # the statistic comes from the launch in front, on the same stream
        _lib.check(_lib.load().rrl_rcpo_penalty(C.byref(args), _lib.current_stream()), "rrl_rcpo_penalty")
        adam_launch(segs, UP.as_f32(3e-4), [d.desc for d in duals])
        assert float(mean) != SENT
        for d in duals:
            d.pool(pool)
        for s in segs:
            s.pool(pool)
    pool.check()
