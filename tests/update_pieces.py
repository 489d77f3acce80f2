"""Inputs and module paths shared by test_update_pieces_cpu.py and test_update_pieces_gpu.py.

Inputs: deterministic row classes interleaved by b % 6, built in float64 and rounded to f32 once, so that the float64 oracle,
the module path and the kernels all read the same f32 values.  Module paths: the project's own torch code (GaussianPolicy /
StochasticPolicy.sample, the loss expressions of sac.py / qrisk.py, torch.optim.Adam) on operands of whatever dtype and
device the caller passes -- float64 on the host to check the oracle, float32 on the device as the yardstick of the kernels."""
import math

import numpy as np
import torch
import torch.nn.functional as F

from recovery_rl_amd.model import GaussianPolicy, StochasticPolicy
from recovery_rl_amd.spaces import Box

F64 = torch.float64
BATCHES = (1, 17, 256, 257, 600, 1024)
SCALE, BIAS = (1.0, 0.5), (0.0, 0.25)           # different per action dim: a swapped index shows
ACT = Box(np.array([-1.0, -0.25]), np.array([1.0, 0.75]))      # the box with that scale and bias
# StochasticPolicy's floor log(1e-6) as the f32 the descriptors carry (rrl_policy_head_t.min_log_std, rrl_loss_t.f0): the
# kernels compare with that value, so "exactly at the floor" means at it -- oracle and module path get the same number
MIN_LOG_STD = float(torch.tensor(math.log(1e-6), dtype=torch.float32))



def as_f32(x):
    """A python number as the f32 an ABI `float` argument carries it."""
    return float(torch.tensor(x, dtype=torch.float32))


# Adam's betas and eps as rrl_adam_step_multi receives them: 0.999 arrives as 0.99900001287, so 1 - beta2 is 0.00099998713,
# 1.3e-5 below the 0.001 torch forms in double.  Oracle, module path and kernel are given the same f32 numbers, like every
# other operand here; what the argument type costs against double betas is recorded in DESIGN.md section 5.
BETAS, ADAM_EPS = (as_f32(0.9), as_f32(0.999)), as_f32(1e-8)
GAUSS_CLASSES = ("interior", "raw_at_max", "raw_at_min", "raw_outside", "saturated", "eps_zero")
CRITIC_CLASSES = ("spread", "pm100", "both_one", "tie", "masked", "spread2")


def _gen(seed, B):
    return torch.Generator().manual_seed(100003 * seed + B)


def _f32(x):
    return x.float()


def gauss_rows(B, seed=1):
    """head [B,4], eps [B,2] (f32), cls [B], pre [B,2] (the float64 pre-activation each row was solved for)."""
    g = _gen(seed, B)
    u = lambda *s: torch.rand(*s, generator=g, dtype=F64)
    b = torch.arange(B)
    cls, alt = b % 6, ((b // 6) % 2 == 0)
    raw = (u(B, 2) * 7.5 - 6.0).float().double()                                     # (-6, 1.5)
    eps = torch.randn(B, 2, generator=g, dtype=F64).clamp(-2.5, 2.5).float().double()
    pre = u(B, 2) * 6.0 - 3.0                                                        # |pre| <= 3
    raw[cls == 1] = 2.0
    raw[cls == 2] = -20.0
    out = torch.where(alt, 2.5, -25.0).double()
    raw[cls == 3] = torch.stack([out, torch.where(alt, -25.0, 2.5).double()], 1)[cls == 3]
    sign = torch.where(alt, 1.0, -1.0).double().unsqueeze(1) * torch.tensor([1.0, -1.0], dtype=F64)
    pre[cls == 4] = (sign * (20.5 + 9.0 * u(B, 2)))[cls == 4]                        # |pre| in [20, 30], both signs
    eps[cls == 5] = 0.0
    mean = pre - raw.clamp(-20.0, 2.0).exp() * eps
    return dict(head=_f32(torch.cat([mean, raw], 1)).contiguous(), eps=_f32(eps).contiguous(), cls=cls, pre=pre)


def pre_f32(rows):
    """mean + exp(clamp(raw)) eps evaluated in f32: what the kernels and the f32 module path feed to tanh."""
    h = rows["head"]
    return h[:, 0:2] + h[:, 2:4].clamp(-20.0, 2.0).exp() * rows["eps"]


def stoch_rows(B, seed=2):
    g = _gen(seed, B)
    raw = torch.randn(B, 2, generator=g, dtype=F64) * 1.5
    b = torch.arange(B)
    raw[b % 6 == 4] = (torch.where((b // 6) % 2 == 0, 1.0, -1.0).double().unsqueeze(1) * 25.0)[b % 6 == 4]     # saturated tanh
    eps = torch.randn(B, 2, generator=g, dtype=F64)
    eps[b % 6 == 5] = 0.0
    return dict(raw=_f32(raw).contiguous(), eps=_f32(eps).contiguous())


# log_std above, exactly at and below min_log_std (per action dim: mixed as well)
def stoch_log_stds():
    m = MIN_LOG_STD
    return {"above": (math.log(0.1), -1.0), "at": (m, m), "below": (m - 1.0, m - 3.0), "mixed": (m, m - 2.0)}


def d_action(B, n_heads, ld, seed=3):
    """dL/d action of n_heads critic heads, [n_heads, B, ld] f32 (columns 2.. of a row are other data: the obs gradient)."""
    return torch.randn(n_heads, B, ld, generator=_gen(seed, B), dtype=F64).float().contiguous()


def critic_rows(B, seed=4, wide=True):
    """Twin outputs a, at [2,B] and the per-row operands r, m, c, logp, logp2, penalty [B] (f32), cls [B].
    wide: the Q_risk classes (pre-sigmoid values at +-100, 20 against 30); else those rows are spread too (SAC's q)."""
    g = _gen(seed, B)
    u = lambda *s: torch.rand(*s, generator=g, dtype=F64)
    b = torch.arange(B)
    cls = b % 6
    a, at = u(2, B) * 16.0 - 8.0, u(2, B) * 16.0 - 8.0
    if wide:
        s = torch.where((b // 6) % 2 == 0, 1.0, -1.0).double()
        a[:, cls == 1] = torch.stack([100.0 * s, -100.0 * s])[:, cls == 1]
        at[:, cls == 1] = torch.stack([-100.0 * s, 100.0 * s])[:, cls == 1]
        a[:, cls == 2] = torch.tensor([[20.0], [30.0]], dtype=F64)
        at[:, cls == 2] = torch.tensor([[30.0], [20.0]], dtype=F64)
    a[1, cls == 3] = a[0, cls == 3]
    at[1, cls == 3] = at[0, cls == 3]
    m = torch.ones(B, dtype=F64)
    m[cls == 4] = 0.0
    r = torch.randn(B, generator=g, dtype=F64)
    c = (u(B) < 0.3).double()
    logp, logp2 = torch.randn(B, generator=g, dtype=F64) * 2.0, torch.randn(B, generator=g, dtype=F64) * 2.0
    penalty = u(B) * 0.7
    t = lambda x: _f32(x).contiguous()
    return dict(a=t(a), at=t(at), r=t(r), m=t(m), c=t(c), logp=t(logp), logp2=t(logp2), penalty=t(penalty), cls=cls)


def select_rows(N, seed=5):
    """z [2,N] spread over +-4, one row in 97 (from row 60 on: about 1 % of a batch) at +-100 (risk exactly 0 or 1 in f32),
    task [N,4] and rec [N,2] actions."""
    g = _gen(seed, N)
    z = torch.rand(2, N, generator=g, dtype=F64) * 8.0 - 4.0
    b = torch.arange(N)
    z[:, b % 97 == 60] = (torch.where((b // 97) % 2 == 0, 100.0, -100.0).double())[b % 97 == 60]
    task = torch.randn(N, 4, generator=g, dtype=F64)
    rec = torch.randn(N, 2, generator=g, dtype=F64)
    return dict(z=_f32(z).contiguous(), task=_f32(task).contiguous(), rec=_f32(rec).contiguous())


def adam_state(n, seed=6):
    """p, g, g2, m, v, target of n elements (f32) from a running state; every 7th entry has v ~ 1e-16, g = 0, m ~ 1e-9."""
    g_ = _gen(seed, n)
    rn = lambda s: torch.randn(n, generator=g_, dtype=F64) * s
    p, g, g2, m, target = rn(0.5), rn(0.1), rn(0.05), rn(0.05), rn(0.5)
    v = rn(0.1) ** 2 + 2.5e-3                # sqrt(v) >= 0.05: steps of a few lr, as a running state has them
    quiet = torch.arange(n) % 7 == 3
    g[quiet], g2[quiet], m[quiet], v[quiet] = 0.0, 0.0, 1e-9, 1e-16
    return {k: _f32(x).contiguous() for k, x in dict(p=p, g=g, g2=g2, m=m, v=v, target=target).items()}


# ---- module paths -------------------------------------------------------------------------------------------------------------
def _policy(cls, like):
    """A policy module whose trunk hands the stack output through and whose last layer is the identity: sample(head) is then
    the module's own sampling code on `head` (x * 1 + y * 0 + 0 is exact)."""
    pol = cls(4 if cls is GaussianPolicy else 2, 2, 4 if cls is GaussianPolicy else 2, ACT)
    pol.trunk = lambda state: state
    with torch.no_grad():
        if cls is GaussianPolicy:
            pol.mean_linear.weight.copy_(torch.eye(4)[0:2])
            pol.log_std_linear.weight.copy_(torch.eye(4)[2:4])
            pol.mean_linear.bias.zero_()
            pol.log_std_linear.bias.zero_()
        else:
            pol.mean.weight.copy_(torch.eye(2))
            pol.mean.bias.zero_()
    return pol.to(device=like.device, dtype=like.dtype)


def module_gauss(head, eps, d_act=None, dlogp=0.0):
    """GaussianPolicy.sample -> action, logp [B], mean_out (and dhead [B,4] by autograd when d_act is given)."""
    pol = _policy(GaussianPolicy, head)
    head = head.clone().requires_grad_(d_act is not None)
    action, logp, mean = pol.sample(head, eps)
    logp = logp.squeeze(1)
    if d_act is None:
        return action.detach(), logp.detach(), mean.detach()
    (dh,) = torch.autograd.grad((action * d_act).sum() + dlogp * logp.sum(), head)
    return action.detach(), logp.detach(), mean.detach(), dh


def module_stoch(raw, eps, log_std, d_act=None):
    """StochasticPolicy.sample -> action, mean_out (and draw [B,2], dlog_std [2] when d_act is given)."""
    pol = _policy(StochasticPolicy, raw)
    pol.min_log_std = MIN_LOG_STD
    with torch.no_grad():
        pol.log_std.copy_(log_std)
    raw = raw.clone().requires_grad_(d_act is not None)
    action, _, mean = pol.sample(raw, torch.zeros_like(raw) if eps is None else eps)
    if d_act is None:
        return action.detach(), mean.detach()
    draw, dls = torch.autograd.grad((action * d_act).sum(), (raw, pol.log_std))
    return action.detach(), mean.detach(), draw, dls


def module_sac_critic(q, qt, logp2, r, m, alpha, gamma, penalty=None):
    """sac.py: next_q and the two MSEs -> dq [2,B], losses [2]."""
    q = q.clone().requires_grad_(True)
    with torch.no_grad():
        min_qn = torch.min(qt[0], qt[1]) - alpha * logp2
        next_q = r + m * gamma * min_qn
        if penalty is not None:
            next_q = next_q - penalty
    l1, l2 = F.mse_loss(q[0], next_q), F.mse_loss(q[1], next_q)
    (dq,) = torch.autograd.grad(l1 + l2, q)
    return dq, torch.stack([l1, l2]).detach()


def module_sac_policy(qp, logp, alpha):
    qp = qp.clone().requires_grad_(True)
    loss = ((alpha * logp) - torch.min(qp[0], qp[1])).mean()
    (dq,) = torch.autograd.grad(loss, qp)
    return dq, loss.detach().reshape(1)


def module_qrisk_critic(z, zt, c, m, gamma_safe):
    """qrisk.py: target and the two MSEs on the squashed heads -> dz [2,B], losses [2]."""
    z = z.clone().requires_grad_(True)
    with torch.no_grad():
        q1n, q2n = torch.sigmoid(zt[0]), torch.sigmoid(zt[1])
        target = c + m * gamma_safe * torch.max(q1n, q2n)
    q1, q2 = torch.sigmoid(z[0]), torch.sigmoid(z[1])
    l1, l2 = F.mse_loss(q1, target), F.mse_loss(q2, target)
    (dz,) = torch.autograd.grad(l1 + l2, z)
    return dz, torch.stack([l1, l2]).detach()


def module_qrisk_policy(zp, nu=None):
    """qrisk.py: max(q1p, q2p).mean(); with nu the Q_risk half of sac.py's Lagrangian policy loss, nu * max_sqf_pi."""
    zp = zp.clone().requires_grad_(True)
    mx = torch.max(torch.sigmoid(zp[0]), torch.sigmoid(zp[1]))
    loss = mx.mean() if nu is None else (nu * mx).mean()
    (dz,) = torch.autograd.grad(loss, zp)
    return dz, mx.mean().detach().reshape(1)


def module_adam(p, g, m, v, t, lr, weight_decay=0.0, g2=None, target=None, tau=0.0, betas=(0.9, 0.999), eps=1e-8):
    """torch.optim.Adam (capturable where the device allows it) from the given state -> p, m, v, target."""
    prm = torch.nn.Parameter(p.clone())
    capturable = p.is_cuda
    opt = torch.optim.Adam([prm], lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, capturable=capturable)
    step = torch.tensor(float(t), dtype=torch.float32, device=p.device) if capturable else torch.tensor(float(t))
    opt.state[prm] = dict(step=step, exp_avg=m.clone(), exp_avg_sq=v.clone())
    prm.grad = g.clone() if g2 is None else g + g2
    opt.step()
    st = opt.state[prm]
    new_t = None
    if target is not None:                      # utils.soft_update
        new_t = target * (1.0 - tau) + prm.data * tau
    return prm.data, st["exp_avg"], st["exp_avg_sq"], new_t


def scaled_err(got, want):
    """(largest absolute error against the float64 `want`, the scale of `want`)."""
    got, want = got.detach().to("cpu", F64), want.detach().to("cpu", F64)
    return float((got - want).abs().max()), float(want.abs().max())
