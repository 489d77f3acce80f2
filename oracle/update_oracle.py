"""float64 restatements of the element-wise pieces of the updates (include/rrl_hip.h: rrl_policy_head_t, rrl_loss_t,
rrl_rcpo_penalty, rrl_recovery_select, rrl_adam_seg_t, rrl_dual_t), on the CPU with torch.

Written from the formulas of the header and of model.py / sac.py / qrisk.py; every backward the header states is taken with
autograd from the forward restated here.  Nothing is shared with recovery_rl_amd.fast_update or the kernels.  Operands that
the kernels read as partial sums (n_part, da_parts / da_group) are INPUTS here: the caller adds the f32 partials in f32 in
the documented order (fixed_order_sum) and passes the sum.
"""
import math

import torch

F64 = torch.float64
LOG_SIG_MIN, LOG_SIG_MAX, EPSILON = -20.0, 2.0, 1e-6            # model.py:14-16


def f64(x):
    """A detached float64 copy on the host (None stays None; python numbers become 0-dim tensors)."""
    if x is None:
        return None
    if not torch.is_tensor(x):
        return torch.as_tensor(x, dtype=F64).clone()
    return x.detach().to(device="cpu", dtype=F64).clone()


def fixed_order_sum(parts, group=1):
    """The documented sum of f32 partials [n, ...] in f32: ((p0 + p1) + p2) + ..., or with group = 4 every four consecutive
    partials first and then the group sums one after the other.  Stays in the partials' dtype and device."""
    if group > 1:
        sums = [fixed_order_sum(parts[k:k + group]) for k in range(0, parts.shape[0], group)]
        return fixed_order_sum(torch.stack(sums))
    acc = parts[0].clone()
    for k in range(1, parts.shape[0]):
        acc = acc + parts[k]
    return acc


# ---- policy heads (rrl_policy_head_t) -------------------------------------------------------------------------------------
def _gauss(head, eps, scale, bias):
    mean, log_std = head[:, 0:2], head[:, 2:4].clamp(min=LOG_SIG_MIN, max=LOG_SIG_MAX)
    y = torch.tanh(mean + log_std.exp() * eps)
    action = y * scale + bias
    logp = (-0.5 * eps.pow(2) - log_std - 0.5 * math.log(2.0 * math.pi) - torch.log(scale * (1.0 - y.pow(2)) + EPSILON)).sum(1)
    return action, logp, torch.tanh(mean) * scale + bias


def gauss_head(head, eps, scale, bias):
    """GaussianPolicy.sample on the stack output head [B,4] = (mean | raw log-std) -> action [B,2], logp [B], mean_out [B,2]."""
    return _gauss(f64(head), f64(eps), f64(scale), f64(bias))


def _stoch(raw, eps, log_std, min_log_std, scale, bias):
    mean = torch.tanh(raw) * scale + bias
    std = log_std.clamp(min=float(min_log_std)).exp()
    action = mean if eps is None else mean + std * eps
    return action, mean


def stoch_head(raw, eps, log_std, min_log_std, scale, bias):
    """StochasticPolicy.sample on the stack output raw [B,2] -> action [B,2], logp (None: the head has none), mean_out [B,2].
    eps = None: no noise."""
    action, mean = _stoch(f64(raw), f64(eps), f64(log_std), min_log_std, f64(scale), f64(bias))
    return action, None, mean


# ---- the seven rrl_loss_t kinds: dOut [G,B,dout] and loss[] ---------------------------------------------------------------------
def _leaf(x):
    return f64(x).requires_grad_(True)


def sac_critic(q, qt, logp2, r, m, alpha, gamma, penalty=None):
    """q, qt [2,B]; y = r + m gamma (min qt - alpha logp2) [- penalty]; loss[g] = mean (q[g] - y)^2; dOut = d(loss0 + loss1)/dq."""
    q, qt = _leaf(q), f64(qt)
    y = f64(r) + f64(m) * float(gamma) * (torch.min(qt[0], qt[1]) - f64(alpha).reshape(()) * f64(logp2))
    if penalty is not None:
        y = y - f64(penalty)
    loss = ((q - y.unsqueeze(0)) ** 2).mean(1)
    (dq,) = torch.autograd.grad(loss.sum(), q)
    return dq.unsqueeze(-1), loss.detach()


def sac_policy(qp, logp, alpha):
    """loss[0] = mean(alpha logp - min(qp0, qp1)); dOut = dloss/dqp (torch.min: ties split 0.5 / 0.5)."""
    qp = _leaf(qp)
    loss = (f64(alpha).reshape(()) * f64(logp) - torch.min(qp[0], qp[1])).mean()
    (dq,) = torch.autograd.grad(loss, qp)
    return dq.unsqueeze(-1), loss.detach().reshape(1)


def qrisk_critic(z, zt, c, m, gamma_safe):
    """z, zt [2,B] pre-sigmoid; y = c + m gamma_safe max sigmoid(zt); loss[g] = mean (sigmoid(z[g]) - y)^2; dOut w.r.t. z."""
    z, zt = _leaf(z), torch.sigmoid(f64(zt))
    y = f64(c) + f64(m) * float(gamma_safe) * torch.max(zt[0], zt[1])
    loss = ((torch.sigmoid(z) - y.unsqueeze(0)) ** 2).mean(1)
    (dz,) = torch.autograd.grad(loss.sum(), z)
    return dz.unsqueeze(-1), loss.detach()


def dgd_qrisk(zp, nu):
    """loss[0] = mean max sigmoid(zp) (without the factor); dOut = nu dloss/dzp."""
    zp = _leaf(zp)
    q = torch.sigmoid(zp)
    loss = torch.max(q[0], q[1]).mean()
    (dz,) = torch.autograd.grad(loss, zp)
    return float(nu) * dz.unsqueeze(-1), loss.detach().reshape(1)


def qrisk_policy(zp):
    return dgd_qrisk(zp, 1.0)


def gauss_head_bwd(head, eps, scale, d_action, dlogp):
    """Backward of gauss_head: d_action [B,2] = dL/d action (already summed over the critic heads), dlogp = dL/d logp[b] (one
    constant) -> dOut [1,B,4]; no loss scalars."""
    head = _leaf(head)
    action, logp, _ = _gauss(head, f64(eps), f64(scale), torch.zeros(2, dtype=F64))
    (dh,) = torch.autograd.grad((action * f64(d_action)).sum() + float(dlogp) * logp.sum(), head)
    return dh.unsqueeze(0), torch.zeros(0, dtype=F64)


def stoch_head_bwd(raw, eps, log_std, min_log_std, scale, d_action):
    """Backward of stoch_head -> dOut [1,B,2] (w.r.t. raw) and loss[2] = dlog_std (summed over the batch)."""
    raw, log_std = _leaf(raw), _leaf(log_std)
    action, _ = _stoch(raw, f64(eps), log_std, min_log_std, f64(scale), torch.zeros(2, dtype=F64))
    draw, dls = torch.autograd.grad((action * f64(d_action)).sum(), (raw, log_std), allow_unused=True)
    return draw.unsqueeze(0), torch.zeros(2, dtype=F64) if dls is None else dls


# ---- penalty and gate ---------------------------------------------------------------------------------------------------------
def risk(z):
    q = torch.sigmoid(f64(z))
    return torch.max(q[0], q[1])


def rcpo_penalty(z, lam):
    """-> penalty [B] = lambda max sigmoid(z), mean = the batch mean of max sigmoid(z)."""
    q = risk(z)
    return float(lam) * q, q.mean()


def recovery_select(z, eps_safe, task, rec):
    """-> real action [N,2], recovery flag [N] (bool), task action [N,2], and the float64 risk the flag was decided on."""
    q = risk(z)
    flag = q > float(eps_safe)
    task, rec = f64(task)[:, 0:2], f64(rec)
    return torch.where(flag.unsqueeze(1), rec, task), flag, task, q


# ---- optimiser ----------------------------------------------------------------------------------------------------------------
def adam_step(p, g, m, v, t, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, g2=None, target=None, tau=0.0):
    """One torch.optim.Adam step number t + 1 (t = steps taken before), bias corrections in double; optional second gradient
    (g + g2), weight decay (g + wd p) and Polyak target on the updated p.  -> p, m, v, target (None without one)."""
    p, g, m, v = f64(p), f64(g), f64(m), f64(v)
    b1, b2 = float(betas[0]), float(betas[1])
    if g2 is not None:
        g = g + f64(g2)
    g = g + float(weight_decay) * p
    m = b1 * m + (1.0 - b1) * g
    v = b2 * v + (1.0 - b2) * g * g
    bc1, bc2 = 1.0 - b1 ** (t + 1), 1.0 - b2 ** (t + 1)
    p = p - float(lr) / bc1 * m / (v.sqrt() / math.sqrt(bc2) + float(eps))
    if target is not None:
        target = (1.0 - float(tau)) * f64(target) + float(tau) * p
    return p, m, v, target


def dual_step(log_p, exp_avg, exp_avg_sq, step, stat, eps_safe, lr, betas=(0.9, 0.999), eps=1e-8, loss_in=None, f_loss=0.0):
    """rrl_dual_t: one Adam step of the 0-dim log_p with gradient eps_safe - stat, value = exp(log_p), loss_out = loss_in +
    f_loss (stat - eps_safe).  log_p = None: no step.  -> dict of 0-dim float64 tensors (absent members: None)."""
    stat = f64(stat).reshape(())
    out = dict(log_p=None, exp_avg=None, exp_avg_sq=None, step=None, value=None, loss_out=None)
    if loss_in is not None:
        out["loss_out"] = f64(loss_in).reshape(()) + float(f_loss) * (stat - float(eps_safe))
    if log_p is not None:
        t = int(round(float(step)))
        p, m, v, _ = adam_step(f64(log_p).reshape(()), float(eps_safe) - stat, f64(exp_avg).reshape(()),
                               f64(exp_avg_sq).reshape(()), t, lr, betas, eps)
        out.update(log_p=p, exp_avg=m, exp_avg_sq=v, step=torch.tensor(float(t + 1), dtype=F64), value=p.exp())
    return out
