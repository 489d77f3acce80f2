"""The float64 restatements of oracle/update_oracle.py are right, and the inputs of test_update_pieces_gpu.py are fair.

Right: each restatement equals the project's module code run in float64 (to 1e-12 of scale) and the reference's known
answers of tests/golden/model_golden.npz (within that file's tolerances).  Fair: every row class is present, no row sits
where the reference formula itself is ill-conditioned, and the f32 module path stays within 1e-5 of scale on these inputs."""
import os

import numpy as np
import pytest
import torch

import update_pieces as UP
from oracle import update_oracle as O

F64 = torch.float64
SCALE, BIAS = torch.tensor(UP.SCALE), torch.tensor(UP.BIAS)
ALPHA, GAMMA, GAMMA_SAFE = torch.tensor(0.2), 0.99, 0.65


def d(x):
    return None if x is None else x.double()


def assert_same(got, want, what, rel=1e-12):
    err, scale = UP.scaled_err(got, want)
    assert err <= rel * max(scale, 1e-300), (what, err, scale)


# ---- the oracle against the module code in float64 --------------------------------------------------------------------------
@pytest.mark.parametrize("B", (17, 600))
def test_gauss_head_and_its_backward_equal_the_module_in_float64(B):
    rows, da = UP.gauss_rows(B), UP.d_action(B, 1, 2)[0]
    act, logp, mean, dh = UP.module_gauss(d(rows["head"]), d(rows["eps"]), d(da), 0.2 / B)
    o_act, o_logp, o_mean = O.gauss_head(rows["head"], rows["eps"], SCALE, BIAS)
    o_dh, _ = O.gauss_head_bwd(rows["head"], rows["eps"], SCALE, da, 0.2 / B)
    for got, want, what in ((o_act, act, "action"), (o_logp, logp, "logp"), (o_mean, mean, "mean"), (o_dh[0], dh, "dhead")):
        assert_same(got, want, what)


@pytest.mark.parametrize("which", sorted(UP.stoch_log_stds()))
def test_stoch_head_and_its_backward_equal_the_module_in_float64(which):
    B = 257
    rows, da = UP.stoch_rows(B), UP.d_action(B, 1, 2)[0]
    ls = torch.tensor(UP.stoch_log_stds()[which], dtype=torch.float32)
    act, mean, draw, dls = UP.module_stoch(d(rows["raw"]), d(rows["eps"]), d(ls), d(da))
    o_act, _, o_mean = O.stoch_head(rows["raw"], rows["eps"], ls, UP.MIN_LOG_STD, SCALE, BIAS)
    o_draw, o_dls = O.stoch_head_bwd(rows["raw"], rows["eps"], ls, UP.MIN_LOG_STD, SCALE, da)
    for got, want, what in ((o_act, act, "action"), (o_mean, mean, "mean"), (o_draw[0], draw, "draw"), (o_dls, dls, "dlog_std")):
        assert_same(got, want, what)
    no_noise, _, _ = O.stoch_head(rows["raw"], None, ls, UP.MIN_LOG_STD, SCALE, BIAS)
    assert torch.equal(no_noise, o_mean)


@pytest.mark.parametrize("B", (17, 257))
def test_loss_kinds_equal_the_module_expressions_in_float64(B):
    s, w = UP.critic_rows(B, wide=False), UP.critic_rows(B)
    for pen in (None, s["penalty"]):
        got = O.sac_critic(s["a"], s["at"], s["logp2"], s["r"], s["m"], ALPHA, GAMMA, pen)
        want = UP.module_sac_critic(d(s["a"]), d(s["at"]), d(s["logp2"]), d(s["r"]), d(s["m"]), d(ALPHA), GAMMA, d(pen))
        assert_same(got[0][..., 0], want[0], "sac critic dq")
        assert_same(got[1], want[1], "sac critic loss")
    got, want = O.sac_policy(s["a"], s["logp"], ALPHA), UP.module_sac_policy(d(s["a"]), d(s["logp"]), d(ALPHA))
    assert_same(got[0][..., 0], want[0], "sac policy dq")
    assert_same(got[1], want[1], "sac policy loss")
    got = O.qrisk_critic(w["a"], w["at"], w["c"], w["m"], GAMMA_SAFE)
    want = UP.module_qrisk_critic(d(w["a"]), d(w["at"]), d(w["c"]), d(w["m"]), GAMMA_SAFE)
    assert_same(got[0][..., 0], want[0], "qrisk critic dz")
    assert_same(got[1], want[1], "qrisk critic loss")
    for nu in (None, 3.5):
        got = O.qrisk_policy(w["a"]) if nu is None else O.dgd_qrisk(w["a"], nu)
        want = UP.module_qrisk_policy(d(w["a"]), nu)
        assert_same(got[0][..., 0], want[0], "qrisk policy dz")
        assert_same(got[1], want[1], "qrisk policy loss")


@pytest.mark.parametrize("t", (0, 1, 999, 99999))
@pytest.mark.parametrize("wd,with_g2,with_target", ((0.0, False, False), (1e-2, True, True)))
def test_adam_step_equals_torch_adam_in_float64(t, wd, with_g2, with_target):
    s = {k: d(x) for k, x in UP.adam_state(1023).items()}
    g2, tgt = (s["g2"] if with_g2 else None), (s["target"] if with_target else None)
    want = UP.module_adam(s["p"], s["g"], s["m"], s["v"], t, 0.1, wd, g2, tgt, 0.005)
    got = O.adam_step(s["p"], s["g"], s["m"], s["v"], t, 0.1, weight_decay=wd, g2=g2, target=tgt, tau=0.005)
    for a, b, what in zip(got, want, ("p", "m", "v", "target")):
        if b is not None:
            assert_same(a, b, what)
    assert_same(got[0] - s["p"], want[0] - s["p"], "update", rel=1e-10)      # a difference of two p: 1e-16 |p| / |update|


@pytest.mark.parametrize("t", (0, 999))
def test_dual_step_is_one_adam_step_then_exp(t):
    stat, eps_safe, lr = 0.37, 0.2, 3e-5
    out = O.dual_step(-1.2, 0.01, 4e-4, t, stat, eps_safe, lr, loss_in=0.8, f_loss=2.5)
    p, m, v, _ = UP.module_adam(torch.tensor([-1.2], dtype=F64), torch.tensor([eps_safe - stat], dtype=F64),
                                torch.tensor([0.01], dtype=F64), torch.tensor([4e-4], dtype=F64), t, lr)
    assert_same(out["log_p"], p[0], "log_p")
    assert_same(out["exp_avg"], m[0], "exp_avg")
    assert_same(out["exp_avg_sq"], v[0], "exp_avg_sq")
    assert_same(out["value"], p[0].exp(), "value")
    assert float(out["step"]) == t + 1
    assert_same(out["loss_out"], torch.tensor(0.8 + 2.5 * (stat - eps_safe), dtype=F64), "loss_out")
    skipped = O.dual_step(None, None, None, None, stat, eps_safe, lr, loss_in=0.8, f_loss=2.5)
    assert skipped["log_p"] is None and skipped["value"] is None and float(skipped["loss_out"]) == float(out["loss_out"])


def test_penalty_and_gate_restatements():
    r = UP.select_rows(600)
    z = d(r["z"])
    want = torch.max(torch.sigmoid(z[0]), torch.sigmoid(z[1]))            # QRiskWrapper.get_value on pre-sigmoid heads
    pen, mean = O.rcpo_penalty(r["z"], 0.7)
    assert_same(pen, 0.7 * want, "penalty")
    assert_same(mean, want.mean(), "mean")
    real, flag, task, risk = O.recovery_select(r["z"], 0.3, r["task"], r["rec"])
    assert torch.equal(flag, want > 0.3) and torch.equal(risk, want)
    assert torch.equal(real[flag], d(r["rec"])[flag]) and torch.equal(real[~flag], d(r["task"])[~flag][:, 0:2])
    assert torch.equal(task, d(r["task"])[:, 0:2])


# ---- the oracle against the reference's known answers --------------------------------------------------------------------------
RTOL, ATOL = 1e-4, 2e-6               # test_models_cpu.py: the tolerances of model_golden.npz


@pytest.fixture(scope="module")
def G(golden_dir):
    return np.load(os.path.join(golden_dir, "model_golden.npz"))


def lin(G, prefix, x):
    return x @ torch.as_tensor(G[prefix + ".weight"]).double().T + torch.as_tensor(G[prefix + ".bias"]).double()


def trunk(G, prefix, x, first="linear1", second="linear2"):
    return torch.relu(lin(G, prefix + "." + second, torch.relu(lin(G, prefix + "." + first, x))))


def near(got, want):
    return np.allclose(got.detach().numpy(), want, rtol=RTOL, atol=ATOL)


def test_heads_match_the_reference_known_answers(G):
    s, eps = torch.as_tensor(G["g3.s"]).double(), torch.as_tensor(G["g3.eps"])
    one, zero = torch.ones(2), torch.zeros(2)                             # the KATs' action box is [-1, 1]^2
    h = trunk(G, "g3.gp", s)
    head = torch.cat([lin(G, "g3.gp.mean_linear", h), lin(G, "g3.gp.log_std_linear", h)], 1)
    act, logp, mean = O.gauss_head(head, eps, one, zero)
    assert near(act, G["g3.gp.action"]) and near(mean, G["g3.gp.mean"])
    # logp: the known answers are the reference's own f32 run, and with a pre-activation in 4 < |pre| < 18 its
    # log(scale (1 - y^2) + 1e-6) loses up to 6 % to the rounding of 1 - y^2 (half of these 8 rows: 7.3447 there against
    # 7.3574 in float64) -- the band the generated inputs keep out of.  The rows outside it hold the tolerance.
    pre = (head[:, 0:2] + head[:, 2:4].clamp(-20, 2).exp() * eps.double()).abs()
    fair = ~((pre > 4.0) & (pre < 18.0)).any(1)
    assert int(fair.sum()) >= 3 and near(logp[fair], G["g3.gp.logp"][:, 0][fair.numpy()])
    raw = lin(G, "g3.sp.mean", trunk(G, "g3.sp", s))
    act, _, mean = O.stoch_head(raw, eps, G["g3.sp.log_std"], UP.MIN_LOG_STD, one, zero)
    assert near(act, G["g3.sp.action"]) and near(mean, G["g3.sp.mean"])


def test_sac_losses_match_the_reference_known_answers(G):
    """`sac.returns` = (q1 loss, q2 loss, policy loss, ...) of one reference update from the `sac.pre` weights on the g4 batch."""
    b = {k: torch.as_tensor(G["g4.batch." + k]).double() for k in ("s", "a", "r", "s2", "m")}
    one, zero = torch.ones(2), torch.zeros(2)
    import arg_utils
    args = arg_utils.get_args(["--env-name", "navigation1", "--hidden_size", "16"] + str(G["sac.argv"]).split())
    alpha = torch.tensor(float(args.alpha))

    def policy(s, eps):
        h = trunk(G, "sac.pre.policy", s)
        head = torch.cat([lin(G, "sac.pre.policy.mean_linear", h), lin(G, "sac.pre.policy.log_std_linear", h)], 1)
        return O.gauss_head(head, eps, one, zero)

    def critic(s, a):
        x = torch.cat([s, a], 1)
        q1 = lin(G, "sac.pre.critic.linear3", trunk(G, "sac.pre.critic", x))
        q2 = lin(G, "sac.pre.critic.linear6", trunk(G, "sac.pre.critic", x, "linear4", "linear5"))
        return torch.stack([q1[:, 0], q2[:, 0]])

    a2, logp2, _ = policy(b["s2"], torch.as_tensor(G["g4.eps_next"]))
    _, loss = O.sac_critic(critic(b["s"], b["a"]), critic(b["s2"], a2), logp2, b["r"], b["m"], alpha, args.gamma)
    pi, logp, _ = policy(b["s"], torch.as_tensor(G["g4.eps_pi"]))
    _, ploss = O.sac_policy(critic(b["s"], pi), logp, alpha)
    assert near(torch.cat([loss, ploss]), G["sac.returns"][0:3])


# ---- the conventions the kernels encode ------------------------------------------------------------------------------------------
def test_min_and_max_split_a_tie_in_halves():
    for fn, sign in ((torch.min, 1.0), (torch.max, 1.0)):
        a = torch.tensor([1.5, 2.0, -3.0], dtype=F64, requires_grad=True)
        b = torch.tensor([1.5, 1.0, -3.0], dtype=F64, requires_grad=True)
        ga, gb = torch.autograd.grad(fn(a, b).sum(), (a, b))
        assert ga[0] == 0.5 and gb[0] == 0.5 and ga[2] == 0.5 and gb[2] == 0.5
        assert {float(ga[1]), float(gb[1])} == {0.0, 1.0}


def test_clamp_passes_the_gradient_at_both_bounds_and_blocks_it_outside():
    x = torch.tensor([-25.0, -20.0, -19.0, 2.0, 2.5], dtype=F64, requires_grad=True)
    (g,) = torch.autograd.grad(torch.clamp(x, min=O.LOG_SIG_MIN, max=O.LOG_SIG_MAX).sum(), x)
    assert g.tolist() == [0.0, 1.0, 1.0, 1.0, 0.0]
    m = UP.MIN_LOG_STD
    y = torch.tensor([m - 1.0, m, m + 1.0], dtype=F64, requires_grad=True)
    (g,) = torch.autograd.grad(torch.clamp(y, min=m).sum(), y)
    assert g.tolist() == [0.0, 1.0, 1.0]


# ---- the input generators ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", UP.BATCHES)
def test_every_row_class_is_present_and_no_row_is_in_the_ill_conditioned_band(B):
    rows, w = UP.gauss_rows(B), UP.critic_rows(B)
    if B >= 6:
        assert set(rows["cls"].tolist()) == set(range(6)) and set(w["cls"].tolist()) == set(range(6))
        h, cls = rows["head"], rows["cls"]
        assert bool((h[cls == 1, 2:4] == 2.0).all()) and bool((h[cls == 2, 2:4] == -20.0).all())
        out = h[cls == 3, 2:4]
        assert bool(((out == 2.5) | (out == -25.0)).all()) and (B < 12 or {2.5, -25.0} == set(out.flatten().tolist()))
        inner = h[(cls == 0) | (cls == 5), 2:4]
        assert bool(((inner > -6.0) & (inner < 1.5)).all()) and bool((rows["eps"][cls == 5] == 0).all())
        a, at, c = w["a"], w["at"], w["cls"]
        assert bool((a[0, c == 3] == a[1, c == 3]).all()) and bool((at[0, c == 3] == at[1, c == 3]).all())
        assert bool((a[:, c == 1].abs() == 100).all()) and bool((w["m"][c == 4] == 0).all()) and bool((w["m"][c != 4] == 1).all())
        both = torch.sigmoid(a[:, c == 2])
        assert bool((both == 1.0).all()) and a[0, c == 2][0] == 20 and a[1, c == 2][0] == 30     # f32: both sigmoids round to 1
    pre = UP.pre_f32(rows).abs()
    assert not bool(((pre > 4.0) & (pre < 18.0)).any())
    sat = pre[rows["cls"] == 4]
    assert bool(((sat >= 20.0) & (sat <= 30.0)).all())
    if B >= 12:
        signed = UP.pre_f32(rows)[rows["cls"] == 4]
        assert bool((signed > 0).any()) and bool((signed < 0).any())
        assert bool((torch.tanh(signed).abs() == 1.0).all())                                   # saturated in f32


@pytest.mark.parametrize("N", UP.BATCHES)
@pytest.mark.parametrize("eps_safe", (0.0, 0.3, 1.0))
def test_the_gate_inputs_exempt_at_most_two_percent_of_the_rows(N, eps_safe):
    r = UP.select_rows(N)
    near_thr = (O.risk(r["z"]) - eps_safe).abs() <= 1e-6
    assert int(near_thr.sum()) <= 0.02 * N


def test_the_f32_module_path_is_within_1e5_of_scale_on_these_inputs():
    worst = {}

    def note(name, got, want):
        err, scale = UP.scaled_err(got, want)
        assert err <= 1e-5 * scale, (name, err, scale)
        worst[name] = max(worst.get(name, 0.0), err / scale)

    for B in UP.BATCHES:
        rows, da = UP.gauss_rows(B), UP.d_action(B, 1, 2)[0]
        act, logp, mean, dh = UP.module_gauss(rows["head"], rows["eps"], da, 0.2 / B)
        o = O.gauss_head(rows["head"], rows["eps"], SCALE, BIAS)
        note("action", act, o[0]), note("logp", logp, o[1]), note("mean_out", mean, o[2])
        note("dhead", dh, O.gauss_head_bwd(rows["head"], rows["eps"], SCALE, da, 0.2 / B)[0][0])
        st = UP.stoch_rows(B)
        ls = torch.tensor(UP.stoch_log_stds()["above"], dtype=torch.float32)
        sact, smean, draw, dls = UP.module_stoch(st["raw"], st["eps"], ls, da)
        note("stoch action", sact, O.stoch_head(st["raw"], st["eps"], ls, UP.MIN_LOG_STD, SCALE, BIAS)[0])
        o_draw, o_dls = O.stoch_head_bwd(st["raw"], st["eps"], ls, UP.MIN_LOG_STD, SCALE, da)
        note("draw", draw, o_draw[0]), note("dlog_std", dls, o_dls)
        s, w = UP.critic_rows(B, wide=False), UP.critic_rows(B)
        got = UP.module_sac_critic(s["a"], s["at"], s["logp2"], s["r"], s["m"], ALPHA, GAMMA, s["penalty"])
        want = O.sac_critic(s["a"], s["at"], s["logp2"], s["r"], s["m"], ALPHA, GAMMA, s["penalty"])
        note("sac critic dq", got[0], want[0][..., 0]), note("sac critic loss", got[1], want[1])
        got, want = UP.module_qrisk_critic(w["a"], w["at"], w["c"], w["m"], GAMMA_SAFE), O.qrisk_critic(w["a"], w["at"], w["c"], w["m"], GAMMA_SAFE)
        note("qrisk critic dz", got[0], want[0][..., 0]), note("qrisk critic loss", got[1], want[1])
        got, want = UP.module_qrisk_policy(w["a"]), O.qrisk_policy(w["a"])
        note("qrisk policy dz", got[0], want[0][..., 0]), note("qrisk policy loss", got[1], want[1])
    for name, rel in sorted(worst.items()):
        print("%s: f32 module path against float64: %.2e of scale" % (name, rel))
