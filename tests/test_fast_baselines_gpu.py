"""The comparison algorithms of the paper (LR, RSPO, SQRL, RCPO: --DGD_constraints, --update_nu, --nu_schedule,
--use_constraint_sampling, --RCPO) on the fused update path, switched on by RRL_FAST_BASELINES=1: the reference's
known answers through the kernels, the fused path against the autograd path, the grouped launches against the separate
ones, the driver and checkpoint / resume."""
import os
import pickle

import numpy as np
import pytest
import torch

import arg_utils
from recovery_rl_amd import checkpoint
from recovery_rl_amd.experiment import Experiment
from recovery_rl_amd.sac import SAC
from recovery_rl_amd.utils import linear_schedule
from test_checkpoint_gpu import _diff
from test_fast_update_gpu import (ACT, DEV, OBS, assert_grads_close, assert_nets_close, batch, close_scaled, load,
                                  make_pair)

pytestmark = pytest.mark.gpu

TWIN = {"linear1.weight": ("W1", 0), "linear4.weight": ("W1", 1), "linear2.weight": ("W2", 0),
        "linear5.weight": ("W2", 1), "linear3.weight": ("W3", 0), "linear6.bias": ("b3", 1),
        "linear2.bias": ("b2", 0), "linear4.bias": ("b1", 1)}

# the SAC-update flags of the comparison lines (scripts/navigation1.sh), and two combinations of their terms
CONFIGS = {"LR": ["--DGD_constraints", "--nu", "50", "--update_nu"],
           "RSPO": ["--DGD_constraints", "--nu_schedule", "--nu_start", "10000", "--num_eps", "400"],
           "RCPO": ["--RCPO", "--lambda_RCPO", "10"],
           "update_nu": ["--nu", "50", "--update_nu"],
           "DGD_RCPO": ["--DGD_constraints", "--nu", "50", "--RCPO", "--lambda_RCPO", "10"]}


def nu_of(args):
    """The nu the driver passes (experiment.py: nu_schedule(1) -- the value the lock-step loop uses throughout)."""
    if args.nu_schedule:
        return linear_schedule(args.nu_start, args.nu_end, args.num_eps)(1)
    return args.nu


def dual_state(agent, name):
    opt, prm = {"nu": (agent.nu_optim, agent.log_nu), "lambda": (agent.lambda_RCPO_optim, agent.log_lambda_RCPO)}[name]
    return opt.state[prm]


@pytest.mark.parametrize("name", ("sac_dgd", "sac_rcpo"))
def test_fused_path_matches_reference_kats(golden_dir, name):
    """G4's LR and RCPO updates (H = 16, B = 8) through the fused kernels: returns, post-step critic, target, policy and the
    log-multipliers against the reference's answers."""
    G = np.load(os.path.join(golden_dir, "model_golden.npz"))
    args = arg_utils.get_args(["--env-name", "navigation1", "--cuda", "--hidden_size", "16"] + str(G[name + ".argv"]).split())
    agent = SAC(OBS, ACT, args, "/tmp")
    pre = name + ".pre"
    load(agent.critic, G, pre + ".critic"); load(agent.critic_target, G, pre + ".critic")
    load(agent.policy, G, pre + ".policy")
    load(agent.safety_critic.safety_critic, G, pre + ".qrisk")
    load(agent.safety_critic.safety_critic_target, G, pre + ".qrisk")
    load(agent.safety_critic.policy, G, pre + ".recpolicy")
    agent.enable_fast_path(8)
    T = lambda k: torch.as_tensor(G[k], device=DEV)
    b = tuple(T("g4.batch." + k) for k in ("s", "a", "r", "s2", "m"))
    res = agent.update_parameters(None, 8, 0, nu=args.nu, safety_critic=agent.safety_critic, batch=b,
                                  eps_next=T("g4.eps_next"), eps_pi=T("g4.eps_pi"), as_floats=True)
    assert np.allclose(res, G[name + ".returns"], rtol=1e-4, atol=2e-6), (res, G[name + ".returns"])
    post = name + ".post"
    for module, prefix in ((agent.critic, ".critic"), (agent.critic_target, ".critic_target"), (agent.policy, ".policy")):
        n = 0
        for k, v in module.state_dict().items():
            if post + prefix + "." + k in G.files:
                assert np.allclose(v.cpu().numpy(), G[post + prefix + "." + k], rtol=1e-4, atol=2e-6), prefix + k
                n += 1
        assert n >= 4
    assert np.isclose(agent.log_nu.item(), G[post + ".log_nu"], rtol=1e-4, atol=2e-6)
    assert np.isclose(agent.log_lambda_RCPO.item(), G[post + ".log_lambda"], rtol=1e-4, atol=2e-6)


@pytest.mark.parametrize("hidden,B", ((32, 64), (256, 256)))
@pytest.mark.parametrize("config", sorted(CONFIGS))
def test_fused_baselines_equal_autograd_path(config, hidden, B):
    """Three SAC + Q_risk updates on identical weights, batches and noise: losses, gradients, parameters, the
    log-multipliers, the multipliers and the duals' Adam state of the fused path against the autograd path."""
    slow, fast, args = make_pair(hidden, CONFIGS[config])
    fast.enable_fast_path(B)
    nu = nu_of(args)
    for step in range(3):
        b_sac, b_qr, e1, e2 = batch(B, 20 + step)
        ls = slow.update_parameters(None, B, step, nu=nu, safety_critic=slow.safety_critic, batch=b_sac, eps_next=e1,
                                    eps_pi=e2)
        lf = fast.update_parameters(None, B, step, nu=nu, safety_critic=fast.safety_critic, batch=b_sac, eps_next=e1,
                                    eps_pi=e2)
        for x, y in zip(ls[:3], lf[:3]):
            assert torch.allclose(x, y, rtol=1e-4, atol=1e-5), (config, step, float(x), float(y))
        fast.fast.gather_first_grads()
        assert_grads_close(slow.critic, fast.fast.critic, TWIN)
        assert_grads_close(slow.policy, fast.fast.policy,
                           {"linear1.weight": ("W1", 0), "linear2.weight": ("W2", 0), "linear2.bias": ("b2", 0)})
        assert close_scaled(fast.fast.policy.g["W3"][0, 0:2], slow.policy.mean_linear.weight.grad)
        assert close_scaled(fast.fast.policy.g["W3"][0, 2:4], slow.policy.log_std_linear.weight.grad)
        slow.safety_critic.update_parameters(policy=slow.policy, batch=b_qr, eps_next=e1, eps_pi=e2)
        fast.safety_critic.update_parameters(policy=fast.policy, batch=b_qr, eps_next=e1, eps_pi=e2)
        for a_, b_ in ((slow.critic, fast.critic), (slow.critic_target, fast.critic_target), (slow.policy, fast.policy),
                       (slow.safety_critic.safety_critic, fast.safety_critic.safety_critic),
                       (slow.safety_critic.policy, fast.safety_critic.policy)):
            assert_nets_close(a_, b_)
        for name, on, log_s, log_f, val_s, val_f in (
                ("nu", args.update_nu, slow.log_nu, fast.log_nu, slow.nu, fast.nu),
                ("lambda", args.RCPO, slow.log_lambda_RCPO, fast.log_lambda_RCPO, slow.lambda_RCPO, fast.lambda_RCPO)):
            assert torch.allclose(log_f, log_s, rtol=1e-4, atol=2e-6), (config, name, float(log_f), float(log_s))
            if not on:
                continue
            assert torch.is_tensor(val_f) and torch.allclose(val_f, torch.as_tensor(val_s, device=DEV), rtol=1e-4)
            st_s, st_f = dual_state(slow, name), dual_state(fast, name)
            assert float(st_f["step"]) == float(st_s["step"]) == step + 1
            assert st_f["step"].dtype == st_s["step"].dtype and st_f["step"].device == st_s["step"].device
            for k in ("exp_avg", "exp_avg_sq"):
                assert torch.allclose(st_f[k], st_s[k], rtol=1e-3, atol=1e-7), (config, name, k)
    if not args.update_nu:
        assert float(fast.log_nu.detach()) == float(np.log(args.nu).astype(np.float32))
    if not args.RCPO:
        assert float(fast.log_lambda_RCPO.detach()) == float(np.log(args.lambda_RCPO).astype(np.float32))


@pytest.mark.parametrize("config", ("LR", "RCPO"))
def test_grouped_baseline_launches_equal_the_separate_ones(config):
    """update_pair (grouped launches) against sac_update / qrisk_update issued one by one, in eager iterations and hipGraph
    replays: every parameter, Adam moment and dual bit-identical."""
    import bench
    loops = []
    for grouped in (True, False):
        cfg = arg_utils.get_args(["--env-name", "navigation1", "--cuda", "--use_recovery", "--MF_recovery", "--num_envs",
                                  "256", "--seed", "4", "--gamma_safe", "0.8", "--eps_safe", "0.3",
                                  "--num_unsafe_transitions", "4000"] + CONFIGS[config])
        loop = bench.build_loop(cfg, torch.device(DEV), pretrain=5)
        loop.agent.fast.grouped = grouped
        loops.append(loop)
    for phase in range(2):
        for loop in loops:
            if phase == 0:
                for _ in range(4):
                    loop.vector_step(True, False, True)
            else:
                loop.capture(online_qrisk=True)
                for _ in range(5):
                    loop.replay()
        torch.cuda.synchronize()
        a, b = loops
        for name in ("critic", "critic_target", "policy", "qrisk", "qrisk_target", "recpolicy"):
            fa, fb = getattr(a.agent.fast, name), getattr(b.agent.fast, name)
            assert torch.equal(fa.flat, fb.flat), (phase, name)
            assert torch.equal(fa.m, fb.m) and torch.equal(fa.v, fb.v) and torch.equal(fa.step, fb.step), (phase, name)
        for attr in ("log_nu", "log_lambda_RCPO"):
            assert torch.equal(getattr(a.agent, attr), getattr(b.agent, attr)), (phase, attr)
        dual = "nu" if config == "LR" else "lambda"
        for k in ("step", "exp_avg", "exp_avg_sq"):
            assert torch.equal(dual_state(a.agent, dual)[k], dual_state(b.agent, dual)[k]), (phase, k)
        assert torch.equal(a.agent.fast.dual_stats, b.agent.fast.dual_stats)
        assert torch.equal(a.env.pos, b.env.pos) and torch.equal(a.stats, b.stats)
    assert float(dual_state(loops[0].agent, dual)["step"]) > 4       # the dual stepped in the replays too


def test_lagrangian_qrisk_gradient_fused_equals_its_stand_alone_kernel():
    """RRL_LOSS_DGD_QRISK inside the head-backward kernel against rrl_loss_dout's launch of its own (fuse_loss = False), the
    one kind tests/test_fast_update_gpu.py's fused / unfused comparison never sends there: the LR line at hidden 32, batch
    64, member by member with the first layer as its own launch on both sides.  Every parameter and gradient after two
    updates bit-identical, the logged losses and dual statistics close."""
    _, a, args = make_pair(32, CONFIGS["LR"])
    _, b, _ = make_pair(32, CONFIGS["LR"])
    B, nu = 64, nu_of(args)
    for ag, fuse in ((a, True), (b, False)):
        ag.enable_fast_path(B)
        ag.fast.fuse_loss = fuse
        ag.fast.set_fuse_first(False)
    for step in range(2):
        b_sac, b_qr, e1, e2 = batch(B, 60 + step)
        for ag in (a, b):
            ag.update_parameters(None, B, step, nu=nu, safety_critic=ag.safety_critic, batch=b_sac, eps_next=e1, eps_pi=e2)
            ag.safety_critic.update_parameters(policy=ag.policy, batch=b_qr, eps_next=e1, eps_pi=e2)
        for name in ("critic", "critic_target", "policy", "qrisk", "qrisk_target", "recpolicy"):
            fa, fb = getattr(a.fast, name), getattr(b.fast, name)
            assert torch.equal(fa.flat, fb.flat), (step, name)
            assert torch.equal(fa.grad, fb.grad), (step, name)
        assert torch.equal(a.log_nu, b.log_nu)
        torch.testing.assert_close(a.fast.losses, b.fast.losses, rtol=1e-5, atol=1e-7)
        torch.testing.assert_close(a.fast.dual_stats, b.fast.dual_stats, rtol=1e-5, atol=1e-7)


def _cfg(tmp, num_eps, extra=()):
    return arg_utils.get_args(["--env-name", "navigation1", "--cuda", "--hidden_size", "32", "--logdir", str(tmp),
                               "--seed", "5", "--num_unsafe_transitions", "2000", "--critic_safe_pretraining_steps",
                               "20", "--num_envs", "64", "--log_every", "10", "--num_eps", str(num_eps),
                               "--gamma_safe", "0.8", "--eps_safe", "0.3"] + list(extra))


# the four comparison lines of scripts/navigation1.sh (without logdir / seed / episode count)
LINES = {"LR": ["--DGD_constraints", "--nu", "5000", "--update_nu"],
         "RSPO": ["--DGD_constraints", "--nu_schedule", "--nu_start", "10000"],
         "SQRL": ["--DGD_constraints", "--use_constraint_sampling", "--nu", "5000", "--update_nu"],
         "RCPO": ["--RCPO", "--lambda_RCPO", "1000"]}


@pytest.mark.parametrize("line", sorted(LINES))
def test_driver_runs_the_comparison_lines_on_the_fused_path(tmp_path, monkeypatch, line):
    calls = []
    orig = SAC._sqrl_action

    def counted(self, *a, **k):
        calls.append(a[0].shape[0])
        return orig(self, *a, **k)
    monkeypatch.setattr(SAC, "_sqrl_action", counted)
    monkeypatch.delenv("RRL_FAST_BASELINES", raising=False)
    assert Experiment(_cfg(tmp_path / "off", 100, LINES[line])).agent.fast is None
    monkeypatch.setenv("RRL_FAST_BASELINES", "1")
    exp = Experiment(_cfg(tmp_path / "on", 150, LINES[line]))
    assert exp.agent.fast is not None and exp.vector_rules["update_path"] == "fused"
    exp.run()
    rs = pickle.load(open(os.path.join(exp.logdir, "run_stats.pkl"), "rb"))
    assert rs["vector_rules"]["update_path"] == "fused"
    assert exp.loop.host_updates[0] > 0
    if line in ("LR", "RCPO"):
        assert exp.loop.graph is not None                 # the steady state replays the captured iteration
    if line == "SQRL":
        assert 64 in calls                                # the training actions of the 64 envs: constraint sampling
    else:
        assert not calls
    if line in ("LR", "SQRL"):
        assert float(exp.agent.log_nu.detach()) != float(np.log(5000.0).astype(np.float32))
    if line == "RCPO":
        assert float(exp.agent.log_lambda_RCPO.detach()) != float(np.log(1000.0).astype(np.float32))
    # env_shard: the duals' gradients are not all-reduced
    with pytest.raises(ValueError, match="comparison algorithms"):
        Experiment(_cfg(tmp_path / "shard", 100, LINES[line] + ["--dp_mode", "env_shard"]), rank=0, world_size=2)


@pytest.mark.parametrize("line", ("LR", "RCPO"))
def test_resumed_fused_baseline_run_equals_uninterrupted_run(tmp_path, monkeypatch, line):
    monkeypatch.setenv("RRL_FAST_BASELINES", "1")
    flags = LINES[line]
    full = Experiment(_cfg(tmp_path / "full", 400, flags))
    assert full.agent.fast is not None
    full.run()
    part = Experiment(_cfg(tmp_path / "part", 150, flags))
    part.run()
    ck = os.path.join(part.logdir, "checkpoint.pt")
    mid = torch.load(ck, map_location="cpu", weights_only=False)
    assert mid["agent"]["update_path"] == "fused"
    cont = Experiment(_cfg(tmp_path / "cont", 400, flags + ["--resume", ck]))
    cont.run()
    a = torch.load(os.path.join(full.logdir, "checkpoint.pt"), map_location="cpu", weights_only=False)
    b = torch.load(os.path.join(cont.logdir, "checkpoint.pt"), map_location="cpu", weights_only=False)
    assert a["extra"]["iteration"] == b["extra"]["iteration"] > mid["extra"]["iteration"]
    d = _diff(a, b)
    assert not d, "\n".join(d)
    # a run on the other path refuses the checkpoint, naming the switch
    monkeypatch.delenv("RRL_FAST_BASELINES")
    other = Experiment(_cfg(tmp_path / "other", 100, flags))
    with pytest.raises(ValueError, match="RRL_FAST_BASELINES"):
        checkpoint.load(other, ck)
