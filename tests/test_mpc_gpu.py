"""GPU parity tests: CEM kernels vs the C oracle (bit-exact) and vs the reference's CEM iteration
(G8); MPC._compile_cost vs the reference KAT (G7c); batched planning end to end."""
import os

import numpy as np
import pytest
import torch

import arg_utils
from oracle import c_oracle as co
from recovery_rl_amd import _lib
from recovery_rl_amd.MPC import MPC
from recovery_rl_amd.config import create_config
from recovery_rl_amd.env import make_vec_env
from recovery_rl_amd.optimizers import CEMOptimizer
from recovery_rl_amd.sac import SAC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def G(golden_dir):
    return np.load(os.path.join(golden_dir, "mpc_golden.npz"))


def T(x, dt=None):
    return torch.as_tensor(np.ascontiguousarray(x), device=DEV) if dt is None else \
        torch.as_tensor(np.ascontiguousarray(x, dtype=dt), device=DEV)


def cem_desc(M, pop, dim, m_dev=None, **tensors):
    """rrl_cem_t over `tensors` (field name -> device tensor); what is not given stays NULL / 0."""
    return _lib.rrl_cem_t(M=M, m_dev=_lib.ptr(m_dev), pop=pop, dim=dim, **{k: _lib.ptr(t) for k, t in tensors.items()})


def hip_cem_sample(mean, var, lb, ub, pop, epsilon=1e-3, sticky=False, active=None, seed=0, counter=0):
    lib = _lib.load()
    M, dim = mean.shape
    mean_t, var_t, lb_t, ub_t = T(mean, np.float64), T(var, np.float64), T(lb, np.float64), T(ub, np.float64)
    act = T(np.ones(M, np.uint8) if active is None else active, np.uint8)
    samples = torch.zeros(M, pop, dim, device=DEV)
    c = cem_desc(M, pop, dim, mean=mean_t, var=var_t, lb=lb_t, ub=ub_t, active=act, samples=samples)
    c.epsilon, c.sticky, c.seed, c.counter = epsilon, int(sticky), seed, counter
    rc = lib.rrl_cem_sample(c, _lib.current_stream())
    assert rc == 0
    return samples.cpu().numpy(), act.cpu().numpy()


def hip_cem_update(samples, costs, mean, var, ne, alpha, active=None):
    lib = _lib.load()
    M, pop, dim = samples.shape
    s, c = T(samples, np.float32), T(costs, np.float32)
    m, v = T(mean, np.float64).clone(), T(var, np.float64).clone()
    a = None if active is None else T(active, np.uint8)
    desc = cem_desc(M, pop, dim, samples=s, costs=c, mean=m, var=v, active=a)
    desc.num_elites, desc.alpha = ne, alpha
    rc = lib.rrl_cem_update(desc, _lib.current_stream())
    assert rc == 0
    return m.cpu().numpy(), v.cpu().numpy()


def cem_device_count(mean, var, lb, ub, pop, costs, ne, alpha, live, seed, counter):
    """Sample, then update on the sample kernel's own output, with the number of problems read from device memory
    (m_dev[0] = live) and every buffer sized for three problems more than `mean` has, sentinels everywhere.
    -> (samples, active, mean, var) of all M + 3 rows after the sample and (mean, var) after the update, the tick."""
    lib, st = _lib.load(), _lib.current_stream()
    M, dim = mean.shape
    pad = lambda x, fill, dt: T(np.concatenate([x, np.full((3,) + x.shape[1:], fill, x.dtype)]), dt)
    mean_t, var_t = pad(mean, -5.0, np.float64), pad(var, -5.0, np.float64)
    act = T(np.full(M + 3, 9, np.uint8))
    samples = torch.full((M + 3, pop, dim), 7.0, device=DEV)
    costs_t = pad(costs, 0.0, np.float32)
    m_dev = T(np.array([live], np.int32))
    tick = torch.zeros(2, dtype=torch.int64, device=DEV)
    c = cem_desc(M + 3, pop, dim, m_dev, mean=mean_t, var=var_t, lb=T(lb, np.float64), ub=T(ub, np.float64), active=act,
                 samples=samples, costs=costs_t, counter_dev=tick)
    c.epsilon, c.seed, c.counter, c.counter_inc, c.num_elites, c.alpha = 1e-3, seed, counter, 1, ne, alpha
    assert lib.rrl_cem_sample(c, st) == 0
    sampled = [t.cpu().numpy().copy() for t in (samples, act, mean_t, var_t)]
    assert lib.rrl_cem_update(c, st) == 0
    return sampled, (mean_t.cpu().numpy(), var_t.cpu().numpy()), int(tick[0].item())


CEM_SHAPES = ((1, 400, 10), (37, 400, 10), (5, 400, 30), (300, 64, 4), (2, 1000, 7))


@pytest.mark.parametrize("M,pop,dim,device_count", [pytest.param(*s, False, id="%d-%d-%d" % s) for s in CEM_SHAPES] + [
    pytest.param(*s, True, id="%d-%d-%d-device_count" % s) for s in ((1, 400, 10), (37, 400, 10), (2, 1000, 7))])
def test_cem_kernels_match_oracle_bit_exact(M, pop, dim, device_count):
    rng = np.random.RandomState(M * 1000 + pop + dim)
    mean = rng.uniform(-0.9, 0.9, (M, dim))
    var = rng.uniform(0.0, 0.3, (M, dim))
    var[M // 2] = 1e-5
    lb, ub = -np.ones(dim), np.ones(dim)
    ref_s, ref_a = co.cem_sample(mean, var, lb, ub, pop, seed=9, counter=4)
    costs = rng.randn(M, pop).astype(np.float32)
    costs[0, :3] = np.nan                                   # NaN -> 1e6
    costs[-1, 5] = costs[-1, 6]                             # tie -> lower index first
    ne = max(1, pop // 10)
    ref_m, ref_v = co.cem_update(ref_s, costs, mean, var, ne, 0.1, active=ref_a)
    if device_count:
        (got_s, got_a, m0, v0), (got_m, got_v), tick = cem_device_count(mean, var, lb, ub, pop, costs, ne, 0.1, M, 9, 4)
        assert np.array_equal(m0[:M], mean) and np.array_equal(v0[:M], var)         # the sample step writes neither
        # the three rows past the count keep their sentinels through both steps
        assert (got_s[M:] == 7.0).all() and (got_a[M:] == 9).all()
        assert (got_m[M:] == -5.0).all() and (got_v[M:] == -5.0).all() and (m0[M:] == -5.0).all() and (v0[M:] == -5.0).all()
        assert tick == 1
        got_s, got_a, got_m, got_v = got_s[:M], got_a[:M], got_m[:M], got_v[:M]
        # an inactive problem's samples are not drawn: the oracle leaves zeros, this buffer its sentinel
        assert (got_s[ref_a == 0] == 7.0).all()
        got_s = np.where((ref_a == 0)[:, None, None], ref_s, got_s)
        # an empty set: nothing is written, the tick stays
        (s_, a_, m_, v_), (m2, v2), tick = cem_device_count(mean, var, lb, ub, pop, costs, ne, 0.1, 0, 9, 4)
        assert (s_ == 7.0).all() and (a_ == 9).all() and tick == 0
        for got_mean, got_var in ((m_, v_), (m2, v2)):
            assert np.array_equal(got_mean[:M], mean) and np.array_equal(got_var[:M], var)
            assert (got_mean[M:] == -5.0).all() and (got_var[M:] == -5.0).all()
    else:
        got_s, got_a = hip_cem_sample(mean, var, lb, ub, pop, seed=9, counter=4)
    assert np.array_equal(got_a, ref_a) and np.array_equal(got_s, ref_s)
    if not device_count:
        got_m, got_v = hip_cem_update(ref_s, costs, mean, var, ne, 0.1, active=ref_a)
    assert np.array_equal(got_m, ref_m) and np.array_equal(got_v, ref_v)
    assert np.array_equal(got_m[M // 2], mean[M // 2])      # inactive env untouched


@pytest.mark.parametrize("case", ("mid", "edge"))
def test_cem_update_kernel_matches_reference_iteration(G, case):
    pre = "cem." + case + "."
    m, v = hip_cem_update(G[pre + "samples"][None], G[pre + "costs"][None], G[pre + "init_mean"][None],
                          G[pre + "init_var"][None], int(G["cem.num_elites"]), float(G["cem.alpha"]))
    assert np.allclose(m[0], G[pre + "new_mean"], rtol=1e-5, atol=1e-6)
    assert np.allclose(v[0], G[pre + "new_var"], rtol=1e-4, atol=1e-7)


def test_cem_optimizer_minimises_a_quadratic_for_many_problems():
    M, dim = 64, 10
    target = torch.rand(M, 1, dim, device=DEV, generator=torch.Generator(device=DEV).manual_seed(0)) * 1.6 - 0.8
    opt = CEMOptimizer(dim, max_iters=8, popsize=400, num_elites=40,
                       cost_function=lambda s: ((s - target) ** 2).sum(-1), upper_bound=np.ones(dim),
                       lower_bound=-np.ones(dim), alpha=0.1, device=DEV, seed=3)
    sol = opt.obtain_solution(torch.zeros(M, dim, dtype=torch.float64, device=DEV),
                              torch.full((M, dim), 0.25, dtype=torch.float64, device=DEV))
    assert sol.shape == (M, dim) and (sol - target.squeeze(1)).abs().max() < 0.08
    assert int(opt.tick[0].item()) == 8
    with pytest.raises(ValueError):
        CEMOptimizer(dim, 5, 10, 11, None, np.ones(dim), -np.ones(dim), device=DEV)
    one = opt.obtain_solution(np.zeros(dim), np.full(dim, 0.25))
    assert isinstance(one, np.ndarray) and one.shape == (dim,)


def build_mpc(n_envs=1, mb_dynamics="model"):
    env = make_vec_env("navigation2", n_envs, device=DEV, seed=1)
    cfg = create_config("navigation2", "MPC", {}, [], "/tmp", env=env)
    return env, MPC(cfg.ctrl_cfg, mb_dynamics=mb_dynamics, seed=1)


def test_compile_cost_matches_reference(G):
    """G7c: same ensemble weights, Q_risk weights, action sequences and injected particle noise."""
    env, mpc = build_mpc()
    sd = {k[3:]: T(G[k]) for k in G.files if k.startswith("pt.") and k[3:] in mpc.model.state_dict()}
    mpc.model.load_state_dict(sd, strict=True)
    mpc.model.inputs_mu.data = T(G["pt.fit_mu"])
    mpc.model.inputs_sigma.data = T(G["pt.fit_sigma"])
    args = arg_utils.get_args(["--env-name", "navigation2", "--hidden_size", "16", "--cuda", "--use_recovery",
                               "--gamma_safe", "0.65", "--eps_safe", "0.2"])
    agent = SAC(env.observation_space, env.action_space, args, "/tmp")
    qsd = {k[len("cc.qrisk."):]: T(G[k]) for k in G.files if k.startswith("cc.qrisk.")}
    agent.safety_critic.safety_critic.load_state_dict(qsd, strict=True)
    mpc.update_value_func(agent.safety_critic)
    noises = [T(n) for n in G["cc.noise"]]
    real = torch.randn_like
    torch.randn_like = lambda t, **k: noises.pop(0)
    try:
        costs = mpc._compile_cost(T(G["cc.ac_seqs"])[None], T(G["cc.cur_obs"], np.float32)[None])
    finally:
        torch.randn_like = real
    assert costs.shape == (1, 6)
    assert np.allclose(costs[0].cpu().numpy(), G["cc.costs"], rtol=2e-4, atol=1e-5)


def test_untrained_controller_returns_uniform_actions_and_train_fits_dynamics():
    env, mpc = build_mpc(n_envs=8)
    a = mpc.act(env.reset(), 0)
    assert a.shape == (8, 2) and (a.abs() <= 1).all() and not mpc.has_been_trained
    # transitions of the true dynamics: s' = s + a + 0.05 eps
    g = torch.Generator(device=DEV).manual_seed(0)
    s = torch.rand(4000, 2, device=DEV, generator=g) * torch.tensor([40.0, 30.0], device=DEV) - \
        torch.tensor([45.0, 15.0], device=DEV)
    ac = torch.rand(4000, 2, device=DEV, generator=g) * 2 - 1
    s2 = s + ac + 0.05 * torch.randn(4000, 2, device=DEV, generator=g)
    mse = mpc.train(s, ac, random=True, next_obs=s2, epochs=6, progress=True)
    assert mpc.has_been_trained and mpc.train_in.shape == (4000, 4) and mpc.train_targs.shape == (4000, 2)
    assert float(mse.max()) < 0.05                           # learned delta = a (+ noise var 0.0025)
    # incremental call with trajectories appends obs[:-1], acs -> obs[1:] - obs[:-1]
    traj_o, traj_a = torch.cumsum(torch.ones(6, 2, device=DEV), 0), torch.ones(5, 2, device=DEV)
    mpc.train([traj_o], [traj_a], epochs=1)
    assert mpc.train_in.shape == (4005, 4)
    assert torch.equal(mpc.train_targs[-5:], torch.ones(5, 2, device=DEV))


@pytest.mark.parametrize("mb_dynamics", ("model", "env"))
def test_batched_planning_steers_away_from_the_obstacle(mb_dynamics):
    """Envs left of the box (navigation2.py:41) heading right: a value function that is high inside
    the box makes the planner choose actions with a negative x component."""
    env, mpc = build_mpc(n_envs=16, mb_dynamics=mb_dynamics)
    g = torch.Generator(device=DEV).manual_seed(1)
    s = torch.rand(6000, 2, device=DEV, generator=g) * torch.tensor([30.0, 30.0], device=DEV) - \
        torch.tensor([45.0, 15.0], device=DEV)
    ac = torch.rand(6000, 2, device=DEV, generator=g) * 2 - 1
    mpc.train(s, ac, random=True, next_obs=s + ac, epochs=8)

    class BoxRisk:
        def get_value(self, states, actions, encoded=False):
            nxt = states + actions
            inside = (nxt[:, 0] >= -31.5) & (nxt[:, 0] <= -20) & (nxt[:, 1].abs() <= 7.5)
            return inside.float().unsqueeze(1)
    mpc.update_value_func(BoxRisk())
    obs = torch.tensor([[-32.0, 0.0]], device=DEV).repeat(16, 1)
    mask = torch.zeros(16, dtype=torch.bool, device=DEV)
    mask[::2] = True
    act = mpc.act(obs, 0, mask=mask)
    assert act.shape == (16, 2)
    assert (act[1::2] == 0).all()                            # rows outside the mask are not planned
    assert (act[::2, 0] < 0.3).all() and act[::2, 0].mean() < 0
    assert not torch.equal(mpc.prev_sol[0], mpc.prev_sol[1])  # planned rows shifted their warm start
    assert torch.equal(mpc.prev_sol[1], torch.zeros(10, dtype=torch.float64, device=DEV))


def test_graph_replayed_training_step_equals_the_eager_loop():
    """MPC.train replays the optimiser step from a hipGraph (same kernels, same order): identical weights."""
    import time
    g = torch.Generator(device=DEV).manual_seed(3)
    s = torch.rand(1500, 2, device=DEV, generator=g) * 20 - 10
    ac = torch.rand(1500, 2, device=DEV, generator=g) * 2 - 1
    s2 = s + ac + 0.05 * torch.randn(1500, 2, device=DEV, generator=g)
    out = {}
    for graph in (True, False):
        torch.manual_seed(11)
        env, mpc = build_mpc()
        mpc.graph_train, mpc.fused_train = graph, False
        torch.manual_seed(12)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        mpc.train(s, ac, random=True, next_obs=s2, epochs=4)
        torch.cuda.synchronize()
        out[graph] = ({k: v.clone() for k, v in mpc.model.state_dict().items()}, time.perf_counter() - t0)
    for k in out[True][0]:
        assert torch.equal(out[True][0][k], out[False][0][k]), k
    print("train 4 epochs x 47 batches: graph %.3f s, eager %.3f s" % (out[True][1], out[False][1]))


def test_fused_training_kernel_fits_like_the_pytorch_loop():
    """MPC.train through rrl_ens_train_grad + rrl_adam_step_multi (default for the reference's shapes) against the
    PyTorch loop on the same data, bootstrap indices and epochs: same fit quality, faster."""
    import time
    g = torch.Generator(device=DEV).manual_seed(3)
    s = torch.rand(3000, 2, device=DEV, generator=g) * 20 - 10
    ac = torch.rand(3000, 2, device=DEV, generator=g) * 2 - 1
    s2 = s + ac + 0.05 * torch.randn(3000, 2, device=DEV, generator=g)
    out = {}
    for fused in (True, False):
        torch.manual_seed(11)
        env, mpc = build_mpc()
        mpc.fused_train = fused
        torch.manual_seed(12)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        mse = mpc.train(s, ac, random=True, next_obs=s2, epochs=6, progress=True)
        torch.cuda.synchronize()
        out[fused] = (mse.clone(), time.perf_counter() - t0, mpc)
    assert out[True][2]._trainer is not None and out[False][2]._trainer is None
    assert float(out[True][0].max()) < 0.05 and float(out[False][0].max()) < 0.05
    torch.testing.assert_close(out[True][0], out[False][0], rtol=0.3, atol=5e-3)
    print("train 6 epochs x 94 batches: fused %.3f s, graph replay %.3f s" % (out[True][1], out[False][1]))
