"""Seed packing for the comparison algorithms (LR, RSPO, RCPO, SAC without a recovery policy): the three packed entry points
against their stand-alone twins bit for bit, every packed seed against its solo run, and the driver."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import arg_utils
import bench
from recovery_rl_amd import _lib
from recovery_rl_amd import packed as packed_module
from recovery_rl_amd.experiment import uses_constraint_buffer
from recovery_rl_amd.packed import PackedLoop
from recovery_rl_amd.utils import linear_schedule
from test_packed_gpu import state_of

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
P = C.POINTER


def gen(seed):
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    return g


def randn(g, *shape):
    return torch.randn(*shape, device=DEV, generator=g)


def stream():
    return _lib.current_stream()


# ---- 1. entry points against their stand-alone twins ---------------------------------------------------------------------
@pytest.mark.parametrize("S", (1, 3, 16))
def test_packed_penalty_equals_the_stand_alone_launches(S):
    lib, g, p = _lib.load(), gen(100 + S), _lib.ptr
    seeds = []
    for s in range(S):
        B, n_part = (8, 200, 256, 300)[s % 4], (1, 4)[(s // 2) % 2]
        z = randn(g, n_part, 2, B) * 2
        lam = torch.rand(1, device=DEV, generator=g) * 10 + 0.5
        want_penalty = s % 3 != 1                                       # some seeds: the mean-only form
        outs = [(torch.full((B,), -7.0, device=DEV), torch.full((1,), -7.0, device=DEV)) for _ in range(2)]
        seeds.append((B, n_part, z, lam, want_penalty, outs))
    args = (_lib.rrl_penalty_args_t * S)()
    for s, (B, n_part, z, lam, want, outs) in enumerate(seeds):
        pen, mean = outs[0]
        args[s] = _lib.rrl_penalty_args_t(B, p(z), n_part, z.stride(0), p(lam) if want else None, p(pen) if want else None, p(mean))
        pen, mean = outs[1]
        solo = _lib.rrl_penalty_args_t(B, p(z), n_part, z.stride(0), p(lam) if want else None, p(pen) if want else None, p(mean))
        assert lib.rrl_rcpo_penalty(solo, stream()) == 0
    assert lib.rrl_rcpo_penalty_packed(S, args, stream()) == 0
    torch.cuda.synchronize()
    for s, (B, n_part, z, lam, want, outs) in enumerate(seeds):
        assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1]), s
        assert float(outs[0][1]) != -7.0 and (float(outs[0][0][0]) != -7.0) == want, s
    lib.rrl_pack_clear()


ROWS = (1, 255, 257, 1056)


def head_member(g, kind, B, variant):
    """Inputs of one policy head and a function (output buffers) -> rrl_policy_head_t; variant picks the optional outputs."""
    p = _lib.ptr
    n_part = (1, 4, 2)[variant % 3]
    width = 4 if kind == _lib.HEAD_GAUSS else 2
    head = randn(g, n_part, B, width)
    eps, scale, bias = randn(g, B, 2), torch.rand(2, device=DEV, generator=g) + 0.5, randn(g, 2) * 0.1
    obs_in, log_std = randn(g, B, 2), randn(g, 2)
    with_logp, with_obs, with_mean, with_eps = variant % 2 == 0, variant % 4 >= 2, variant % 3 == 0, variant % 5 != 4

    def outputs():
        return {"xa": torch.full((B, 4), -7.0, device=DEV), "logp": torch.full((B,), -7.0, device=DEV),
                "mean": torch.full((B, 2), -7.0, device=DEV), "act2": torch.full((B, 2), -7.0, device=DEV)}

    def desc(o):
        if kind == _lib.HEAD_GAUSS:
            action = o["xa"][:, 2:4] if with_obs else o["act2"]
            return _lib.rrl_policy_head_t(kind, B, p(head), n_part, head.stride(0), p(eps), p(scale), p(bias), p(action),
                                          action.stride(0), p(o["logp"]) if with_logp else None,
                                          p(o["mean"]) if with_mean else None, p(obs_in) if with_obs else None,
                                          p(o["xa"]) if with_obs else None, None, 0.0)
        return _lib.rrl_policy_head_t(kind, B, p(head), n_part, head.stride(0), p(eps) if with_eps else None, p(scale), p(bias),
                                      p(o["act2"]), 2, None, p(o["mean"]) if with_mean else None, None, None, p(log_std), -1.5)
    keep = (head, eps, scale, bias, obs_in, log_std)
    return outputs, desc, keep


@pytest.mark.parametrize("S", (1, 3, 16))
def test_packed_policy_heads_equal_the_stand_alone_launches(S):
    lib, g = _lib.load(), gen(200 + S)
    solo_out, pack_out, arrays, counts, keep = [], [], [], [], []
    j = 0
    for s in range(S):
        n = 1 + (s + S) % 4                                           # 1 .. 4 members, differing by seed
        members = []
        for k in range(n):
            kind = (_lib.HEAD_GAUSS, _lib.HEAD_STOCH)[(s + k) % 2]
            members.append(head_member(g, kind, ROWS[j % 4], j))
            j += 1
        a, b = [m[0]() for m in members], [m[0]() for m in members]
        solo_arr = (_lib.rrl_policy_head_t * n)(*[m[1](o) for m, o in zip(members, a)])
        pack_arr = (_lib.rrl_policy_head_t * n)(*[m[1](o) for m, o in zip(members, b)])
        assert lib.rrl_policy_heads_fwd_multi(n, solo_arr, stream()) == 0
        solo_out.append(a), pack_out.append(b), arrays.append(pack_arr), counts.append(n), keep.append(members)
    n_arr = (C.c_int * S)(*counts)
    ptrs = (P(_lib.rrl_policy_head_t) * S)(*[C.cast(a, P(_lib.rrl_policy_head_t)) for a in arrays])
    assert lib.rrl_policy_heads_fwd_multi_packed(S, n_arr, ptrs, stream()) == 0
    torch.cuda.synchronize()
    written = 0
    for s in range(S):
        for a, b in zip(solo_out[s], pack_out[s]):
            for key in a:
                assert torch.equal(a[key], b[key]), (s, key)
                written += int((b[key] != -7.0).any())
    assert written >= sum(counts)                                     # every member wrote its actions at least
    assert len({c for c in counts}) > 1 or S == 1
    lib.rrl_pack_clear()


N_SEG = 134658            # the twin critics' parameter count at hidden width 256: n % 4 == 2, two float4 slots per thread and a tail


class DualSeed:
    """One seed's arguments of rrl_adam_step_multi_duals: n_seg segments with a Polyak target, n_dual dual members."""

    def __init__(self, g, n_seg, n_dual, stat_only):
        self.t = {}
        z = lambda n: torch.zeros(n, device=DEV)
        for k in range(n_seg):
            self.t.update({"p%d" % k: randn(g, N_SEG) * 0.1, "g%d" % k: randn(g, N_SEG) * 0.01, "m%d" % k: z(N_SEG),
                           "v%d" % k: z(N_SEG), "target%d" % k: randn(g, N_SEG) * 0.1,
                           "step%d" % k: torch.zeros(2, dtype=torch.int64, device=DEV)})
        for j in range(n_dual):
            self.t.update({"log_p%d" % j: randn(g, 1), "exp_avg%d" % j: z(1), "exp_avg_sq%d" % j: z(1), "dstep%d" % j: z(1),
                           "value%d" % j: z(1), "stat%d" % j: torch.rand(1, device=DEV, generator=g),
                           "loss_in%d" % j: randn(g, 1), "loss_out%d" % j: z(1)})
        self.n_seg, self.n_dual, self.stat_only = n_seg, n_dual, stat_only

    def clone(self):
        other = DualSeed.__new__(DualSeed)
        other.t = {k: v.clone() for k, v in self.t.items()}
        other.n_seg, other.n_dual, other.stat_only = self.n_seg, self.n_dual, self.stat_only
        return other

    def descs(self):
        t, p = self.t, _lib.ptr
        segs = (_lib.rrl_adam_seg_t * max(self.n_seg, 1))()
        for k in range(self.n_seg):
            segs[k] = _lib.rrl_adam_seg_t(N_SEG, p(t["p%d" % k]), p(t["g%d" % k]), p(t["m%d" % k]), p(t["v%d" % k]),
                                          p(t["step%d" % k]), p(t["target%d" % k]), 0.005, 0.0, None, None, 0, 0, 0, None, None,
                                          0, 0)
        duals = (_lib.rrl_dual_t * self.n_dual)()
        for j in range(self.n_dual):
            d = _lib.rrl_dual_t(stat=p(t["stat%d" % j]), eps_safe=0.3, lr=3e-5)
            if j == self.n_dual - 1 and self.stat_only:       # RSPO's member: a statistic and no step
                d.loss_in, d.loss_out, d.f_loss = p(t["loss_in%d" % j]), p(t["loss_out%d" % j]), 50.0
            else:
                d.log_p, d.exp_avg, d.exp_avg_sq, d.step = (p(t["log_p%d" % j]), p(t["exp_avg%d" % j]),
                                                            p(t["exp_avg_sq%d" % j]), p(t["dstep%d" % j]))
                d.value = p(t["value%d" % j])
                if j == 0:
                    d.loss_in, d.loss_out, d.f_loss = p(t["loss_in%d" % j]), p(t["loss_out%d" % j]), 5000.0
            duals[j] = d
        return segs, duals


@pytest.mark.parametrize("S,n_segs", [(1, 2), (3, 2), (9, 2), (3, 0), (3, None)])     # None: seeds differ, one without segments
def test_packed_dual_step_equals_the_stand_alone_launches(S, n_segs):
    lib, g = _lib.load(), gen(300 + S)
    solo, pack = [], []
    for s in range(S):
        n_seg = n_segs if n_segs is not None else (2, 0, 1)[s % 3]
        seed = DualSeed(g, n_seg, n_dual=1 + s % 2 if S > 1 else 2, stat_only=s % 3 == 1 or S == 1)
        solo.append(seed), pack.append(seed.clone())
    lr = [3e-4 * (1 + s) for s in range(S)]
    b1, b2, eps = 0.9, 0.999, 1e-8
    solo_d, pack_d = [x.descs() for x in solo], [x.descs() for x in pack]
    n_seg = (C.c_int * S)(*[x.n_seg for x in pack])
    n_dual = (C.c_int * S)(*[x.n_dual for x in pack])
    segs = (P(_lib.rrl_adam_seg_t) * S)(*[C.cast(d[0], P(_lib.rrl_adam_seg_t)) if x.n_seg else P(_lib.rrl_adam_seg_t)()
                                          for d, x in zip(pack_d, pack)])
    duals = (P(_lib.rrl_dual_t) * S)(*[C.cast(d[1], P(_lib.rrl_dual_t)) for d in pack_d])
    lrs = (C.c_float * S)(*lr)
    for step in range(3):
        for s in range(S):
            assert lib.rrl_adam_step_multi_duals(solo[s].n_seg, solo_d[s][0] if solo[s].n_seg else None, solo[s].n_dual,
                                                 solo_d[s][1], lrs[s], b1, b2, eps, stream()) == 0
        assert lib.rrl_adam_step_multi_duals_packed(S, n_seg, segs, n_dual, duals, lrs, b1, b2, eps, stream()) == 0
    torch.cuda.synchronize()
    for s in range(S):
        for key in solo[s].t:
            assert torch.equal(solo[s].t[key], pack[s].t[key]), (s, key)
        t = pack[s].t
        for k in range(pack[s].n_seg):
            assert t["step%d" % k].tolist() == [3, 0] and float(t["m%d" % k].abs().max()) > 0
        for j in range(pack[s].n_dual):
            stepped = not (j == pack[s].n_dual - 1 and pack[s].stat_only)
            assert float(t["dstep%d" % j]) == (3.0 if stepped else 0.0), (s, j)
            if stepped:
                assert float(t["value%d" % j]) == pytest.approx(float(torch.exp(t["log_p%d" % j])), rel=1e-6)
            else:
                assert float(t["loss_out%d" % j]) != 0.0 and float(t["exp_avg%d" % j]) == 0.0
    assert any(x.stat_only for x in pack)
    lib.rrl_pack_clear()


def test_new_packed_entry_points_validate_before_launching():
    lib = _lib.load()
    one = (C.c_int * 1)(1)
    g = gen(7)
    seed = DualSeed(g, 1, 1, False)
    segs, duals = seed.descs()
    sp = (P(_lib.rrl_adam_seg_t) * 1)(C.cast(segs, P(_lib.rrl_adam_seg_t)))
    dp = (P(_lib.rrl_dual_t) * 1)(C.cast(duals, P(_lib.rrl_dual_t)))
    lr = (C.c_float * 1)(3e-4)
    before = {k: v.clone() for k, v in seed.t.items()}
    for S in (0, 17):
        assert lib.rrl_adam_step_multi_duals_packed(S, one, sp, one, dp, lr, 0.9, 0.999, 1e-8, stream()) != 0
        assert lib.rrl_rcpo_penalty_packed(S, (_lib.rrl_penalty_args_t * 1)(), stream()) != 0
        assert lib.rrl_policy_heads_fwd_multi_packed(S, one, (P(_lib.rrl_policy_head_t) * 1)(), stream()) != 0
    assert lib.rrl_adam_step_multi_duals_packed(1, None, sp, one, dp, lr, 0.9, 0.999, 1e-8, stream()) != 0
    assert lib.rrl_adam_step_multi_duals_packed(1, one, None, one, dp, lr, 0.9, 0.999, 1e-8, stream()) != 0
    assert lib.rrl_adam_step_multi_duals_packed(1, one, sp, None, dp, lr, 0.9, 0.999, 1e-8, stream()) != 0
    assert lib.rrl_adam_step_multi_duals_packed(1, one, sp, one, None, lr, 0.9, 0.999, 1e-8, stream()) != 0
    assert lib.rrl_adam_step_multi_duals_packed(1, one, sp, one, dp, None, 0.9, 0.999, 1e-8, stream()) != 0
    assert lib.rrl_rcpo_penalty_packed(2, None, stream()) != 0
    assert lib.rrl_policy_heads_fwd_multi_packed(2, None, None, stream()) != 0
    assert lib.rrl_policy_heads_fwd_multi_packed(2, (C.c_int * 2)(1, 1), None, stream()) != 0
    # a bad second seed refuses the whole call: nothing of the first seed is launched
    two = (C.c_int * 2)(1, 1)
    bad = (_lib.rrl_dual_t * 1)(_lib.rrl_dual_t())                      # no statistic
    dp2 = (P(_lib.rrl_dual_t) * 2)(C.cast(duals, P(_lib.rrl_dual_t)), C.cast(bad, P(_lib.rrl_dual_t)))
    sp2 = (P(_lib.rrl_adam_seg_t) * 2)(sp[0], sp[0])
    assert lib.rrl_adam_step_multi_duals_packed(2, two, sp2, two, dp2, (C.c_float * 2)(3e-4, 3e-4), 0.9, 0.999, 1e-8,
                                                stream()) != 0
    pen = (_lib.rrl_penalty_args_t * 2)()
    z, mean = torch.zeros(2, 8, device=DEV), torch.full((1,), -7.0, device=DEV)
    pen[0] = _lib.rrl_penalty_args_t(8, _lib.ptr(z), 1, 0, None, None, _lib.ptr(mean))
    pen[1] = _lib.rrl_penalty_args_t(8, _lib.ptr(z), 5, 0, None, None, _lib.ptr(mean))        # n_part out of range
    assert lib.rrl_rcpo_penalty_packed(2, pen, stream()) != 0
    torch.cuda.synchronize()
    assert float(mean) == -7.0
    for k, v in before.items():
        assert torch.equal(v, seed.t[k]), k


# ---- 2. every packed seed equals its solo run -----------------------------------------------------------------------------
LINES = {"SAC": [], "LR": ["--DGD_constraints", "--nu", "50", "--update_nu"], "RCPO": ["--RCPO", "--lambda_RCPO", "10"],
         "RSPO": ["--DGD_constraints", "--nu_schedule", "--nu_start", "10000", "--num_eps", "400"]}


def make_loop(line, recovery, seed, n_envs=128):
    argv = bench.config_argv("navigation1", seed, n_envs, 1) + ["--num_unsafe_transitions", "3000"] + LINES[line]
    if not recovery:
        argv = [a for a in argv if a not in ("--use_recovery", "--MF_recovery")]
    cfg = arg_utils.get_args(argv)
    loop = bench.build_loop(cfg, DEV, pretrain=10)
    if cfg.nu_schedule:       # the multiplier the driver's lock-step loop uses throughout: nu_schedule(1)
        loop.nu_schedule = linear_schedule(cfg.nu_start, cfg.nu_end, cfg.num_eps)
    return loop


def duals_of(loop):
    ag, out = loop.agent, {}
    for name, opt, prm, val in (("nu", ag.nu_optim, ag.log_nu, ag.nu), ("lambda", ag.lambda_RCPO_optim, ag.log_lambda_RCPO,
                                                                      ag.lambda_RCPO)):
        out["log_" + name] = prm.detach().clone()
        out[name] = torch.as_tensor(val, dtype=torch.float32, device=DEV).detach().clone()
        for k, v in opt.state.get(prm, {}).items():
            out["%s.%s" % (name, k)] = v.detach().clone()
    out["dual_stats"] = ag.fast.dual_stats.clone()
    return out


@pytest.mark.parametrize("line,recovery,S", [("SAC", False, 3), ("LR", False, 3), ("RCPO", False, 3), ("RSPO", False, 3),
                                             ("LR", True, 3), ("LR", False, 9)])      # 9: block-form backward, no W2 copy
def test_every_packed_baseline_seed_equals_its_solo_run(line, recovery, S):
    K = 9
    loops = [make_loop(line, recovery, 1 + s) for s in range(S)]
    online = bool(uses_constraint_buffer(loops[0].cfg))
    assert online == (line != "SAC" or recovery)
    first = duals_of(loops[0])
    packed = PackedLoop(loops, online_qrisk=online)
    done = packed.capture()
    kinds = [op[0] for op in packed.tapes[0]]
    assert "unsupported" not in kinds
    assert kinds.count("adam_duals") == (0 if line == "SAC" else 1) and kinds.count("penalty") == (1 if line == "RCPO" else 0)
    assert kinds.count("heads") == (0 if recovery else 1) and kinds.count("step") == 1
    packed.replay()                  # one single iteration,
    packed.advance(4)                # one four-iteration graph,
    for _ in range(K - 5):           # then singles
        packed.replay()
    assert packed.graph_many_iters == 4 and packed.graph_many is not None
    torch.cuda.synchronize()
    got = [dict(state_of(l), **duals_of(l)) for l in packed.loops]
    stats = packed.read_stats()
    packed.close()
    del packed, loops
    updates = done + K
    for s in range(S):
        solo = make_loop(line, recovery, 1 + s)
        for _ in range(updates):
            solo.vector_step(True, False, online)
        torch.cuda.synchronize()
        want = dict(state_of(solo), **duals_of(solo))
        assert set(want) == set(got[s])
        for k in want:
            assert torch.equal(got[s][k], want[k]), (line, s, k)
        st = solo.read_stats()
        assert st == stats[s] and st["sac_updates"] == updates and st["qrisk_updates"] == (updates if online else 0)
        assert int(solo.agent.fast.critic.step[0].item()) == updates
    for name, stepped in (("nu", line == "LR"), ("lambda", line == "RCPO")):
        if stepped:
            assert float(got[0][name + ".step"]) == updates
            assert not torch.equal(got[0]["log_" + name], first["log_" + name])
        else:
            assert name + ".step" not in got[0] and torch.equal(got[0]["log_" + name], first["log_" + name])
    # the seeds are different learners
    assert not torch.equal(got[0]["critic.flat"], got[1]["critic.flat"]) and not torch.equal(got[0]["pos"], got[1]["pos"])
    assert all(bool(torch.isfinite(v.float()).all()) for v in got[0].values())


# ---- 3. the driver ---------------------------------------------------------------------------------------------------------
def test_seeds_per_gpu_runs_the_lr_line_packed(tmp_path, monkeypatch, capsys):
    """`rrl_main --seeds_per_gpu 2` on the LR line: two experiments (own log directories) advanced by one shared graph; the
    second one's counters and log-multiplier equal the solo run of that seed stepped through the same phases."""
    from recovery_rl_amd.experiment import Experiment, run_packed
    monkeypatch.setenv("RRL_FAST_BASELINES", "1")
    made = []

    class Spy(PackedLoop):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            made.append(self)
    monkeypatch.setattr(packed_module, "PackedLoop", Spy)
    argv = ["--env-name", "navigation1", "--cuda", "--DGD_constraints", "--nu", "5000", "--update_nu", "--gamma_safe", "0.8",
            "--eps_safe", "0.3", "--num_unsafe_transitions", "3000", "--critic_safe_pretraining_steps", "30", "--num_envs",
            "128", "--log_every", "20", "--num_eps", "100000", "--num_steps", str(128 * 40 - 1)]
    hists = run_packed(arg_utils.get_args(argv + ["--seed", "4", "--seeds_per_gpu", "2", "--logdir", str(tmp_path / "packed")]))
    assert len(hists) == 2 and all(h[-1]["iteration"] == 40 and h[-1]["env_steps"] == 40 * 128 for h in hists)
    dirs = sorted(os.listdir(tmp_path / "packed"))
    assert len(dirs) == 2 and dirs[0].endswith("_seed4") and dirs[1].endswith("_seed5")
    assert len(made) == 1 and made[0].S == 2 and made[0].graph is not None
    assert "unsupported" not in [op[0] for op in made[0].tapes[0]]
    assert hists[0][-1]["sac_updates"] > 30 and hists[0][-1] != hists[1][-1]
    log_nu = made[0].loops[1].agent.log_nu.detach().clone()
    solo_cfg = arg_utils.get_args(argv + ["--seed", "5", "--logdir", str(tmp_path / "solo")])
    solo = Experiment(solo_cfg)
    assert solo.agent.fast is not None
    solo.pretrain_critic_recovery()
    loop = solo.loop
    loop.start()
    for _ in range(40):
        loop.vector_step(do_update=len(solo.memory) > solo_cfg.batch_size,
                         random_actions=solo_cfg.start_steps > loop.total_numsteps, online_qrisk=solo.online_qrisk_enabled())
    want = loop.read_stats()
    got = {k: v for k, v in hists[1][-1].items() if k != "iteration"}
    assert got == want
    assert torch.equal(log_nu, solo.agent.log_nu.detach())
    assert float(log_nu) != float(np.log(5000.0).astype(np.float32))
