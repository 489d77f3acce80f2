"""Seed packing for SQRL (RRL_PACK_SQRL=1): rrl_sqrl_act_packed against its stand-alone twin bit for bit -- every mapping of
the packed grid, seeds that differ in everything but k -- a bad seed refusing the whole call, every packed SQRL seed against
its solo run, and the driver."""
import functools
import os
import pickle
import types

import numpy as np
import pytest
import torch

import arg_utils
import bench
from recovery_rl_amd import _lib
from recovery_rl_amd import packed as packed_module
from recovery_rl_amd.packed import PackedLoop
from test_packed_baselines_gpu import duals_of
from test_packed_gpu import state_of
from test_sqrl_act_cpu import KS, MODES, PHILOX_SEED, SQRL, case, draws, make_agent
from test_sqrl_act_gpu import DIAG, buffers, launch, same

pytestmark = pytest.mark.gpu
DEV = "cuda"
EINVAL, ERANGE = -1, -3
SEED_NS = (65, 1, 3)                    # envs of seed s: SEED_NS[s % 3] -- more than one wave of workgroups, one, a few


@pytest.fixture(scope="module")
def rig():
    """The weights of tests/test_sqrl_act_gpu.py and a second Q_risk: a seeded perturbation, its W2 re-packed in fragment order."""
    agent = make_agent(DEV)
    fast = agent.enable_fast_path(256)
    g = torch.Generator(device=DEV).manual_seed(77)
    p2 = {name: (t + 0.05 * torch.randn(t.shape, device=DEV, generator=g)).contiguous() for name, t in fast.qrisk.p.items()}
    w2p = torch.empty_like(fast.qrisk.w2_packed())
    W2 = p2["W2"]
    _lib.check(_lib.load().rrl_w2_pack(W2.shape[0], W2.shape[1], W2.data_ptr(), w2p.data_ptr(), _lib.current_stream()), "w2_pack")
    other = types.SimpleNamespace(qrisk=types.SimpleNamespace(p=p2, w2_packed=lambda: w2p), scale=fast.scale, bias=fast.bias)
    torch.cuda.synchronize()
    assert not torch.equal(w2p, fast.qrisk.w2_packed())
    cases = functools.lru_cache(maxsize=None)(lambda n, k: case(agent, n, k, device=DEV))     # one per shape, shared
    return cases, (fast, other)


def seed_inputs(cases, nets, s, k):
    """Seed s of a call: its own env count, weights, Philox seed, device tick, threshold, head partials and diagnostics."""
    n = SEED_NS[s % 3]
    c = cases(n, k)
    head, n_part, stride = c["head"], 1, 0
    if s % 2:                            # the head as two partial sums
        g = torch.Generator(device=DEV).manual_seed(500 + s)
        r = torch.randn(n, 4, device=DEV, generator=g) * 0.3
        head = torch.stack([0.5 * c["head"] + r, 0.5 * c["head"] - r]).contiguous()
        n_part, stride = 2, head.stride(0)
    return types.SimpleNamespace(n=n, k=k, fast=nets[(s // 2) % 2], obs=c["obs"], head=head, n_part=n_part, stride=stride,
                                 thr=c["thr"][MODES[s % 3]], seed=PHILOX_SEED + 7919 * s, t0=1000 + 17 * s,
                                 diag=s % 3 != 2)                       # every third seed asks for no diagnostic


def outputs(x):
    out = buffers(x.n, x.k)              # poisoned: an element the kernel does not write shows
    return out if x.diag else {"action": out["action"]}


def tick_of(x):
    return torch.tensor([x.t0, 0], dtype=torch.int64, device=DEV)


def descriptor(x, tick, out):
    """Seed x's stand-alone descriptor, as FastActor.act_sqrl builds it."""
    p, P = _lib.ptr, x.fast.qrisk.p
    return _lib.rrl_sqrl_act_t(n=x.n, k=x.k, H=256, d_obs=2, d_act=2, obs=p(x.obs), head=p(x.head), n_part=x.n_part,
                               part_stride=x.stride, scale=p(x.fast.scale), bias=p(x.fast.bias), W1=p(P["W1"]), b1=p(P["b1"]),
                               W2p=p(x.fast.qrisk.w2_packed()), b2=p(P["b2"]), W3=p(P["W3"]), b3=p(P["b3"]),
                               eps_safe=float(x.thr), seed=x.seed, counter=0, counter_dev=p(tick), counter_inc=1,
                               **{name: p(t) for name, t in out.items()})


def pack(xs, ticks, outs):
    return (_lib.rrl_sqrl_act_t * len(xs))(*[descriptor(x, t, o) for x, t, o in zip(xs, ticks, outs)])


def solo(x, tick, **kw):
    return launch(x.fast, x.obs, x.head, x.k, x.thr, n_part=x.n_part, part_stride=x.stride, seed=x.seed, tick=tick,
                  out=outputs(x), **kw)


# S: the solo path, pinned with p = 4, pinned with padding workgroups (three seeds on four XCD groups), the linear mapping,
# pinned with p = 1 -- and, beyond what PackedLoop packs, the entry point's own limit: two seeds taking turns on every XCD
@pytest.mark.parametrize("S,k", [(1, 100), (2, 17), (3, 100), (5, 128), (8, 100), (16, 17)])
def test_packed_equals_stand_alone_bit_for_bit(rig, S, k):
    cases, nets = rig
    assert k in KS
    lib = _lib.load()
    xs = [seed_inputs(cases, nets, s, k) for s in range(S)]
    assert S == 1 or (len({x.n for x in xs}) > 1 and len({x.n_part for x in xs}) > 1 and len({x.thr for x in xs}) > 1)
    assert S < 3 or (len({id(x.fast) for x in xs}) == 2 and len({x.diag for x in xs}) == 2)
    # every seed alone, twice
    want = []
    for x in xs:
        tick = tick_of(x)
        first, second = solo(x, tick), solo(x, tick)
        assert tick.tolist() == [x.t0 + 2, 0]
        assert not torch.equal(first["action"], second["action"])       # the second launch drew at the next tick
        want.append((first, second))
    # the pack, twice, on clones of the ticks
    ticks = [tick_of(x) for x in xs]
    got = [outputs(x) for x in xs], [outputs(x) for x in xs]
    for outs in got:
        assert lib.rrl_sqrl_act_packed(S, pack(xs, ticks, outs), _lib.current_stream()) == 0
    torch.cuda.synchronize()
    for s, x in enumerate(xs):
        assert set(got[0][s]) == set(want[s][0]) == (set(DIAG) | {"action"} if x.diag else {"action"})
        assert same(got[0][s], want[s][0]) and same(got[1][s], want[s][1]), s
        assert ticks[s].tolist() == [x.t0 + 2, 0], s                    # the seed's own tick, advanced by its own workgroups
        assert not any(bool(torch.isnan(t).any()) for t in got[0][s].values() if t.is_floating_point())
    # a hipGraph holding the packed launch, replayed twice from the initial ticks
    outs = [outputs(x) for x in xs]
    args = pack(xs, ticks, outs)
    if S == 2:                                   # a block the library has not seen cannot be built inside a capture
        g = torch.cuda.CUDAGraph()
        with pytest.raises(_lib.RRLError, match="capturing"):
            with torch.cuda.graph(g):
                _lib.check(lib.rrl_sqrl_act_packed(S, args, _lib.current_stream()), "rrl_sqrl_act_packed")
        del g
        torch.cuda.synchronize()
    assert lib.rrl_sqrl_act_packed(S, args, _lib.current_stream()) == 0          # (eager once: the block is cached)
    for s, x in enumerate(xs):
        ticks[s].copy_(tick_of(x))
        for name, t in outs[s].items():
            t.copy_(outputs(x)[name])
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        _lib.check(lib.rrl_sqrl_act_packed(S, args, _lib.current_stream()), "rrl_sqrl_act_packed")
    assert all(t.tolist() == [x.t0, 0] for t, x in zip(ticks, xs))              # the capture executed nothing
    for turn in (0, 1):
        g.replay()
        torch.cuda.synchronize()
        for s in range(S):
            assert same(outs[s], want[s][turn]), (turn, s)
    assert all(t.tolist() == [x.t0 + 2, 0] for t, x in zip(ticks, xs))
    del g
    # one seed's packed output is what the oracle's draws for ITS seed and tick give a stand-alone launch
    s = max(i for i, x in enumerate(xs) if x.diag)
    x = xs[s]
    eps, u = draws(x.n, k, x.seed, x.t0)
    inj = solo(x, None, eps=torch.as_tensor(eps, device=DEV), u=torch.as_tensor(u, device=DEV))
    assert same(inj, got[0][s])
    if S > 1:                                    # ... and not what another seed's stream gives
        eps, u = draws(x.n, k, xs[0].seed, xs[0].t0)
        assert not same(solo(x, None, eps=torch.as_tensor(eps, device=DEV), u=torch.as_tensor(u, device=DEV)), got[0][s])
    lib.rrl_pack_clear()


def test_a_bad_seed_refuses_the_whole_call_on_the_device(rig):
    cases, nets = rig
    lib, S = _lib.load(), 3
    xs = [seed_inputs(cases, nets, s, 100) for s in range(S)]
    ticks, outs = [tick_of(x) for x in xs], [outputs(x) for x in xs]
    lib.rrl_pack_clear()
    for at, fields, code in ((2, dict(W2p=xs[2].fast.qrisk.w2_packed().data_ptr() + 8), EINVAL), (2, dict(H=32), EINVAL),
                             (1, dict(head=None), EINVAL), (2, dict(k=129), ERANGE), (2, dict(k=96), EINVAL), (0, dict(k=17), EINVAL)):
        args = pack(xs, ticks, outs)
        for name, v in fields.items():
            setattr(args[at], name, v)
        assert lib.rrl_sqrl_act_packed(S, args, _lib.current_stream()) == code, fields
    assert lib.rrl_sqrl_act_packed(0, pack(xs, ticks, outs), _lib.current_stream()) == EINVAL
    assert lib.rrl_sqrl_act_packed(S, None, _lib.current_stream()) == EINVAL
    torch.cuda.synchronize()
    for s, x in enumerate(xs):
        assert ticks[s].tolist() == [x.t0, 0], s
        for name, t in outs[s].items():          # still poisoned: NaN / -77 everywhere
            assert bool((torch.isnan(t) if t.is_floating_point() else t == -77).all()), (s, name)
    assert lib.rrl_pack_clear() == 0             # nothing was stored either


# ---- every packed SQRL seed equals its solo run ------------------------------------------------------------------------------
def make_loop(seed, n_envs=128):
    argv = bench.config_argv("navigation1", seed, n_envs, 1) + ["--num_unsafe_transitions", "3000"] + SQRL
    argv = [a for a in argv if a not in ("--use_recovery", "--MF_recovery")]
    return bench.build_loop(arg_utils.get_args(argv), DEV, pretrain=10)


def full_state(loop):
    return dict(state_of(loop), **duals_of(loop), sqrl_tick=loop.sqrl_actor().sqrl_tick.clone())


@pytest.mark.parametrize("S", (3, 8))
def test_every_packed_sqrl_seed_equals_its_solo_run(monkeypatch, S):
    monkeypatch.setenv("RRL_FAST_BASELINES", "1")
    monkeypatch.setenv("RRL_FAST_SQRL", "1")
    K = 9
    loops = [make_loop(1 + s) for s in range(S)]
    assert all(l.sqrl_hip and int(l.cfg.hidden_size) == 256 and not l.cfg.use_recovery for l in loops)
    first = duals_of(loops[0])
    packed = PackedLoop(loops, online_qrisk=True)
    done = packed.capture()
    kinds = [op[0] for op in packed.tapes[0]]
    assert "unsupported" not in kinds
    assert kinds.count("sqrl") == 1 and kinds.count("heads") == 0 and kinds.count("step") == 1 and kinds.count("adam_duals") == 1
    assert [st[0] for st in packed.stages if st[2][0][0] == "sqrl"] == [packed.lib.rrl_sqrl_act_packed]
    packed.replay()                  # one single iteration,
    packed.advance(4)                # one four-iteration graph,
    for _ in range(K - 5):           # then singles
        packed.replay()
    assert packed.graph_many_iters == 4 and packed.graph_many is not None
    torch.cuda.synchronize()
    got = [full_state(l) for l in packed.loops]
    stats = packed.read_stats()
    packed.close()
    del packed, loops
    updates = done + K
    for s in range(S):
        ref = make_loop(1 + s)
        for _ in range(updates):
            ref.vector_step(True, False, True)
        torch.cuda.synchronize()
        want = full_state(ref)
        assert set(want) == set(got[s])
        for k in want:
            assert torch.equal(got[s][k], want[k]), (s, k)
        st = ref.read_stats()
        assert st == stats[s] and st["sac_updates"] == updates and st["qrisk_updates"] == updates
        # one tick per iteration that did not act at random: every iteration since build_loop's random-action phase
        assert got[s]["sqrl_tick"].tolist() == [updates, 0]
    assert float(got[0]["nu.step"]) == updates and not torch.equal(got[0]["log_nu"], first["log_nu"])
    # the seeds are different learners
    assert not torch.equal(got[0]["critic.flat"], got[1]["critic.flat"]) and not torch.equal(got[0]["pos"], got[1]["pos"])
    assert not torch.equal(got[0]["qrisk.flat"], got[1]["qrisk.flat"])
    assert all(bool(torch.isfinite(v.float()).all()) for v in got[0].values())


def test_packed_loop_refuses_nine_sqrl_loops(monkeypatch):
    monkeypatch.setenv("RRL_FAST_BASELINES", "1")
    monkeypatch.setenv("RRL_FAST_SQRL", "1")
    loop = make_loop(1)
    with pytest.raises(ValueError, match="at most 8 seeds"):
        PackedLoop([loop] * 9, online_qrisk=True)
    assert loop.agent.fast.qrisk.w2p is not None          # refused before any net gave up its fragment-order copy


# ---- the driver ----------------------------------------------------------------------------------------------------------------
def test_seeds_per_gpu_runs_the_sqrl_line_packed(tmp_path, monkeypatch, capsys):
    """`rrl_main --seeds_per_gpu 2` on the SQRL line under the three switches: two experiments (own log directories) advanced
    by one shared graph whose acting launch is rrl_sqrl_act_packed; the second one's counters and log-multiplier equal the solo
    run of that seed stepped through the same phases."""
    from recovery_rl_amd.experiment import Experiment, run_packed
    for name in ("RRL_FAST_BASELINES", "RRL_FAST_SQRL", "RRL_PACK_SQRL"):
        monkeypatch.setenv(name, "1")
    made = []

    class Spy(PackedLoop):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            made.append(self)
    monkeypatch.setattr(packed_module, "PackedLoop", Spy)
    argv = ["--env-name", "navigation1", "--cuda"] + SQRL + ["--gamma_safe", "0.8",
            "--eps_safe", "0.3", "--num_unsafe_transitions", "3000", "--critic_safe_pretraining_steps", "30", "--num_envs",
            "128", "--log_every", "20", "--num_eps", "100000", "--num_steps", str(128 * 40 - 1)]
    hists = run_packed(arg_utils.get_args(argv + ["--seed", "4", "--seeds_per_gpu", "2", "--logdir", str(tmp_path / "packed")]))
    assert len(hists) == 2 and all(h[-1]["iteration"] == 40 and h[-1]["env_steps"] == 40 * 128 for h in hists)
    dirs = sorted(os.listdir(tmp_path / "packed"))
    assert len(dirs) == 2 and dirs[0].endswith("_seed4") and dirs[1].endswith("_seed5")
    assert len(made) == 1 and made[0].S == 2 and made[0].graph is not None           # one captured graph
    kinds = [op[0] for op in made[0].tapes[0]]
    assert "unsupported" not in kinds and kinds.count("sqrl") == 1
    for d in dirs:
        rs = pickle.load(open(os.path.join(tmp_path / "packed", d, "run_stats.pkl"), "rb"))
        assert rs["vector_rules"]["sqrl_acting"] == "hip" and rs["seeds_per_gpu"] == 2
    assert hists[0][-1]["sac_updates"] > 30 and hists[0][-1] != hists[1][-1]
    log_nu = made[0].loops[1].agent.log_nu.detach().clone()
    tick = made[0].loops[1].sqrl_actor().sqrl_tick.clone()
    solo_cfg = arg_utils.get_args(argv + ["--seed", "5", "--logdir", str(tmp_path / "solo")])
    ref = Experiment(solo_cfg)
    assert ref.agent.fast is not None and ref.loop.sqrl_hip
    ref.pretrain_critic_recovery()
    loop = ref.loop
    loop.start()
    for _ in range(40):
        loop.vector_step(do_update=len(ref.memory) > solo_cfg.batch_size,
                         random_actions=solo_cfg.start_steps > loop.total_numsteps, online_qrisk=ref.online_qrisk_enabled())
    want = loop.read_stats()
    got = {k: v for k, v in hists[1][-1].items() if k != "iteration"}
    assert got == want
    assert torch.equal(log_nu, ref.agent.log_nu.detach())
    assert torch.equal(tick, loop.sqrl_actor().sqrl_tick) and int(tick[0]) > 30
    assert float(log_nu) != float(np.log(5000.0).astype(np.float32))
