"""Draw-ahead: the task batch's keys are selected one env step early (rrl_draw_select / rrl_fwd_riders_t.select) and the draw
launch is dissolved into the first policy forward (rrl_mlp3_forward_riders).  Same Philox arguments and the same ring size give
the same keys, the gather reads the same slots after the same pushes, every tick advances once per draw: everything is
bit-identical to the stand-alone draw, which is what these tests assert -- no tolerance anywhere."""
import ctypes as C

import pytest
import torch

import arg_utils
from recovery_rl_amd import _lib, checkpoint
from recovery_rl_amd.replay_memory import ReplayMemory

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B = 256


def _rows(n, gen):
    f = lambda *s: torch.rand(*s, generator=gen, device=DEV, dtype=torch.float32)
    return f(n, 2), f(n, 2), f(n), f(n, 2), f(n)


def _select(mem, rows_ahead, batch=B):
    d, _ = mem.draw_desc(batch, ahead=rows_ahead)
    sel = _lib.rrl_draw_ahead_t(C.pointer(d), rows_ahead, _lib.ptr(mem.ahead_keys(batch)))
    _lib.check(_lib.load().rrl_draw_select(C.byref(sel), _lib.current_stream()), "rrl_draw_select")
    return mem.ahead_keys(batch)


def _policy_stack(gen, M):
    """A one-head 2 -> 256 -> 256 -> 4 stack (the task policy's shape) as a hand-made rrl_stack_t."""
    f = lambda *s: (torch.rand(*s, generator=gen, device=DEV, dtype=torch.float32) - 0.5) * 0.2
    t = {"W1": f(1, 256, 2), "b1": f(1, 256), "W2": f(1, 256, 256), "b2": f(1, 256), "W3": f(1, 4, 256), "b3": f(1, 4),
         "out": torch.zeros(1, M, 4, device=DEV), "scratch": torch.zeros(4, 1, M, 4, device=DEV),
         "x": torch.zeros(M, 4, device=DEV)}
    p = _lib.ptr
    desc = _lib.rrl_stack_t(1, M, 256, 2, 4, 4, p(t["x"]), p(t["W1"]), p(t["b1"]), p(t["W2"]), p(t["b2"]), p(t["W3"]),
                            p(t["b3"]), None, None, p(t["out"]), p(t["scratch"]), _lib.rrl_policy_head_t(), 0, None)
    return desc, t


# ring capacity, rows before the push, rows pushed: filling / wrapping inside this very push / full before and after
RINGS = {"filling": (10000, 1000, 500), "wraps_in_this_push": (1200, 1000, 500), "full": (1000, 1000, 500)}


@pytest.mark.parametrize("ring", sorted(RINGS))
def test_keys_selected_before_a_push_are_the_draws_indices_after_it(ring):
    """Select (rows_ahead = n) -> push n rows -> stand-alone draw: the draw's idx ARE the keys, and selecting moved neither
    the tick nor the error flag.  Then the gather half (a rider of a 2B-row policy forward that reads its rows through the
    keys) leaves the batch, the tick and the forward's output of the stand-alone draw + forward."""
    cap, before, n = RINGS[ring]
    gen = torch.Generator(device=DEV).manual_seed(11)
    mems = [ReplayMemory(cap, 5, device=DEV) for _ in range(2)]
    first, pushed = _rows(before, gen), _rows(n, gen)
    for m in mems:
        m.push(*first)
        m.sample(B)                                   # a tick other than zero
    ahead, alone = mems
    tick0, state0 = ahead.tick.clone(), ahead.state.clone()
    keys = _select(ahead, n).clone()
    assert torch.equal(ahead.tick, tick0) and torch.equal(ahead.state, state0)
    for m in mems:
        m.push(*pushed)
    rows = [tuple(torch.zeros(B, 4, device=DEV) for _ in range(3)) for _ in range(2)]
    alone.sample(B, rows=rows[1])
    idx = alone._batch(B)[5]
    assert torch.equal(keys[:B].to(torch.int64), idx)
    assert int(keys[B + 4]) == 0 and int(keys[B + 2]) == min(cap, before + n)
    # the gather half + the keyed forward against the stand-alone draw + the plain forward
    desc_k, tk = _policy_stack(torch.Generator(device=DEV).manual_seed(3), 2 * B)
    desc_p, tp = _policy_stack(torch.Generator(device=DEV).manual_seed(3), 2 * B)
    d, batch = ahead.draw_desc(B, rows=(rows[0][0], tk["x"][:B], tk["x"][B:]))
    gat = _lib.rrl_draw_ahead_t(C.pointer(d), 0, _lib.ptr(ahead.ahead_keys(B)))
    riders = _lib.rrl_fwd_riders_t(None, C.pointer(gat), None, 0, 0, 0, None, 0, None)
    lib = _lib.load()
    _lib.check(lib.rrl_mlp3_forward_riders(C.byref(desc_k), C.byref(riders), _lib.current_stream()), "riders")
    tp["x"][:B, 0:2] = alone._batch(B)[3]
    tp["x"][B:, 0:2] = alone._batch(B)[0]
    _lib.check(lib.rrl_mlp3_forward_multi(1, C.byref(desc_p), _lib.current_stream()), "forward")
    torch.cuda.synchronize()
    assert torch.equal(ahead.tick, alone.tick) and torch.equal(ahead.state, alone.state)
    for x, y in zip(ahead._batch(B), alone._batch(B)):
        assert torch.equal(x, y)
    assert torch.equal(rows[0][0], rows[1][0])
    assert torch.equal(tk["x"][:, 0:2], tp["x"][:, 0:2])
    assert torch.equal(tk["scratch"], tp["scratch"])


def test_a_batch_larger_than_the_ring_after_the_push_raises_the_draws_flag():
    """B > size': the select half records it, the gather half raises flag 1 (random.sample's ValueError) without advancing
    the tick -- what the stand-alone draw does; keys drawn for another tick are refused with flag 4."""
    gen = torch.Generator(device=DEV).manual_seed(2)
    ahead, alone = (ReplayMemory(4096, 5, device=DEV) for _ in range(2))
    first, pushed = _rows(100, gen), _rows(100, gen)
    for m in (ahead, alone):
        m.push(*first)
        m._len = 4096                                 # the host-side check is not what is tested here
    keys = _select(ahead, 100)
    assert int(keys[B + 4]) == 1 and int(ahead.state[3]) == 0
    for m in (ahead, alone):
        m.push(*pushed)
        m._len = 4096
    desc, t = _policy_stack(gen, 2 * B)

    def gather(mem):
        d, _ = mem.draw_desc(B)
        gat = _lib.rrl_draw_ahead_t(C.pointer(d), 0, _lib.ptr(mem.ahead_keys(B)))
        riders = _lib.rrl_fwd_riders_t(None, C.pointer(gat), None, 0, 0, 0, None, 0, None)
        _lib.check(_lib.load().rrl_mlp3_forward_riders(C.byref(desc), C.byref(riders), _lib.current_stream()), "riders")
    gather(ahead)
    alone.sample(B)
    assert int(ahead.state[3]) == int(alone.state[3]) == 1 and torch.equal(ahead.tick, alone.tick)
    with pytest.raises(ValueError):
        ahead.check_error()
    # stale keys: drawn at this tick, used after another draw moved it
    big = ReplayMemory(4096, 5, device=DEV)
    big.push(*_rows(1000, gen))
    _select(big, 0)
    big.sample(B)
    gather(big)
    assert int(big.state[3]) == 4


# ---- the loop ----------------------------------------------------------------------------------------------------------
def _loop(tmp_path, ahead, updates_per_step=1, seed=7):
    import bench
    cfg = arg_utils.get_args(bench.config_argv("navigation1", seed, 4096, updates_per_step) +
                             ["--num_unsafe_transitions", "3000", "--logdir", str(tmp_path)])
    loop = bench.build_loop(cfg, torch.device(DEV), pretrain=10)
    loop.draw_ahead = ahead
    return loop


def _state(loop):
    """Everything the iteration writes: both rings, env state, counters, every tick, parameters, moments, targets, losses."""
    torch.cuda.synchronize()
    env, fast = loop.env, loop.agent.fast
    if hasattr(env, "refresh_arrays"):
        env.refresh_arrays()
    out = {"env.pos": env.pos, "env.obs": env.obs, "env.t": env.t, "env.flags": env._flags, "env.tick": env.tick,
           "stats": loop.stats, "reward_sums": loop.reward_sums, "ep_reward": loop.ep_reward,
           "noise_tick": fast.noise_tick, "losses": fast.losses}
    for name, m in (("memory", loop.memory), ("recovery_memory", loop.recovery_memory)):
        for f in ("s", "a", "r", "s2", "m", "state", "tick"):
            out[name + "." + f] = getattr(m, f)
    for name in ("critic", "critic_target", "policy", "qrisk", "qrisk_target", "recpolicy"):
        net = getattr(fast, name)
        for f in ("flat", "m", "v", "step"):
            out[name + "." + f] = getattr(net, f)
    out = {k: v.clone() for k, v in out.items()}
    out["host"] = (loop.total_numsteps, loop.updates, tuple(loop.host_updates), len(loop.memory), len(loop.recovery_memory))
    return out


def _assert_same(a, b):
    assert set(a) == set(b)
    bad = [k for k in a if not (torch.equal(a[k], b[k]) if torch.is_tensor(a[k]) else a[k] == b[k])]
    assert not bad, bad


def _run(loop, mode, iters=13):
    if mode == "eager":
        for _ in range(iters):
            loop.vector_step(True, False, True)
    else:
        done = loop.capture(online_qrisk=True, iters=1 if mode == "graph1" else None)
        loop.advance(iters - done)


@pytest.mark.parametrize("mode", ("eager", "graph1", "graph4"))
def test_loop_with_keys_drawn_ahead_equals_the_loop_without(tmp_path, mode):
    states = []
    for ahead in (True, False):
        loop = _loop(tmp_path, ahead)
        _run(loop, mode)
        if ahead:
            # the path under test ran: keys are pending for the next iteration, and the graphs replay the keyed iteration
            assert loop.memory.ahead.ready(B) and loop.agent.fast.keyed
            assert mode == "eager" or loop._graph_ahead
        else:
            assert loop.memory.ahead.pending is None and not loop.agent.fast.keyed
        states.append(_state(loop))
    _assert_same(*states)


def test_two_update_pairs_per_iteration_keep_the_stand_alone_draws(tmp_path):
    states = []
    for ahead in (True, False):
        loop = _loop(tmp_path, ahead, updates_per_step=2)
        _run(loop, "graph4")
        assert loop.memory.ahead.pending is None
        states.append(_state(loop))
    _assert_same(*states)


def test_log_point_and_checkpoint_in_the_middle_see_and_restore_the_switch_off_state(tmp_path):
    """After 6 iterations: a log point (read_stats) and a checkpoint of everything; the run goes on from the graphs, a second
    run resumes from the checkpoint.  The checkpoint equals the switch-off run's at that point (pending keys are not state:
    no tick moved for them), and both continuations end where the switch-off run ends."""
    def snap(loop):
        return {"memory": checkpoint.replay_state(loop.memory), "recovery_memory": checkpoint.replay_state(loop.recovery_memory),
                "env": checkpoint.env_state(loop.env), "agent": checkpoint.agent_state(loop.agent),
                "loop": checkpoint.loop_state(loop)}
    mids, ends = [], []
    for ahead in (True, False):
        loop = _loop(tmp_path, ahead)
        for _ in range(6):
            loop.vector_step(True, False, True)
        loop.read_stats()
        mids.append((snap(loop), _state(loop)))
        for _ in range(6):
            loop.vector_step(True, False, True)
        ends.append(_state(loop))
    _assert_same(mids[0][1], mids[1][1])
    _assert_same(*ends)
    resumed = _loop(tmp_path, True)
    sd = mids[0][0]
    checkpoint.load_replay_state(resumed.memory, sd["memory"])
    checkpoint.load_replay_state(resumed.recovery_memory, sd["recovery_memory"])
    resumed.memory._len, resumed.recovery_memory._len = sd["memory"]["size"], sd["recovery_memory"]["size"]
    checkpoint.load_env_state(resumed.env, sd["env"])
    checkpoint.load_agent_state(resumed.agent, sd["agent"])
    checkpoint.load_loop_state(resumed, sd["loop"])
    assert resumed.memory.ahead.pending is None
    for _ in range(6):
        resumed.vector_step(True, False, True)
    assert resumed.agent.fast.keyed
    _assert_same(_state(resumed), ends[1])


@pytest.mark.parametrize("touch", ("push", "sample"))
@pytest.mark.parametrize("mode", ("eager", "graph4"))
def test_an_eager_push_or_sample_between_two_iterations_drops_the_pending_keys(tmp_path, touch, mode):
    gen = torch.Generator(device=DEV).manual_seed(9)
    extra = _rows(300, gen)
    states = []
    for ahead in (True, False):
        loop = _loop(tmp_path, ahead)
        _run(loop, mode, iters=7)
        assert loop.memory.ahead.ready(B) == ahead
        if touch == "push":
            loop.memory.push(*extra)
        else:
            loop.memory.sample(B)
        assert loop.memory.ahead.pending is None
        if mode == "eager":
            for _ in range(6):
                loop.vector_step(True, False, True)
        else:
            loop.advance(6)
        assert loop.memory.ahead.ready(B) == ahead
        states.append(_state(loop))
    _assert_same(*states)
