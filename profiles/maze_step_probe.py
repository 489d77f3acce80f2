"""Latency of the fused step + push kernel at 4096 envs, Maze next to Navigation 1, with and without auto-reset and with
zero actions (Maze: no move -> no collision search).  HIP events around a captured graph of 200 launches."""
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from recovery_rl_amd import _lib  # noqa: E402
from recovery_rl_amd.env import make_vec_env  # noqa: E402
from recovery_rl_amd.replay_memory import ConstraintReplayMemory, ReplayMemory  # noqa: E402

dev = torch.device("cuda:0")
lib = _lib.load()
n = int(sys.argv[1]) if len(sys.argv) > 1 else 4096


def time_case(env_name, auto_reset, zero_action, with_rmem=True):
    env = make_vec_env(env_name, n, device=dev, seed=1)
    env.reset()
    hi = float(env.action_space.high[0])
    act = (torch.rand(n, 2, device=dev) * 2 - 1) * hi
    if zero_action:
        act.zero_()
    real = act.clone()
    rec = torch.zeros(n, dtype=torch.uint8, device=dev)
    mem, rmem = ReplayMemory(1000000, 1, device=dev), ConstraintReplayMemory(1000000, 1, device=dev)
    stats = torch.zeros(10, dtype=torch.int64, device=dev)
    sums = torch.zeros(2, dtype=torch.float64, device=dev)
    ep_reward = torch.zeros(n, device=dev)
    p = _lib.ptr
    a = _lib.rrl_step_push_t()
    a.n, a.pos, a.t, a.obs = n, p(env.pos), p(env.t), p(env.obs)
    a.task_action, a.ld_task, a.real_action, a.recovery = p(act), 2, p(real), p(rec)
    a.seed, a.counter, a.counter_dev, a.counter_inc = env.seed_value, 0, p(env.tick), 1
    a.horizon, a.auto_reset, a.reward_penalty, a.push_real_action = env.horizon, int(auto_reset), 0.0, 0
    a.memory, a.recovery_memory = C.pointer(mem._desc), C.pointer(rmem._desc) if with_rmem else None
    a.next_obs, a.reward = p(env.next_obs), p(env.reward)
    a.done, a.constraint, a.success, a.ep_done = p(env.done), p(env.constraint), p(env.success), p(env.ep_done)
    a.stats, a.reward_sums, a.ep_reward = p(stats), p(sums), p(ep_reward)

    def launch():
        if env_name == "maze":
            return lib.rrl_maze_step_push_x(C.byref(a), _lib.current_stream())
        return lib.rrl_nav_step_push_x(env.kind, C.byref(a), _lib.current_stream())
    for _ in range(10):
        assert launch() == 0
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(200):
            launch()
    g.replay()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    g.replay()
    e1.record()
    torch.cuda.synchronize()
    return round(e0.elapsed_time(e1) * 1e3 / 200, 2)


out = {"n": n}
for env_name in ("navigation1", "maze"):
    for auto in (1, 0):
        for zero in (0, 1):
            out["%s_auto%d_zero%d_us" % (env_name, auto, zero)] = time_case(env_name, auto, zero)
    out["%s_no_safety_buffer_us" % env_name] = time_case(env_name, 1, 0, with_rmem=False)
print(json.dumps(out, indent=1))
