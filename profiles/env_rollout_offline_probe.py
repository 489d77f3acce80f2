"""Launch times of the env kernels that profiles/nav_step_probe.py does not reach: the open-loop rollout (rrl_nav_rollout,
both kinds) and the maze's offline constraint data (rrl_maze_offline).  HIP events around 20 launches each, best of 3
rounds, one JSON object.
    python profiles/env_rollout_offline_probe.py"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from recovery_rl_amd import _lib  # noqa: E402

dev = torch.device("cuda:0")
lib = _lib.load()
p = _lib.ptr


def timeit(f, reps=20):
    assert f() == 0
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        f()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


n, T = 1 << 20, 8
pos = torch.zeros(n, 2, dtype=torch.float64, device=dev)
pos[:, 0] = -50.0
acts = torch.rand(T, n, 2, device=dev) * 2 - 1
obs = torch.zeros(T, n, 2, device=dev)
rew = torch.zeros(T, n, device=dev)
cons = torch.zeros(T, n, dtype=torch.uint8, device=dev)
done = torch.zeros(T, n, dtype=torch.uint8, device=dev)
num = 1 << 22
s, a, s2 = (torch.zeros(num, 2, device=dev) for _ in range(3))
c, m = torch.zeros(num, device=dev), torch.zeros(num, device=dev)


def rollout(kind):
    return lambda: lib.rrl_nav_rollout(kind, n, T, p(pos), p(acts), 1, 0, None, p(obs), p(rew), p(cons), p(done),
                                       _lib.current_stream())


cases = [("nav1_rollout_2^20x8", rollout(0)), ("nav2_rollout_2^20x8", rollout(1)),
         ("maze_offline_2^22", lambda: lib.rrl_maze_offline(num, 1, p(s), p(a), p(c), p(s2), p(m), num, _lib.current_stream()))]
out = {}
for rnd in range(3):
    for name, f in cases:
        out[name + "_us"] = round(min(timeit(f), out.get(name + "_us", 1e9)), 1)
print(json.dumps(out, indent=1))
