"""Q-sampling recovery (--use_recovery --Q_sampling_recovery) at 4096 envs, hidden 256, k = 1000: the acting pass on the
rrl_qsample_act kernels (RRL_FAST_QSAMPLE=1, the `hip` leg) against the module path (QRiskWrapper.select_action on all n x 1000
rows, gated or not), the two legs alternated in one process, at gated shares 0, 1/64, 1/8 and 1.

    python profiles/qsample_iteration.py [--iters 30] [--rounds 3] [--out profiles/qsample_act.json]

Two measurements per share:
  * the acting launches alone, back to back between two HIP events: rrl_qsample_act (both kernels) on a mask with exactly
    round(share n) envs gated, spread evenly -- and what the module path runs in its place, select_action on the n
    observations plus the torch.where that merges its result (its cost does not depend on the share);
  * the captured iteration (hipGraph replay, one update per iteration, online Q_risk update) with eps_safe set to the
    quantile of Q_risk(obs, task action) that gates that share when the graph is captured (0: eps_safe = 1, 1: eps_safe = -1);
    the share the timed replays really gated is recorded beside the time (the envs move and Q_risk trains).
Rates are against the FLOPs the algorithm needs for the GATED rows (267 264 per candidate row of the twin 4-256-256-1
network) and against the rows executed with the padding of the last chunk to 16-row tiles."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import arg_utils  # noqa: E402
import bench  # noqa: E402

Q_FLOP_PER_ROW = 2 * (2 * 4 * 256 + 2 * 256 * 256 + 2 * 256)     # the twin Q_risk heads on one candidate row: 267 264
K = 1000
SHARES = (("0", 0.0), ("1/64", 1.0 / 64), ("1/8", 1.0 / 8), ("1", 1.0))


def time_it(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e3


def build(path, envs, dev):
    """One loop on `path`: hip = RRL_FAST_QSAMPLE=1 (read when the loop is built), modules = the switch unset."""
    cfg = arg_utils.get_args(["--env-name", "navigation1", "--cuda", "--gamma_safe", "0.8", "--eps_safe", "0.3", "--hidden_size",
                              "256", "--num_envs", str(envs), "--seed", "1", "--num_unsafe_transitions", "4000",
                              "--use_recovery", "--Q_sampling_recovery"])
    saved = os.environ.pop("RRL_FAST_QSAMPLE", None)
    if path == "hip":
        os.environ["RRL_FAST_QSAMPLE"] = "1"
    try:
        loop = bench.build_loop(cfg, dev, fast=True, pretrain=5)
    finally:
        os.environ.pop("RRL_FAST_QSAMPLE", None)
        if saved is not None:
            os.environ["RRL_FAST_QSAMPLE"] = saved
    assert loop.qsample_hip == (path == "hip")
    for _ in range(5):
        loop.vector_step(True, False, True)
    return loop


def events_ms(fn, launches, rounds):
    out = []
    for _ in range(rounds + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(launches):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / launches)
    return out[1:]                                     # the first round warms up


def acting_legs(loops, share, launches, rounds):
    """(hip ms per call, modules ms per call, gated envs): the acting launches alone at an exact share."""
    from recovery_rl_amd import _lib
    hip, mod = loops["hip"], loops["modules"]
    n = hip.n
    gated = int(round(share * n))
    mask = torch.zeros(n, dtype=torch.uint8, device=hip.device)
    if gated:
        mask[torch.linspace(0, n - 1, gated, device=hip.device).round().long()] = 1
    assert int(mask.sum()) == gated
    actor, lib, st = hip.qsample_actor(), _lib.load(), _lib.current_stream()
    a = type(actor._qsample_args).from_buffer_copy(actor._qsample_args)
    a.mask = mask.data_ptr()
    qr, obs, task = mod.agent.safety_critic, mod.obs, torch.zeros(n, 2, device=mod.device)
    m = mask.bool().unsqueeze(1)
    out = {"hip": [], "modules": []}
    for _ in range(rounds):                            # alternating
        # (a window of comparable length at every share: more calls where few envs are gated)
        out["hip"] += events_ms(lambda: _lib.check(lib.rrl_qsample_act(C.byref(a), st), "rrl_qsample_act"),
                                launches * (1 if 8 * gated >= n else 16), 1)
        out["modules"] += events_ms(lambda: torch.where(m, qr.select_action(obs), task), max(2, launches // 5), 1)
    return out["hip"], out["modules"], gated


def set_share(loop, share):
    """eps_safe of the loop such that about `share` of its envs are gated on their current observations."""
    if share <= 0.0:
        eps = 1.0
    elif share >= 1.0:
        eps = -1.0
    else:
        with torch.no_grad():
            action = loop.agent.policy.sample(loop.obs)[0]
            q = loop.agent.safety_critic.get_value(loop.obs, action).squeeze(1)
            eps = float(torch.quantile(q, 1.0 - share))
    loop.cfg.eps_safe = eps
    return eps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    paths = ("hip", "modules")
    loops = {path: build(path, a.envs, dev) for path in paths}
    res = {}
    for name, share in SHARES:
        hip_ms, mod_ms, gated = acting_legs(loops, share, a.launches, a.rounds)
        rows = gated * K
        padded = gated * 16 * ((K + 15) // 16)
        ms = min(hip_ms)
        out = {"gated_envs": gated, "acting_hip_ms": hip_ms, "acting_modules_ms": mod_ms,
               "acting_hip": {"ms_best": ms, "gflop_needed": rows * Q_FLOP_PER_ROW / 1e9,
                              "tflops_needed": rows * Q_FLOP_PER_ROW / ms / 1e9,
                              "tflops_executed": padded * Q_FLOP_PER_ROW / ms / 1e9, "f32_mfma_peak_tflops": 157.3},
               "acting_modules": {"ms_best": min(mod_ms), "gflop_executed": a.envs * K * Q_FLOP_PER_ROW / 1e9}}
        for path in paths:
            out[path + "_eps_safe"] = set_share(loops[path], share)
            loops[path].capture(online_qrisk=True)
            out[path + "_graph_ms"], out[path + "_gated_share"] = [], []
        for _ in range(a.rounds):                      # alternating
            for path in paths:
                out[path + "_graph_ms"].append(time_it(loops[path].replay, a.iters))
                out[path + "_gated_share"].append(float(loops[path]._last_recovery.float().mean()))
        res[name] = json.loads(json.dumps(out), parse_float=lambda x: round(float(x), 4))
        print(name, json.dumps(res[name]), flush=True)
    res["setup"] = {"envs": a.envs, "hidden": 256, "batch": 256, "k": K, "iters": a.iters, "rounds": a.rounds,
                    "launches": a.launches, "device": torch.cuda.get_device_name(0)}
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
