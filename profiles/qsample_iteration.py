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
network) and against the rows executed with the padding of the last chunk to 16-row tiles.

    python profiles/qsample_iteration.py --packed [--seeds 2,4,8] [--out profiles/packed_qsample.json]

Seed packing of this line (RRL_PACK_QSAMPLE=1: the gate evaluated inside the qsample call, the call as one
rrl_qsample_act_packed stage): the captured iteration at eps_safe = 1 (nothing gated) and -1 (everything gated), the two
shares that are exact under graph replay -- the parent's path solo (RRL_FAST_QSAMPLE=1 alone), the gated form solo, and the
packed iteration of S seeds, as a multiple of S parent-path solo iterations.  Legs with their own learners, alternated in one
process; the realised share is recorded per round."""
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


def build(path, envs, dev, seed=1):
    """One loop on `path`: hip = RRL_FAST_QSAMPLE=1 (read when the loop is built), modules = the switch unset."""
    cfg = arg_utils.get_args(["--env-name", "navigation1", "--cuda", "--gamma_safe", "0.8", "--eps_safe", "0.3", "--hidden_size",
                              "256", "--num_envs", str(envs), "--seed", str(seed), "--num_unsafe_transitions", "4000",
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


class gate_in_launch:
    """RRL_PACK_QSAMPLE for the loops built inside the block (VectorLoop reads it once, when it is built)."""

    def __init__(self, on):
        self.on = on

    def __enter__(self):
        self.saved = os.environ.pop("RRL_PACK_QSAMPLE", None)
        if self.on:
            os.environ["RRL_PACK_QSAMPLE"] = "1"

    def __exit__(self, *exc):
        os.environ.pop("RRL_PACK_QSAMPLE", None)
        if self.saved is not None:
            os.environ["RRL_PACK_QSAMPLE"] = self.saved


def packed_main(a):
    from recovery_rl_amd.packed import PackedLoop
    dev = torch.device("cuda:0")
    seeds = [int(x) for x in a.seeds.split(",")]
    with gate_in_launch(False):
        parent = build("hip", a.envs, dev)
    with gate_in_launch(True):
        gated = build("hip", a.envs, dev)
        members = [build("hip", a.envs, dev, seed=1 + s) for s in range(max(seeds))]
    assert not parent.qsample_gated and gated.qsample_gated and all(m.qsample_gated for m in members)
    share_of = lambda loop: float(loop._last_recovery.float().mean())
    res = {}
    for name, eps in (("0", 1.0), ("1", -1.0)):
        for loop in [parent, gated] + members:
            loop.cfg.eps_safe = eps
        parent.capture(online_qrisk=True)
        gated.capture(online_qrisk=True)
        out = {"eps_safe": eps, "parent_solo_ms": [], "parent_solo_share": [], "gated_solo_ms": [], "gated_solo_share": []}
        for S in seeds:
            packed = PackedLoop(members[:S], online_qrisk=True)
            packed.capture()
            kinds = [op[0] for op in packed.tapes[0]]
            assert kinds.count("qsample") == 1 and "unsupported" not in kinds
            key = "packed_S%d" % S
            out[key + "_ms"], out[key + "_share"], out[key + "_launches"] = [], [], packed.launches
            for _ in range(a.rounds):                  # alternating with the two solo legs
                out["parent_solo_ms"].append(time_it(parent.replay, a.iters))
                out["parent_solo_share"].append(share_of(parent))
                out["gated_solo_ms"].append(time_it(gated.replay, a.iters))
                out["gated_solo_share"].append(share_of(gated))
                out[key + "_ms"].append(time_it(packed.replay, a.iters))
                out[key + "_share"].append([share_of(loop) for loop in packed.loops])
            packed.close()
        solo = sorted(out["parent_solo_ms"])[len(out["parent_solo_ms"]) // 2]
        out["parent_solo_median_ms"] = solo
        out["parent_solo_spread"] = (max(out["parent_solo_ms"]) - min(out["parent_solo_ms"])) / solo
        out["gated_solo_over_parent"] = sorted(out["gated_solo_ms"])[len(out["gated_solo_ms"]) // 2] / solo
        for S in seeds:
            ms = sorted(out["packed_S%d_ms" % S])[a.rounds // 2]
            out["packed_S%d_over_S_solo" % S] = ms / (S * solo)
            out["packed_S%d_env_steps_per_s" % S] = S * a.envs / ms * 1e3
        res[name] = json.loads(json.dumps(out), parse_float=lambda x: round(float(x), 4))
        print(name, json.dumps(res[name]), flush=True)
    res["setup"] = {"envs_per_seed": a.envs, "hidden": 256, "batch": 256, "k": K, "iters": a.iters, "rounds": a.rounds,
                    "seeds": seeds, "device": torch.cuda.get_device_name(0)}
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--packed", action="store_true")
    ap.add_argument("--seeds", default="2,4,8")
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.packed:
        return packed_main(a)
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
