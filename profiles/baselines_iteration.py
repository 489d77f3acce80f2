"""Milliseconds per lock-step iteration of the comparison lines of scripts/navigation1.sh (LR, RSPO, SQRL, RCPO) at
4096 envs, hidden 256, batch 256: the fused update path (what RRL_FAST_BASELINES=1 selects) against the autograd path,
measured alternately on the same process, steady state (one update per iteration, online Q_risk update).

    python profiles/baselines_iteration.py [--iters 100] [--rounds 3] [--out profiles/baselines_iteration.json]

Eager iterations for every line and path; for the fused LR, RCPO and SQRL lines also the captured iteration (hipGraph replay:
what the driver runs in its steady state -- RSPO is not captured there).  SQRL has a third leg, `hip`: the fused path with
its constraint-sampling acting pass on the rrl_sqrl_act kernel (RRL_FAST_SQRL=1) instead of module code, alternated with the
other two in the same process, plus the acting launch's own time from HIP events and its rate against the FLOPs the
algorithm needs (n k rows of the twin 4-256-256-1 network) and against the FLOPs executed with the row padding.  Launches per
iteration: run under `rocprofv3 --kernel-trace --stats -- python profiles/baselines_iteration.py --iters 20 --rounds 1`."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import arg_utils  # noqa: E402
import bench  # noqa: E402

LINES = {"LR": ["--DGD_constraints", "--nu", "5000", "--update_nu"],
         "RSPO": ["--DGD_constraints", "--nu_schedule", "--nu_start", "10000"],
         "SQRL": ["--DGD_constraints", "--use_constraint_sampling", "--nu", "5000", "--update_nu"],
         "RCPO": ["--RCPO", "--lambda_RCPO", "1000"]}


def time_it(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e3


Q_FLOP_PER_ROW = 2 * (2 * 4 * 256 + 2 * 256 * 256 + 2 * 256)     # the twin Q_risk heads on one candidate row: 267 264
SQRL_K = 100


def build(line, path, envs, dev):
    """One loop of `line` on `path`: fused / autograd, or hip = fused with RRL_FAST_SQRL=1 (both switches are read when the
    loop is built)."""
    cfg = arg_utils.get_args(["--env-name", "navigation1", "--cuda", "--gamma_safe", "0.8", "--eps_safe", "0.3",
                              "--num_envs", str(envs), "--seed", "1", "--num_unsafe_transitions", "4000"] + LINES[line])
    switches = {"RRL_FAST_BASELINES": "1", "RRL_FAST_SQRL": "1"} if path == "hip" else {}
    saved = {k: os.environ.get(k) for k in switches}
    os.environ.update(switches)
    try:
        loop = bench.build_loop(cfg, dev, fast=path != "autograd", pretrain=5)
    finally:
        for k, v in saved.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v
    assert loop.sqrl_hip == (path == "hip")
    for _ in range(5):
        loop.vector_step(True, False, True)
    return loop


def acting_launch_ms(loop, launches=50, rounds=3):
    """The rrl_sqrl_act launch alone, back to back between two HIP events (its argument block as the acting pass left it;
    every launch draws at the next tick)."""
    from recovery_rl_amd import _lib
    import ctypes as C
    actor, lib = loop.sqrl_actor(), _lib.load()
    a, st = actor._sqrl_args, _lib.current_stream()
    out = []
    for _ in range(rounds + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(launches):
            _lib.check(lib.rrl_sqrl_act(C.byref(a), st), "rrl_sqrl_act")
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / launches)
    return out[1:]                                     # the first round warms up


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--lines", default="LR,RSPO,SQRL,RCPO")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    res = {}
    for line in a.lines.split(","):
        paths = ("fused", "hip", "autograd") if line == "SQRL" else ("fused", "autograd")
        loops = {path: build(line, path, a.envs, dev) for path in paths}
        out = {path + "_eager_ms": [] for path in paths}
        for _ in range(a.rounds):                      # alternating: fused, (hip,) autograd, fused, ...
            for path in paths:
                out[path + "_eager_ms"].append(time_it(lambda: loops[path].vector_step(True, False, True), a.iters))
        if line != "RSPO":
            graphed = [p for p in paths if p != "autograd"]
            for path in graphed:
                loops[path].capture(online_qrisk=True)
                out[path + "_graph_ms"] = []
            for _ in range(a.rounds):                  # alternating here too
                for path in graphed:
                    out[path + "_graph_ms"].append(time_it(loops[path].replay, a.iters))
        if line == "SQRL":
            out["hip_acting_launch_ms"] = acting_launch_ms(loops["hip"])
        res[line] = {k: [round(x, 4) for x in v] for k, v in out.items()}
        if line == "SQRL":
            ms = min(out["hip_acting_launch_ms"])
            rows, padded = a.envs * SQRL_K, a.envs * 16 * ((SQRL_K + 15) // 16)
            res[line]["acting_launch"] = {"ms_best": round(ms, 4), "gflop_needed": round(rows * Q_FLOP_PER_ROW / 1e9, 2),
                                          "gflop_executed": round(padded * Q_FLOP_PER_ROW / 1e9, 2),
                                          "tflops_needed": round(rows * Q_FLOP_PER_ROW / ms / 1e9, 1),
                                          "tflops_executed": round(padded * Q_FLOP_PER_ROW / ms / 1e9, 1),
                                          "f32_mfma_peak_tflops": 157.3}
        print(line, json.dumps(res[line]), flush=True)
        del loops
        torch.cuda.empty_cache()
    res["setup"] = {"envs": a.envs, "hidden": 256, "batch": 256, "iters": a.iters, "rounds": a.rounds,
                    "device": torch.cuda.get_device_name(0)}
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
