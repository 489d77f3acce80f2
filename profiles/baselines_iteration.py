"""Milliseconds per lock-step iteration of the comparison lines of scripts/navigation1.sh (LR, RSPO, SQRL, RCPO) at
4096 envs, hidden 256, batch 256: the fused update path (what RRL_FAST_BASELINES=1 selects) against the autograd path,
measured alternately on the same process, steady state (one update per iteration, online Q_risk update).

    python profiles/baselines_iteration.py [--iters 100] [--rounds 3] [--out profiles/baselines_iteration.json]

Eager iterations for every line and path; for the fused LR and RCPO lines also the captured iteration (hipGraph replay:
what the driver runs in its steady state -- RSPO is not captured there, SQRL's acting is module code).  Launches per
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
        loops = {}
        for path in ("fused", "autograd"):
            cfg = arg_utils.get_args(["--env-name", "navigation1", "--cuda", "--gamma_safe", "0.8", "--eps_safe", "0.3",
                                      "--num_envs", str(a.envs), "--seed", "1", "--num_unsafe_transitions", "4000"]
                                     + LINES[line])
            loops[path] = bench.build_loop(cfg, dev, fast=path == "fused", pretrain=5)
            for _ in range(5):
                loops[path].vector_step(True, False, True)
        out = {"fused_eager_ms": [], "autograd_eager_ms": []}
        for _ in range(a.rounds):                      # alternating: fused, autograd, fused, ...
            for path in ("fused", "autograd"):
                out[path + "_eager_ms"].append(time_it(lambda: loops[path].vector_step(True, False, True), a.iters))
        if line in ("LR", "RCPO"):
            lp = loops["fused"]
            lp.capture(online_qrisk=True)
            out["fused_graph_ms"] = [time_it(lp.replay, a.iters) for _ in range(a.rounds)]
        res[line] = {k: [round(x, 4) for x in v] for k, v in out.items()}
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
