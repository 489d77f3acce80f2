"""Seed packing for the comparison lines of scripts/navigation1.sh (LR, RCPO, SQRL; fused update path, no recovery policy) at
4096 envs, hidden 256, batch 256: milliseconds per packed iteration, aggregate gradient steps and env steps per second at
S = 1, 4, 8 seeds per GPU against the solo hipGraph replay of the same configuration (what `--seeds_per_gpu 1` runs in its
steady state).  Times are HIP-event times.

    python profiles/packed_baselines.py [--rounds 5] [--seconds 1.2] [--out profiles/packed_baselines.json]
    python profiles/packed_baselines.py --lines SQRL --seeds 1,2,4,8 --seconds 3 --out profiles/packed_sqrl.json

The SQRL line acts on the rrl_sqrl_act kernel (RRL_FAST_SQRL=1 is set for it here) and packs that pass as one
rrl_sqrl_act_packed launch; its row also times that launch ALONE (`acting_launch`: the packed launch of S seeds against S times
the stand-alone launch of one, same descriptors as the iteration's).

Every leg (solo, S = 1, S = 4, S = 8) has its own learners; the legs are timed alternately in one process, each for at least
`--seconds` after warm-up, the way the drivers run them (bench.production_step: advance() -- the many-iteration graphs -- up to
every 100th iteration, where the counters are read and the episode tables drained).  The run-to-run noise the S = 1 leg is
judged against is the spread of the alternated solo legs."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import arg_utils  # noqa: E402
import bench  # noqa: E402
from recovery_rl_amd.packed import PackedLoop  # noqa: E402

LINES = {"LR": ["--DGD_constraints", "--nu", "5000", "--update_nu"],
         "RCPO": ["--RCPO", "--lambda_RCPO", "1000"],
         "SQRL": ["--DGD_constraints", "--use_constraint_sampling", "--nu", "5000", "--update_nu"]}


def make_loop(line, envs, seed, dev):
    cfg = arg_utils.get_args(["--env-name", "navigation1", "--cuda", "--gamma_safe", "0.8", "--eps_safe", "0.3",
                              "--num_envs", str(envs), "--seed", str(seed), "--num_unsafe_transitions", "4000"] + LINES[line])
    return bench.build_loop(cfg, dev, pretrain=5)


def timed(advance, iters):
    """ms per iteration of advance(iters), between two HIP events"""
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    advance(iters)
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / iters


def acting_launch_alone(solo, packs, seconds):
    """SQRL's acting launch outside the iteration: us per packed launch of S seeds, and per stand-alone launch of one seed (the
    descriptors the loops recorded; the device ticks keep advancing, as in the iteration)."""
    from recovery_rl_amd import _lib
    import ctypes as C
    lib, st = _lib.load(), _lib.current_stream()
    one = solo.sqrl_actor()._sqrl_args
    legs = {"solo": lambda: lib.rrl_sqrl_act(C.byref(one), st)}
    for pk in packs:
        fn, args, _ = [stage for stage in pk.stages if stage[2][0][0] == "sqrl"][0]
        legs["S%d" % pk.S] = lambda fn=fn, args=args: fn(*args, st)
    out = {}
    for name, launch in legs.items():
        def many(n, launch=launch):
            for _ in range(n):
                assert launch() == 0
        many(50)
        ms = timed(many, 200)
        out[name] = round(timed(many, max(200, int(seconds / (ms * 1e-3)))) * 1e3, 2)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--seconds", type=float, default=1.2)
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--seeds", default="1,4,8")
    ap.add_argument("--lines", default="LR,RCPO")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    sizes = [int(s) for s in a.seeds.split(",")]
    res = {}
    for line in a.lines.split(","):
        legs, seed = {}, 1
        if line == "SQRL":           # the acting pass on the kernel: what the packed form packs
            os.environ["RRL_FAST_SQRL"] = os.environ["RRL_FAST_BASELINES"] = "1"
        else:
            os.environ.pop("RRL_FAST_SQRL", None)
        solo = make_loop(line, a.envs, seed, dev)
        solo.capture(online_qrisk=True)
        legs["solo"] = (1, bench.production_step(solo.replay, [solo], advance=solo.advance).many)
        packs = []
        for S in sizes:
            loops = []
            for _ in range(S):
                seed += 1
                loops.append(make_loop(line, a.envs, seed, dev))
            pk = PackedLoop(loops, online_qrisk=True)
            pk.capture()
            packs.append(pk)
            legs["S%d" % S] = (S, bench.production_step(pk.replay, loops, advance=pk.advance).many)
        launches = {"S%d" % pk.S: pk.launches for pk in packs}
        iters = {}
        for name, (S, adv) in legs.items():             # warm-up, and the iterations that fill `--seconds`
            adv(200)
            ms = timed(adv, 400)
            iters[name] = max(400, 4 * int(a.seconds / (ms * 1e-3) / 4 + 1))
        out = {name: [] for name in legs}
        for _ in range(a.rounds):                        # alternating: solo, S = 1, S = 4, S = 8, solo, ...
            for name, (S, adv) in legs.items():
                out[name].append(timed(adv, iters[name]))
        row = {}
        for name, (S, _) in legs.items():
            med = statistics.median(out[name])
            row[name] = {"ms_per_iteration": [round(x, 4) for x in out[name]], "median_ms": round(med, 4), "seeds": S,
                         "grad_steps_per_s": round(S * 1e3 / med, 1), "env_steps_per_s": round(S * a.envs * 1e3 / med),
                         "iterations_per_leg": iters[name]}
            if name in launches:
                row[name]["launches"] = launches[name]
        s = out["solo"]
        row["solo"]["spread"] = round((max(s) - min(s)) / statistics.median(s), 4)
        if line == "SQRL":
            assert solo.sqrl_hip and all(l.sqrl_hip for pk in packs for l in pk.loops)
            row["acting_launch_us"] = acting_launch_alone(solo, packs, a.seconds)
        res[line] = row
        print(line, json.dumps(row), flush=True)
        for pk in packs:
            pk.graph = pk.graph_many = None
        packs[-1].close()
        del packs, legs, solo
        torch.cuda.empty_cache()
    res["setup"] = {"envs": a.envs, "hidden": 256, "batch": 256, "rounds": a.rounds, "seconds_per_leg": a.seconds,
                    "device": torch.cuda.get_device_name(0)}
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
