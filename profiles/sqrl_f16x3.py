"""f16x3 scoring for SQRL's acting pass (RRL_SQRL_F16X3=1: rrl_w2_pack_f16x3 + rrl_sqrl_act_f16x3) against the f32 kernel of
the same build (rrl_sqrl_act), at 4096 envs, k = 100, Navigation 1, hidden 256:

  * the acting launch ALONE, HIP-event time: the f32 launch, and the pack + f16x3 launch pair, on the descriptors the loops
    recorded (the device ticks keep advancing, as in the iteration); legs alternated over `--rounds` rounds;
  * the SQRL line's env-steps/s with and without the switch, solo (the hipGraph replay of `--seeds_per_gpu 1`) and packed at
    S = 4 (RRL_PACK_SQRL=1), the way the drivers run them (bench.production_step), legs alternated likewise.

    python profiles/sqrl_f16x3.py [--rounds 5] [--seconds 1.5] [--out profiles/sqrl_f16x3.json]

Every leg has its own learners.  The spread of a leg is (max - min) / median over its rounds.  Not measured here: Maze, S = 2 / 8."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import bench  # noqa: E402
from packed_baselines import make_loop, timed  # noqa: E402
from recovery_rl_amd import _lib  # noqa: E402
from recovery_rl_amd.packed import PackedLoop  # noqa: E402


def loops_of(S, f16x3, envs, seed, dev):
    """S SQRL learners built with the switch in the given position (VectorLoop reads it once, when it is built)."""
    os.environ["RRL_SQRL_F16X3"] = "1" if f16x3 else "0"
    loops = [make_loop("SQRL", envs, seed + s, dev) for s in range(S)]
    assert all(l.sqrl_hip and l.sqrl_f16x3 == f16x3 for l in loops)
    return loops


def spread(xs):
    return round((max(xs) - min(xs)) / statistics.median(xs), 4)


def launches_alone(f32_loop, f16_loop, rounds, seconds):
    """us per acting launch outside the iteration: rrl_sqrl_act, and rrl_w2_pack_f16x3 + rrl_sqrl_act_f16x3 together."""
    lib, st = _lib.load(), _lib.current_stream()
    a32 = f32_loop.sqrl_actor()._sqrl_args
    actor = f16_loop.sqrl_actor()
    a16, W2 = actor._sqrl_args, f16_loop.agent.fast.qrisk.p["W2"]
    pack = (W2.shape[0], W2.shape[1], W2.data_ptr(), actor.sqrl_w2h.data_ptr())
    assert a16.W2p == actor.sqrl_w2h.data_ptr() and a32.W2p != a16.W2p and (a32.n, a32.k) == (a16.n, a16.k)

    def f32(n):
        for _ in range(n):
            assert lib.rrl_sqrl_act(C.byref(a32), st) == 0

    def f16x3(n):
        for _ in range(n):
            assert lib.rrl_w2_pack_f16x3(*pack, st) == 0 and lib.rrl_sqrl_act_f16x3(C.byref(a16), st) == 0

    def f16x3_no_pack(n):
        for _ in range(n):
            assert lib.rrl_sqrl_act_f16x3(C.byref(a16), st) == 0

    legs = {"f32": f32, "f16x3_with_pack": f16x3, "f16x3_launch_only": f16x3_no_pack}
    iters = {}
    for name, many in legs.items():
        many(50)
        ms = timed(many, 100)
        iters[name] = max(100, int(seconds / (ms * 1e-3)))
    out = {name: [] for name in legs}
    for _ in range(rounds):
        for name, many in legs.items():
            out[name].append(round(timed(many, iters[name]) * 1e3, 2))
    row = {name: {"us_per_launch": xs, "median_us": statistics.median(xs), "spread": spread(xs), "launches_per_leg": iters[name]}
           for name, xs in out.items()}
    row["f32_over_f16x3_with_pack"] = round(row["f32"]["median_us"] / row["f16x3_with_pack"]["median_us"], 3)
    row["n"], row["k"] = a32.n, a32.k
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--seconds", type=float, default=1.5)
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--packed_seeds", type=int, default=4)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    for name in ("RRL_FAST_SQRL", "RRL_FAST_BASELINES", "RRL_PACK_SQRL"):
        os.environ[name] = "1"
    S = a.packed_seeds
    legs, solos, packs, seed = {}, {}, [], 1
    for f16x3 in (False, True):
        tag = "f16x3" if f16x3 else "f32"
        solo = loops_of(1, f16x3, a.envs, seed, dev)[0]
        solo.capture(online_qrisk=True)
        solos[tag] = solo
        legs["solo_" + tag] = (1, bench.production_step(solo.replay, [solo], advance=solo.advance).many)
        loops = loops_of(S, f16x3, a.envs, seed + 1, dev)        # the same seeds in both positions of the switch
        pk = PackedLoop(loops, online_qrisk=True)
        pk.capture()
        kinds = [op[0] for op in pk.tapes[0]]
        assert kinds.count("sqrl_f16x3" if f16x3 else "sqrl") == 1
        packs.append(pk)
        legs["S%d_%s" % (S, tag)] = (S, bench.production_step(pk.replay, loops, advance=pk.advance).many)
    iters = {}
    for name, (_, adv) in legs.items():                  # warm-up, and the iterations that fill `--seconds`
        adv(100)
        ms = timed(adv, 100)
        iters[name] = max(100, 4 * int(a.seconds / (ms * 1e-3) / 4 + 1))
    out = {name: [] for name in legs}
    for _ in range(a.rounds):                            # alternating: solo f32, S f32, solo f16x3, S f16x3, solo f32, ...
        for name, (_, adv) in legs.items():
            out[name].append(timed(adv, iters[name]))
    res = {"line": {}}
    for name, (n_seeds, _) in legs.items():
        med = statistics.median(out[name])
        res["line"][name] = {"ms_per_iteration": [round(x, 4) for x in out[name]], "median_ms": round(med, 4),
                             "spread": spread(out[name]), "seeds": n_seeds, "env_steps_per_s": round(n_seeds * a.envs * 1e3 / med),
                             "iterations_per_leg": iters[name]}
    for shape in ("solo", "S%d" % S):
        res["line"]["%s_f16x3_over_f32" % shape] = round(res["line"][shape + "_f16x3"]["env_steps_per_s"]
                                                        / res["line"][shape + "_f32"]["env_steps_per_s"], 3)
    res["acting_launch"] = launches_alone(solos["f32"], solos["f16x3"], a.rounds, a.seconds)
    res["setup"] = {"envs": a.envs, "k": 100, "env": "navigation1", "hidden": 256, "batch": 256, "rounds": a.rounds,
                    "seconds_per_leg": a.seconds, "packed_seeds": S, "device": torch.cuda.get_device_name(0),
                    "not_measured": ["maze", "S = 2", "S = 8"]}
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    for pk in packs:
        pk.graph = pk.graph_many = None
    for pk in packs:
        pk.close()


if __name__ == "__main__":
    main()
