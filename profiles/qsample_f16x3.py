"""f16x3 scoring for the acting pass of Q-sampling recovery (RRL_QSAMPLE_F16X3=1: rrl_w2_pack_f16x3 + rrl_qsample_act_f16x3) against
the f32 kernels of the same build (rrl_qsample_act), at 4096 envs, k = 1000, Navigation 1, hidden 256, both loops under
RRL_FAST_QSAMPLE=1:

  * the acting call ALONE, HIP-event time, on a mask with exactly 0, 64, 512 and 4096 of the envs gated (spread evenly): the f32
    call (both kernels), and the pack + f16x3 call together, on the descriptors the loops recorded (the device ticks keep
    advancing, as in the iteration); the two legs alternated over `--rounds` rounds;
  * the captured iteration (hipGraph replay, one update per iteration, online Q_risk update) at eps_safe = 1 (nothing gated) and
    -1 (everything gated), the two shares that are exact under graph replay; legs alternated likewise.

    python profiles/qsample_f16x3.py [--rounds 3] [--launches 20] [--iters 30] [--out profiles/qsample_f16x3.json]

Every leg has its own learner (the same seed).  The spread of a leg is (max - min) / median over its rounds.  Not measured here:
Maze, the packed launch, any k other than 1000."""
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

from qsample_iteration import K, Q_FLOP_PER_ROW, build, events_ms, time_it  # noqa: E402
from recovery_rl_amd import _lib  # noqa: E402

GATED = (0, 64, 512, 4096)


def loop_of(f16x3, envs, dev):
    """A Q-sampling learner on the kernels, built with the switch in the given position (VectorLoop reads it once, when it is built)."""
    saved = os.environ.pop("RRL_QSAMPLE_F16X3", None)
    if f16x3:
        os.environ["RRL_QSAMPLE_F16X3"] = "1"
    try:
        loop = build("hip", envs, dev)
    finally:
        os.environ.pop("RRL_QSAMPLE_F16X3", None)
        if saved is not None:
            os.environ["RRL_QSAMPLE_F16X3"] = saved
    assert loop.qsample_hip and loop.qsample_f16x3 == f16x3
    return loop


def summary(xs):
    med = statistics.median(xs)
    return {"ms": [round(x, 5) for x in xs], "median_ms": round(med, 5), "spread": round((max(xs) - min(xs)) / med, 4)}


def acting_call(loops, gated, launches, rounds):
    """ms per acting call outside the iteration with exactly `gated` envs gated: rrl_qsample_act, and rrl_w2_pack_f16x3 +
    rrl_qsample_act_f16x3 together (and the f16x3 call without the pack)."""
    lib, st = _lib.load(), _lib.current_stream()
    n, dev = loops["f32"].n, loops["f32"].device
    mask = torch.zeros(n, dtype=torch.uint8, device=dev)
    if gated:
        mask[torch.linspace(0, n - 1, gated, device=dev).round().long()] = 1
    assert int(mask.sum()) == gated
    args = {}
    for tag, loop in loops.items():
        actor = loop.qsample_actor()
        a = type(actor._qsample_args).from_buffer_copy(actor._qsample_args)
        a.mask = mask.data_ptr()
        args[tag] = a
    actor = loops["f16x3"].qsample_actor()
    W2 = loops["f16x3"].agent.fast.qrisk.p["W2"]
    pack = (W2.shape[0], W2.shape[1], W2.data_ptr(), actor.qsample_w2h.data_ptr())
    assert args["f16x3"].W2p == actor.qsample_w2h.data_ptr() != args["f32"].W2p
    assert (args["f32"].n, args["f32"].k) == (args["f16x3"].n, args["f16x3"].k) == (n, K)

    def f32():
        assert lib.rrl_qsample_act(C.byref(args["f32"]), st) == 0

    def f16x3():
        assert lib.rrl_w2_pack_f16x3(*pack, st) == 0 and lib.rrl_qsample_act_f16x3(C.byref(args["f16x3"]), st) == 0

    def f16x3_no_pack():
        assert lib.rrl_qsample_act_f16x3(C.byref(args["f16x3"]), st) == 0

    legs = {"f32": f32, "f16x3_with_pack": f16x3, "f16x3_call_only": f16x3_no_pack}
    count = launches * (1 if 8 * gated >= n else 16)           # a window of comparable length at every share
    out = {name: [] for name in legs}
    for _ in range(rounds):                                    # alternating
        for name, fn in legs.items():
            out[name] += events_ms(fn, count, 1)
    row = {name: summary(xs) for name, xs in out.items()}
    row["gated_envs"], row["launches_per_leg"] = gated, count
    row["f32_over_f16x3_with_pack"] = [round(a / b, 4) for a, b in zip(out["f32"], out["f16x3_with_pack"])]
    row["f16x3_faster_in_every_round"] = all(b < a for a, b in zip(out["f32"], out["f16x3_with_pack"]))
    if gated:
        for name in ("f32", "f16x3_with_pack"):
            row[name]["tflops_needed"] = round(gated * K * Q_FLOP_PER_ROW / row[name]["median_ms"] / 1e9, 2)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    loops = {"f32": loop_of(False, a.envs, dev), "f16x3": loop_of(True, a.envs, dev)}
    res = {"acting_call": {}, "iteration": {}}
    for gated in GATED:
        if gated <= a.envs:
            res["acting_call"][str(gated)] = acting_call(loops, gated, a.launches, a.rounds)
            print(gated, json.dumps(res["acting_call"][str(gated)]), flush=True)
    for eps in (1.0, -1.0):
        out = {tag: [] for tag in loops}
        share = {tag: [] for tag in loops}
        for tag, loop in loops.items():
            loop.cfg.eps_safe = eps
            loop.capture(online_qrisk=True)
        for _ in range(a.rounds):                              # alternating
            for tag, loop in loops.items():
                out[tag].append(time_it(loop.replay, a.iters))
                share[tag].append(float(loop._last_recovery.float().mean()))
        row = {tag: dict(summary(out[tag]), gated_share=share[tag],
                         env_steps_per_s=round(a.envs * 1e3 / statistics.median(out[tag]))) for tag in loops}
        row["f32_over_f16x3"] = [round(x / y, 4) for x, y in zip(out["f32"], out["f16x3"])]
        res["iteration"]["eps_safe_%g" % eps] = row
        print(eps, json.dumps(row), flush=True)
    res["setup"] = {"envs": a.envs, "k": K, "env": "navigation1", "hidden": 256, "batch": 256, "rounds": a.rounds,
                    "launches": a.launches, "iters": a.iters, "device": torch.cuda.get_device_name(0),
                    "not_measured": ["maze", "the packed launch", "k other than 1000"]}
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
