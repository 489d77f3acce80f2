"""Seed packing for the comparison algorithms (LR, RSPO, RCPO, SAC without a recovery policy), the parts that need no GPU:
the three packed entry points are declared and exported, every launch of the comparison algorithms' grouped SAC update and
of the acting pass without a recovery policy lands on the launch tape under a kind PackedLoop can pack, taping changes no
launch, and run_packed names the flag or switch of what it does not pack."""
import os
import re

import numpy as np
import pytest
import torch

import arg_utils
from recovery_rl_amd import _lib, fast_update
from recovery_rl_amd.experiment import run_packed
from recovery_rl_amd.sac import SAC
from recovery_rl_amd.spaces import Box
from recovery_rl_amd.utils import linear_schedule

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ACT = Box(-np.ones(2), np.ones(2))
OBS = Box(-np.ones(2) * np.inf, np.ones(2) * np.inf)
HOST_ONLY = ("rrl_mlp3_is_split", "rrl_abi_version", "rrl_last_hip_error")
NEW = ("rrl_adam_step_multi_duals_packed", "rrl_rcpo_penalty_packed", "rrl_policy_heads_fwd_multi_packed")

# the SAC-update flags of the comparison lines (scripts/navigation1.sh) and two combinations of their terms:
# (flags, "penalty" launches of one SAC update)
CONFIGS = {"LR": (["--DGD_constraints", "--nu", "50", "--update_nu"], 0),
           "RSPO": (["--DGD_constraints", "--nu_schedule", "--nu_start", "10000", "--num_eps", "400"], 0),
           "RCPO": (["--RCPO", "--lambda_RCPO", "10"], 1),
           "update_nu": (["--nu", "50", "--update_nu"], 1),
           "DGD_RCPO": (["--DGD_constraints", "--nu", "50", "--RCPO", "--lambda_RCPO", "10"], 1)}


def test_header_and_loader_carry_the_three_packed_entry_points():
    src = open(os.path.join(ROOT, "include", "rrl_hip.h")).read()
    table = src[src.index("Packed launches:"):]
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, src), name            # declared ...
        assert name in table.split("typedef")[0], name                     # ... and listed in the packed-launch table
        assert name in _lib.EXPORTS, name
    assert "rrl_penalty_args_t" in src
    assert [f[0] for f in _lib.rrl_penalty_args_t._fields_] == ["B", "z", "n_part", "part_stride", "lambda_", "penalty", "mean"]


@pytest.fixture
def calls(monkeypatch):
    real, names = _lib.load(), []

    class Recorder:
        def __getattr__(self, name):
            if name in HOST_ONLY:
                return getattr(real, name)
            return lambda *args: names.append(name[4:]) or 0           # without the rrl_ prefix

    monkeypatch.setattr(_lib, "_lib", Recorder())
    monkeypatch.setattr(_lib, "current_stream", lambda: 0)
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: False)
    monkeypatch.setenv("RRL_FAST_BASELINES", "1")
    return names


def updater(flags, hidden=256, B=256, recovery=True):
    argv = ["--env-name", "navigation1", "--hidden_size", str(hidden), "--gamma_safe", "0.8", "--eps_safe", "0.3"]
    argv += ["--use_recovery", "--MF_recovery"] if recovery else []
    args = arg_utils.get_args(argv + list(flags))
    torch.manual_seed(0)
    fast = SAC(OBS, ACT, args, "/tmp").enable_fast_path(B)
    r = lambda *s: torch.randn(*s)
    nu = linear_schedule(args.nu_start, args.nu_end, args.num_eps)(1) if args.nu_schedule else args.nu
    return fast, (r(B, 2), r(B, 2), r(B), r(B, 2), r(B)), r(B, 2), r(B, 2), nu


def taped(calls, fn, *args, **kw):
    """(library calls, tape) of one call of `fn` with a launch tape set."""
    del calls[:]
    tape = []
    fast_update.set_tape(tape)
    try:
        fn(*args, **kw)
    finally:
        fast_update.set_tape(None)
    return list(calls), tape


@pytest.mark.parametrize("config", sorted(CONFIGS))
def test_grouped_baseline_update_is_taped_without_an_unsupported_launch(calls, config):
    flags, penalties = CONFIGS[config]
    fast, batch, e1, e2, nu = updater(flags)
    assert fast.grouped and fast.cri_a.split and fast.cri_a.fuse_first
    del calls[:]
    fast.sac_update(batch, e1, e2, nu=nu, grouped=True)
    plain = list(calls)
    got, tape = taped(calls, fast.sac_update, batch, e1, e2, nu=nu, grouped=True)
    kinds = [op[0] for op in tape]
    assert "unsupported" not in kinds, (config, [op for op in tape if op[0] == "unsupported"])
    assert kinds.count("adam_duals") == 1 and kinds.count("adam") == 0
    assert kinds.count("penalty") == penalties
    assert got == plain                                                   # taping changes no launch ...
    assert len(kinds) == len(plain)                                       # ... and every launch is on the tape
    of = {"mlp3_forward_multi": "forward", "mlp_backward_pair_multi": "pair_bwd", "rcpo_penalty": "penalty",
          "adam_step_multi_duals": "adam_duals"}
    assert kinds == [of[name] for name in plain]
    # the payloads the packed entry points take, alive on the tape
    op = tape[kinds.index("adam_duals")]
    segs, n_seg, duals, n_dual = op[1:5]
    assert isinstance(segs, _lib.rrl_adam_seg_t * 2) and n_seg == 2
    assert isinstance(duals, _lib.rrl_dual_t * n_dual) and 1 <= n_dual <= 2
    assert op[5:] == (float(fast.agent.lr), 0.9, 0.999, 1e-8)
    for op in tape:
        if op[0] == "penalty":
            a = op[1]
            assert isinstance(a, _lib.rrl_penalty_args_t) and a.B == 256 and a.z and a.mean
            assert bool(a.penalty) == bool(a.lambda_) == (config != "update_nu")


def test_plain_sac_update_keeps_the_plain_optimiser_launch_on_the_tape(calls):
    fast, batch, e1, e2, nu = updater([], recovery=False)
    got, tape = taped(calls, fast.sac_update, batch, e1, e2, grouped=True)
    assert [op[0] for op in tape] == ["forward", "forward", "pair_bwd", "pair_bwd", "adam"]
    assert got == ["mlp3_forward_multi", "mlp3_forward_multi", "mlp_backward_pair_multi", "mlp_backward_pair_multi",
                   "adam_step_multi"]


def test_acting_pass_without_recovery_policy_is_taped_as_forward_and_heads(calls):
    """FastActor.act(use_recovery=False): the policy forward through the group entry point (the column-split kernels' body),
    the head through rrl_policy_heads_fwd_multi -- kinds "forward" and "heads"."""
    fast, _, _, _, _ = updater(CONFIGS["LR"][0], recovery=False)
    n = 128
    actor = fast_update.FastActor(fast, n)
    assert actor.pol.split
    got, tape = taped(calls, actor.act, torch.randn(n, 2), 0.3, False, False, noise=torch.randn(2, n, 2))
    assert got == ["mlp3_forward_multi", "policy_heads_fwd_multi"]
    assert [op[0] for op in tape] == ["forward", "heads"]
    heads, count = tape[1][1:]
    assert count == 1 and heads[0].kind == _lib.HEAD_GAUSS and heads[0].B == n and not heads[0].logp
    # a width without the column-split kernels keeps the stand-alone forward: nothing the tape can pack
    small, _, _, _, _ = updater([], hidden=32, B=64, recovery=False)
    got, tape = taped(calls, fast_update.FastActor(small, n).act, torch.randn(n, 2), 0.3, False, False,
                      noise=torch.randn(2, n, 2))
    assert got == ["mlp3_forward", "policy_heads_fwd_multi"] and [op[0] for op in tape] == ["unsupported", "heads"]


BASE = ["--env-name", "navigation1", "--cuda", "--num_envs", "128", "--seeds_per_gpu", "2", "--gamma_safe", "0.8",
        "--eps_safe", "0.3"]
MF = ["--use_recovery", "--MF_recovery"]
LR = ["--DGD_constraints", "--nu", "5000", "--update_nu"]


@pytest.mark.parametrize("switch,flags,names", [
    ("1", LR + ["--use_constraint_sampling"], "use_constraint_sampling"),              # SQRL
    ("1", MF + ["--use_constraint_sampling"], "use_constraint_sampling"),
    (None, LR, "RRL_FAST_BASELINES"),
    (None, MF + ["--RCPO"], "RRL_FAST_BASELINES"),
    ("0", ["--DGD_constraints", "--nu_schedule"], "RRL_FAST_BASELINES"),
    ("1", ["--use_recovery"], "MF_recovery"),                                           # model-based recovery
    ("1", ["--use_recovery", "--Q_sampling_recovery"], "MF_recovery"),
    ("1", LR + ["--dp_mode", "env_shard"], "env_shard"),
    ("1", LR + ["--resume", "somewhere.pt"], "resume"),
    ("1", MF + ["--checkpoint_every", "100"], "checkpoint_every"),
])
def test_run_packed_names_what_it_does_not_pack(monkeypatch, tmp_path, switch, flags, names):
    if switch is None:
        monkeypatch.delenv("RRL_FAST_BASELINES", raising=False)
    else:
        monkeypatch.setenv("RRL_FAST_BASELINES", switch)
    cfg = arg_utils.get_args(BASE + ["--logdir", str(tmp_path)] + flags)
    with pytest.raises(ValueError, match=names):
        run_packed(cfg)
    assert not os.listdir(tmp_path)                       # refused before anything was set up


def test_packed_entry_points_validate_every_seed_without_gpu():
    """What the three entry points answer to malformed input: every call returns before anything is stored or launched (dummy
    non-null device pointers: validation never follows them)."""
    import ctypes as C
    lib, d, P = _lib.load(), 0x1000, C.POINTER
    EINVAL = -1
    seg = (_lib.rrl_adam_seg_t * 1)(_lib.rrl_adam_seg_t(n=64, p=d, g=d, m=d, v=d, step_dev=d))
    dual = (_lib.rrl_dual_t * 1)(_lib.rrl_dual_t(log_p=d, exp_avg=d, exp_avg_sq=d, step=d, stat=d))
    no_stat = (_lib.rrl_dual_t * 1)(_lib.rrl_dual_t(log_p=d, exp_avg=d, exp_avg_sq=d, step=d))
    idle = (_lib.rrl_dual_t * 1)(_lib.rrl_dual_t(stat=d))                             # neither a step nor a statistic to write
    segs = lambda *a: (P(_lib.rrl_adam_seg_t) * len(a))(*[C.cast(x, P(_lib.rrl_adam_seg_t)) for x in a])
    duals = lambda *a: (P(_lib.rrl_dual_t) * len(a))(*[C.cast(x, P(_lib.rrl_dual_t)) for x in a])
    ints = lambda *a: (C.c_int * len(a))(*a)
    lr = (C.c_float * 2)(3e-4, 3e-4)
    adam = lambda S, n, s, nd, du, rates=lr: lib.rrl_adam_step_multi_duals_packed(S, n, s, nd, du, rates, 0.9, 0.999, 1e-8, None)
    for S in (0, -1, 17):
        assert adam(S, ints(1), segs(seg), ints(1), duals(dual)) == EINVAL
    assert adam(2, None, segs(seg, seg), ints(1, 1), duals(dual, dual)) == EINVAL
    assert adam(2, ints(1, 1), None, ints(1, 1), duals(dual, dual)) == EINVAL
    assert adam(2, ints(1, 1), segs(seg, seg), None, duals(dual, dual)) == EINVAL
    assert adam(2, ints(1, 1), segs(seg, seg), ints(1, 1), None) == EINVAL
    assert adam(2, ints(1, 1), segs(seg, seg), ints(1, 1), duals(dual, dual), None) == EINVAL
    assert adam(2, ints(1, 13), segs(seg, seg), ints(1, 1), duals(dual, dual)) == EINVAL          # > RRL_ADAM_MAX_SEGS
    assert adam(2, ints(1, -1), segs(seg, seg), ints(1, 1), duals(dual, dual)) == EINVAL
    assert adam(2, ints(1, 1), segs(seg, seg), ints(1, 0), duals(dual, dual)) == EINVAL           # a seed without a dual
    assert adam(2, ints(1, 1), segs(seg, seg), ints(1, 5), duals(dual, dual)) == EINVAL           # > RRL_ADAM_MAX_DUALS
    assert adam(2, ints(1, 1), segs(seg, seg), ints(1, 1), duals(dual, no_stat)) == EINVAL        # the second seed's member
    assert adam(2, ints(1, 1), segs(seg, seg), ints(1, 1), duals(idle, dual)) == EINVAL
    bad_seg = (_lib.rrl_adam_seg_t * 1)(_lib.rrl_adam_seg_t(n=64, p=d, g=d, m=d, v=d))           # no step counter
    assert adam(2, ints(1, 1), segs(seg, bad_seg), ints(1, 1), duals(dual, dual)) == EINVAL
    assert adam(1, ints(1), segs(seg), ints(1), duals(no_stat)) == EINVAL                         # one seed: the solo entry's answer

    pen = lambda **k: _lib.rrl_penalty_args_t(**dict(dict(B=8, z=d, n_part=1, mean=d), **k))
    arr = lambda *a: (_lib.rrl_penalty_args_t * len(a))(*a)
    for S in (0, 17):
        assert lib.rrl_rcpo_penalty_packed(S, arr(pen()), None) == EINVAL
    assert lib.rrl_rcpo_penalty_packed(2, None, None) == EINVAL
    for bad in (pen(z=None), pen(B=0), pen(n_part=0), pen(n_part=5), pen(penalty=d), pen(mean=None)):
        assert lib.rrl_rcpo_penalty_packed(2, arr(pen(), bad), None) == EINVAL
        assert lib.rrl_rcpo_penalty_packed(1, arr(bad), None) == EINVAL
        assert lib.rrl_rcpo_penalty(C.byref(bad), None) == EINVAL                                 # the solo entry: the same check
    assert lib.rrl_rcpo_penalty(None, None) == EINVAL

    gauss = lambda **k: _lib.rrl_policy_head_t(**dict(dict(kind=_lib.HEAD_GAUSS, B=8, head=d, n_part=1, eps=d, scale=d, bias=d,
                                                           action=d, ld_action=2), **k))
    stoch = lambda **k: _lib.rrl_policy_head_t(**dict(dict(kind=_lib.HEAD_STOCH, B=8, head=d, n_part=1, scale=d, bias=d,
                                                           action=d, ld_action=2, log_std=d), **k))
    group = lambda *a: (_lib.rrl_policy_head_t * len(a))(*a)
    heads = lambda *a: (P(_lib.rrl_policy_head_t) * len(a))(*[C.cast(x, P(_lib.rrl_policy_head_t)) for x in a])
    ok = group(gauss(), stoch())
    for S in (0, 17):
        assert lib.rrl_policy_heads_fwd_multi_packed(S, ints(2), heads(ok), None) == EINVAL
    assert lib.rrl_policy_heads_fwd_multi_packed(2, None, heads(ok, ok), None) == EINVAL
    assert lib.rrl_policy_heads_fwd_multi_packed(2, ints(2, 2), None, None) == EINVAL
    assert lib.rrl_policy_heads_fwd_multi_packed(2, ints(2, 0), heads(ok, ok), None) == EINVAL
    assert lib.rrl_policy_heads_fwd_multi_packed(2, ints(2, 5), heads(ok, ok), None) == EINVAL
    for bad in (gauss(eps=None), gauss(head=None), gauss(B=0), gauss(n_part=5), gauss(obs_in=d), stoch(log_std=None),
                gauss(kind=2), stoch(action=None)):
        assert lib.rrl_policy_heads_fwd_multi_packed(2, ints(2, 1), heads(ok, group(bad)), None) == EINVAL
        assert lib.rrl_policy_heads_fwd_multi_packed(1, ints(1), heads(group(bad)), None) == EINVAL
