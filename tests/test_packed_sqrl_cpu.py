"""Seed packing for SQRL (RRL_PACK_SQRL=1), the parts that need no GPU: rrl_sqrl_act_packed is declared, exported and listed
in the header's packed-launch table at the unchanged ABI version, it checks every seed's descriptor before anything is stored
or launched, PackedLoop turns the "sqrl" ops of the seeds' tapes into one stage calling it and refuses more than 8 such
seeds, and run_packed lifts its refusal of --use_constraint_sampling only under the switch and inside the limits."""
import ctypes as C
import os
import re
import types

import pytest
import torch

import arg_utils
from recovery_rl_amd import _lib, fast_update
from recovery_rl_amd.experiment import run_packed
from recovery_rl_amd.packed import PackedLoop
from test_packed_baselines_cpu import calls, taped, updater  # noqa: F401  (calls: the library-call recorder, a fixture)
from test_sqrl_act_cpu import SQRL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, ERANGE = -1, -3


# ---- ABI ---------------------------------------------------------------------------------------------------------------
def test_symbol_is_declared_exported_and_listed_at_the_same_abi():
    src = open(os.path.join(ROOT, "include", "rrl_hip.h")).read()
    table = src[src.index("Packed launches:"):].split("typedef")[0]
    assert "rrl_sqrl_act_packed" in table and "rrl_sqrl_act " in table.split("rrl_sqrl_act_packed")[1]   # ... with its twin
    assert re.search(r"\bk\b", table.split("rrl_sqrl_act_packed")[1])                                  # and the same-k rule
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    decl = re.search(r"\bint\s+rrl_sqrl_act_packed\s*\(\s*int\s+S\s*,\s*const\s+rrl_sqrl_act_t\s*\*\s*\w+\s*,\s*void\s*\*", code)
    assert decl and decl.start() > re.search(r"\bint\s+rrl_sqrl_act\s*\(", code).start()       # declared after rrl_sqrl_act
    assert "rrl_sqrl_act_packed" in _lib.EXPORTS
    lib = _lib.load()
    assert lib.rrl_abi_version() == 8                                  # additive: no existing struct changed layout
    assert lib.rrl_sqrl_act_packed.argtypes == [C.c_int, C.POINTER(_lib.rrl_sqrl_act_t), C.c_void_p]
    assert "rrl_sqrl_act_packed" in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def desc(**fields):
    """A well-formed rrl_sqrl_act_t whose device pointers are dummy non-null integers (validation never follows them)."""
    d = 0x1000
    a = _lib.rrl_sqrl_act_t(n=8, k=100, H=256, d_obs=2, d_act=2, obs=d, head=d, n_part=1, part_stride=0, scale=d, bias=d,
                            W1=d, b1=d, W2p=d, b2=d, W3=d, b3=d, eps_safe=0.3, action=d)
    for k, v in fields.items():
        setattr(a, k, v)
    return a


def seeds(*descs):
    return (_lib.rrl_sqrl_act_t * len(descs))(*descs)


def test_every_seed_is_validated_without_gpu():
    lib = _lib.load()
    for S in (0, -1, 17):
        assert lib.rrl_sqrl_act_packed(S, seeds(*[desc() for _ in range(17)]), None) == EINVAL, S
    assert lib.rrl_sqrl_act_packed(2, None, None) == EINVAL
    # one k per call: the kernel's row tiles are a template parameter (100 and 96 differ in them; 100 and 97 do not, and the
    # rule is the same k)
    assert lib.rrl_sqrl_act_packed(2, seeds(desc(k=100), desc(k=96)), None) == EINVAL
    assert lib.rrl_sqrl_act_packed(2, seeds(desc(k=100), desc(k=97)), None) == EINVAL
    assert lib.rrl_sqrl_act_packed(3, seeds(desc(), desc(), desc(k=17)), None) == EINVAL
    # one bad seed, wherever it stands, refuses the whole call with the stand-alone entry's code
    for bad, code in ((dict(W2p=None), EINVAL), (dict(H=32), EINVAL), (dict(k=129), ERANGE), (dict(W2p=0x1008), EINVAL),
                      (dict(n=0), EINVAL), (dict(n_part=5), EINVAL), (dict(action=None), EINVAL), (dict(n=2 ** 25, k=128), ERANGE)):
        assert lib.rrl_sqrl_act(C.byref(desc(**bad)), None) == code, bad
        for S in (1, 2, 3, 8, 16):
            for at in {0, S // 2, S - 1}:
                group = [desc() for _ in range(S)]
                group[at] = desc(**bad)
                assert lib.rrl_sqrl_act_packed(S, seeds(*group), None) == code, (bad, S, at)


# ---- PackedLoop --------------------------------------------------------------------------------------------------------
def sqrl_iteration_tape(calls, n=128):
    """The acting pass and the SAC update of one SQRL iteration on the launch tape (nothing runs: the library is the recorder)."""
    fast, batch, e1, e2, nu = updater(SQRL, recovery=False)
    fast.qrisk.w2p = torch.empty(2 * 256 * 256)              # (a CPU FlatNet keeps no fragment-order copy)
    actor = fast_update.FastActor(fast, n)

    def iteration():
        actor.act_sqrl(torch.zeros(n, 2), 0.3)
        fast.sac_update(batch, e1, e2, nu=nu, grouped=True)
    got, tape = taped(calls, iteration)
    return got, tape, (fast, actor)


def test_build_stages_packs_the_acting_launch(calls):
    S = 3
    tapes, keep = [], []
    for _ in range(S):
        got, tape, alive = sqrl_iteration_tape(calls)
        tapes.append(tape), keep.append(alive)
    kinds = [op[0] for op in tapes[0]]
    assert kinds.count("sqrl") == 1 and "heads" not in kinds and "unsupported" not in kinds
    assert kinds[:2] == ["forward", "sqrl"] and kinds.count("adam_duals") == 1          # the update is LR's
    assert got.count("sqrl_act") == 1 and "policy_heads_fwd_multi" not in got
    packed = PackedLoop([types.SimpleNamespace(sqrl_hip=True) for _ in range(S)])
    packed.tapes = tapes
    packed.stages = packed._build_stages()
    assert len(packed.stages) == len(kinds) == packed.launches        # one launch per kind of this tape (S <= PAIR_MAX_SEEDS)
    stage = [st for st in packed.stages if st[2][0][0] == "sqrl"]
    assert len(stage) == 1
    fn, args, ops = stage[0]
    assert args[0] == S and isinstance(args[1], _lib.rrl_sqrl_act_t * S)
    for s in range(S):                                                 # seed s's stand-alone descriptor, byte for byte
        assert bytes(args[1][s]) == bytes(tapes[s][1][1]) and args[1][s].counter_dev == keep[s][1].sqrl_tick.data_ptr()
    assert len({args[1][s].counter_dev for s in range(S)}) == S
    del calls[:]
    packed.launch()
    assert calls.count("sqrl_act_packed") == 1 and "sqrl_act" not in calls and len(calls) == len(kinds)
    assert calls[1] == "sqrl_act_packed" and calls[0] == "mlp3_forward_multi_packed"


def test_packed_loop_refuses_nine_sqrl_loops_by_name():
    sqrl = lambda: types.SimpleNamespace(sqrl_hip=True, agent=types.SimpleNamespace(fast=None))
    other = lambda: types.SimpleNamespace(sqrl_hip=False, agent=types.SimpleNamespace(fast=None))
    with pytest.raises(ValueError, match=r"SQRL.*at most 8 seeds"):
        PackedLoop([sqrl() for _ in range(9)])
    with pytest.raises(ValueError, match=r"at most 8 seeds"):
        PackedLoop([other() for _ in range(8)] + [sqrl()])
    assert PackedLoop([sqrl() for _ in range(8)]).S == 8
    assert PackedLoop([other() for _ in range(9)]).S == 9             # the limit is SQRL's


# ---- run_packed --------------------------------------------------------------------------------------------------------
BASE = ["--env-name", "navigation1", "--cuda", "--num_envs", "128", "--gamma_safe", "0.8", "--eps_safe", "0.3"]


@pytest.mark.parametrize("pack,fast_sqrl,extra,seeds_per_gpu,names", [
    (None, "1", [], 2, "no packed form"),                                     # the switch unset: today's message
    ("0", "1", [], 2, "no packed form"),
    ("1", None, [], 2, "RRL_FAST_SQRL"),
    ("1", "0", [], 2, "RRL_FAST_SQRL"),
    ("1", "1", ["--use_recovery", "--MF_recovery"], 2, "use_recovery"),
    ("1", "1", ["--hidden_size", "32"], 2, "hidden_size"),
    ("1", "1", [], 9, "at most 8 seeds"),
])
def test_run_packed_switch_matrix(monkeypatch, tmp_path, pack, fast_sqrl, extra, seeds_per_gpu, names):
    monkeypatch.setenv("RRL_FAST_BASELINES", "1")
    monkeypatch.delenv("RRL_W2_FRAG", raising=False)
    for name, val in (("RRL_PACK_SQRL", pack), ("RRL_FAST_SQRL", fast_sqrl)):
        if val is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, val)
    cfg = arg_utils.get_args(BASE + ["--seeds_per_gpu", str(seeds_per_gpu), "--logdir", str(tmp_path)] + SQRL + extra)
    with pytest.raises(ValueError, match=names) as err:
        run_packed(cfg)
    assert "use_constraint_sampling" in str(err.value)
    assert not os.listdir(tmp_path)                       # refused before anything was set up


def test_run_packed_names_the_fused_path_when_it_is_missing(monkeypatch, tmp_path):
    monkeypatch.setenv("RRL_PACK_SQRL", "1")
    monkeypatch.setenv("RRL_FAST_SQRL", "1")
    monkeypatch.delenv("RRL_FAST_BASELINES", raising=False)
    cfg = arg_utils.get_args(BASE + ["--seeds_per_gpu", "2", "--logdir", str(tmp_path)] + SQRL)
    with pytest.raises(ValueError, match="RRL_FAST_BASELINES") as err:
        run_packed(cfg)
    assert "use_constraint_sampling" in str(err.value) and not os.listdir(tmp_path)
