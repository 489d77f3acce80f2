"""Policy evaluation as one rollout kernel (rrl_eval_rollout), the parts that need no GPU: the symbols are declared and
exported, the descriptor is validated before any launch (stand-alone and packed entry), the switch matrix (which
configurations evaluate on the kernel) -- and the cases of tests/test_eval_rollout_gpu.py are fair: restated whole in float64
from oracle pieces (eval_cases.rollout64), they hold rows that end by constraint, by success and rows that survive, a gate that
fires and one that does not, and few (row, step) pairs close enough to eps_safe for the f32 gate to fall on either side.

What a case CAN show depends on its shape.  A case with one row has one fate, and a reset = 1 case starts every row at
(-50, 0) + N(0, I), fifty steps from the goal: neither can hold a success, a constraint and a survivor at once, whatever the
weights.  So the three fates are proven for every reset = 0 case with n >= 17 (the start states of eval_cases.start_states put
every fate into any four consecutive rows) and for reset = 1 and n = 1 over what they can reach (stated at the assertions).
The two gate outcomes are proven for EVERY case with the recovery group and n >= 17, reset = 1 included: eps_safe is a
central split of the first-step q64 of the case's own rows (eval_cases.eps_safe).  A case with n = 1 has one row and one outcome per step: it cannot show both.
The band bound is proven for every case."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import arg_utils
import eval_cases as EC
from recovery_rl_amd import _lib, fast_update

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, ERANGE = -1, -3
MF = ["--use_recovery", "--MF_recovery"]
CTYPES = {"int": C.c_int, "float": C.c_float, "uint64_t": C.c_uint64}


# ---- ABI ---------------------------------------------------------------------------------------------------------------
def test_symbols_are_declared_exported_and_additive():
    src = open(os.path.join(ROOT, "include", "rrl_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"\bint\s+rrl_eval_rollout\s*\(\s*const\s+rrl_eval_rollout_t\s*\*\s*\w+\s*,\s*void\s*\*", code)
    assert re.search(r"\bint\s+rrl_eval_rollout_packed\s*\(\s*int\s+S\s*,\s*const\s+rrl_eval_rollout_t\s*\*", code)
    assert re.search(r"RRL_STREAM_EVAL\s*=\s*12\b", code)
    for name in ("rrl_eval_rollout", "rrl_eval_rollout_packed"):
        assert name in _lib.EXPORTS
    assert "eval_kernels.hip" in _lib.HIP_SOURCES
    assert _lib.STREAM_EVAL == EC.STREAM_EVAL == 12
    lib = _lib.load()
    assert lib.rrl_abi_version() == 8                       # additive: nothing existing changed layout
    assert lib.rrl_eval_rollout.argtypes[0] == C.POINTER(_lib.rrl_eval_rollout_t)
    assert lib.rrl_eval_rollout_packed.argtypes[:2] == [C.c_int, C.POINTER(_lib.rrl_eval_rollout_t)]
    row = [l for l in open(os.path.join(ROOT, "INTEGRATION.md")) if l.startswith("| `rrl_eval_rollout`")]
    assert len(row) == 1 and "recovery_rl/experiment.py:493-538" in row[0]


def test_struct_layout_follows_the_header():
    """The ctypes fields, in order, are the header's members (names; every pointer is a void*, the rest by C type)."""
    src = open(os.path.join(ROOT, "include", "rrl_hip.h")).read()
    body = re.search(r"typedef struct \{((?:(?!typedef).)*?)\} rrl_eval_rollout_t;", src, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    want = []
    for decl in filter(None, (d.strip() for d in body.split(";"))):
        base, rest = re.match(r"(?:const\s+)?(\w+)\s*(.*)", decl, flags=re.S).groups()
        for name in rest.split(","):
            name = name.strip()
            want.append((name.lstrip("* "), C.c_void_p if name.startswith("*") else CTYPES[base]))
    assert [(n, t) for n, t in _lib.rrl_eval_rollout_t._fields_] == want
    assert len(want) == 47
    zero = _lib.rrl_eval_rollout_t()                      # a zero-initialised struct has every option off
    assert not any(getattr(zero, n) for n, _ in want)


REQUIRED = ("pW1", "pb1", "pW2p", "pb2", "pW3", "pb3", "scale", "bias", "ret", "success", "violation", "steps")
QGROUP = ("qW1", "qb1", "qW2p", "qb2", "qW3", "qb3")
RGROUP = ("rW1", "rb1", "rW2p", "rb2", "rW3", "rb3", "rscale", "rbias", "rlog_std")


def _desc(groups="qr", **fields):
    """A well-formed rrl_eval_rollout_t whose device pointers are dummy non-null integers (validation never follows them)."""
    d = 0x1000
    a = _lib.rrl_eval_rollout_t(n=8, T=101, H=256, d_obs=2, d_act=2, env_kind=0, reset=1, **{k: d for k in REQUIRED})
    for k in (QGROUP if "q" in groups else ()) + (RGROUP if "r" in groups else ()):
        setattr(a, k, d)
    for k, v in fields.items():
        setattr(a, k, v)
    return a


def _solo(lib, a):
    return lib.rrl_eval_rollout(C.byref(a), None)


def _packed(lib, a, S=2):
    """the descriptor under test as the LAST of S seeds, behind well-formed ones"""
    arr = (_lib.rrl_eval_rollout_t * S)(*([_desc()] * (S - 1) + [a]))
    return lib.rrl_eval_rollout_packed(S, arr, None)


@pytest.mark.parametrize("call", [_solo, _packed])
def test_descriptor_validation_without_gpu(call):
    lib = _lib.load()
    for name in REQUIRED:
        assert call(lib, _desc(**{name: None})) == EINVAL, name
    # a group given only in part, from either end; the recovery policy needs the gate that selects it
    for group in (QGROUP, RGROUP):
        for name in group:
            assert call(lib, _desc(**{name: None})) == EINVAL, name
            assert call(lib, _desc("r" if group is QGROUP else "q", **{name: 0x1000})) == EINVAL, name
    assert call(lib, _desc("r")) == EINVAL
    for fields in (dict(H=32), dict(H=512), dict(d_obs=3), dict(d_act=1), dict(n=0), dict(n=-4), dict(env_kind=2),
                   dict(env_kind=-1), dict(pW2p=0x1004), dict(qW2p=0x1008), dict(rW2p=0x100c), dict(reset=0)):
        assert call(lib, _desc(**fields)) == EINVAL, fields
    for fields in (dict(T=0), dict(T=-1), dict(T=4097), dict(n=2 ** 22 + 1)):
        assert call(lib, _desc(**fields)) == ERANGE, fields
    # an invalid field wins over a size out of range, whatever the order of the struct
    assert call(lib, _desc(T=5000, H=32)) == EINVAL
    assert call(lib, _desc(n=2 ** 22 + 1, steps=None)) == EINVAL
    assert call(lib, _desc(T=0, qb3=None)) == EINVAL


def test_packed_entry_checks_its_own_arguments():
    lib = _lib.load()
    one = (_lib.rrl_eval_rollout_t * 17)(*[_desc()] * 17)
    assert lib.rrl_eval_rollout_packed(2, None, None) == EINVAL
    for S in (0, -1, 17):
        assert lib.rrl_eval_rollout_packed(S, one, None) == ERANGE, S
    # every seed is checked, and an invalid field of a later seed wins over a size out of range of an earlier one
    arr = (_lib.rrl_eval_rollout_t * 3)(_desc(T=0), _desc(), _desc(ret=None))
    assert lib.rrl_eval_rollout_packed(3, arr, None) == EINVAL
    arr = (_lib.rrl_eval_rollout_t * 3)(_desc(), _desc(T=4097), _desc())
    assert lib.rrl_eval_rollout_packed(3, arr, None) == ERANGE


# ---- the switch --------------------------------------------------------------------------------------------------------
def _cfg(*flags, env="navigation1"):
    return arg_utils.get_args(["--env-name", env, "--gamma_safe", "0.8", "--eps_safe", "0.3", "--hidden_size", "256",
                               "--num_envs", "128"] + list(flags))


@pytest.mark.parametrize("switch,env,flags,want", [
    ("1", "navigation1", MF, "hip"),
    ("1", "navigation2", MF, "hip"),
    ("1", "navigation1", [], "hip"),                                                   # no recovery policy: the task policy alone
    ("1", "navigation1", MF + ["--Q_sampling_recovery"], "hip"),                       # model-free wins in the module code
    (None, "navigation1", MF, "modules"),                                              # the switch is opt-in
    ("0", "navigation1", MF, "modules"),
    ("1", "maze", MF, "modules"),
    ("1", "navigation1", ["--use_recovery", "--Q_sampling_recovery"], "modules"),
    ("1", "navigation1", ["--use_recovery"], "modules"),                               # model-based recovery
    ("1", "navigation1", MF + ["--use_constraint_sampling"], "modules"),
    ("1", "navigation1", MF + ["--hidden_size", "32"], "modules"),
    ("1", "navigation1", MF + ["--hidden_size", "512"], "modules"),
    ("1", "navigation1", MF + ["--no_fast_path"], "modules"),
    ("1", "navigation1", MF + ["--automatic_entropy_tuning", "True"], "modules"),
    ("1", "navigation1", MF + ["--num_envs", "1"], "modules"),
])
def test_switch_matrix(monkeypatch, switch, env, flags, want):
    if switch is None:
        monkeypatch.delenv("RRL_FAST_EVAL", raising=False)
    else:
        monkeypatch.setenv("RRL_FAST_EVAL", switch)
    monkeypatch.setenv("RRL_FAST_BASELINES", "1")           # (so that --use_constraint_sampling alone would keep the fused path)
    assert fast_update.fast_eval_enabled() == (switch == "1")
    assert fast_update.eval_rollout_path(_cfg(*flags, env=env)) == want
    if want == "hip":
        monkeypatch.delenv("RRL_FAST_BASELINES")            # the Recovery-RL configurations need no other switch ...
        monkeypatch.setenv("RRL_W2_FRAG", "0")              # ... and the rollout keeps its own fragment-order copies
        assert fast_update.eval_rollout_path(_cfg(*flags, env=env)) == "hip"


# ---- fairness of the generated cases -----------------------------------------------------------------------------------
def test_the_case_table_is_the_issues():
    cases = EC.all_cases()
    assert len(cases) == len(set(cases)) == 16 * 2 * 2 * 2
    assert {(n, T) for _, n, T, _, _ in cases} == {(n, T) for n in (1, 17, 64, 65, 130) for T in (1, 2, 7)} | {(65, 101)}


def test_start_states_hold_every_fate():
    for kind in EC.KINDS:
        pos = EC.start_states(kind, 130)
        r = np.hypot(pos[:, 0], pos[:, 1])
        inside = np.array([EC.co.obstacle(kind, x, y) for x, y in pos], bool)
        assert (r[1::4] < 3).all() and inside[2::4].all() and not inside[0::4].any() and not inside[3::4].any()
        # far rows: no obstacle and no goal within 102 unit steps (+ 102 noise draws of sd 0.05, never 0.1 in sum per step)
        far = pos[3::4]
        assert ((far[:, 1] if kind == "navigation1" else far[:, 0]) > 10 + 102 * 1.1).all()
        for n in EC.NS:                                      # (a smaller case is not a prefix of a larger one: own draws)
            assert EC.start_states(kind, n).shape == (n, 2)


@pytest.mark.parametrize("kind,n,T,recovery,reset", EC.all_cases())
def test_cases_are_fair(kind, n, T, recovery, reset):
    r = EC.rollout64(kind, n, T, recovery, reset)
    pairs = int(r["alive"].sum())
    assert r["alive"][0].all() and pairs >= n
    if recovery:
        band = int((r["alive"] & (np.abs(r["q"] - EC.eps_safe(kind, n, reset)) <= EC.BAND)).sum())
        assert band <= 0.02 * pairs, (band, pairs)          # the share the GPU test may leave out of the gate comparison
    if recovery and n >= 17:
        # eps_safe is a central split of the first-step q64 of the case's own rows: both outcomes on step 0 already, at least
        # a quarter of the rows each, reset = 1 included
        assert n // 4 <= r["gate"][0].sum() <= n - n // 4
        assert r["gate"].any() and (r["alive"] & ~r["gate"]).any()
    elif recovery:
        # one row has one gate outcome per step; over the n = 1 cases of a (kind, reset) whatever the float64 rollout says
        assert n == 1 and r["gate"][0].sum() in (0, 1)
    if reset == 0 and n >= 17:
        assert r["constraint"].any() and r["success"].any() and r["survived"].any()
        assert r["constraint"][2::4].all() and r["success"][1::4].all() and r["survived"][3::4].all()
        if T >= 2:
            # rows next to the obstacle are carried in by the executed action, not placed there: some on a later step
            assert r["constraint"][0::4].any() and (r["alive"][1][0::4]).any()
    elif reset == 0:
        # one row (the one next to the obstacle): alive at step 0; its fate is the float64 rollout's, whatever it is
        assert n == 1 and r["constraint"].sum() + r["success"].sum() + r["survived"].sum() == 1
    else:
        # reset = 1: every row starts at (-50, 0) + N(0, I), 46 steps from the goal at least -- no success within these T
        # (T = 101 included: the policies push towards the obstacle); the rows split into survivors and, from T = 7 on in
        # Navigation 1 (y = 5 is seven pushed steps away), rows that end by constraint
        assert not r["success"].any() and (r["constraint"] | r["survived"]).all()
        if kind == "navigation1" and T >= 7 and n >= 17:
            assert r["constraint"].any()
        if kind == "navigation1" and T == 7 and n >= 17:
            assert r["survived"].any()
