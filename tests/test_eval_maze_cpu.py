"""Maze evaluation on the rollout kernel (rrl_eval_rollout_maze), the parts that need no GPU: the symbols are declared and
exported, the descriptor and the horizon are validated before any launch (stand-alone and packed entry), the switch matrix
(RRL_FAST_EVAL_MAZE=1 on top of RRL_FAST_EVAL=1) -- and the cases of tests/test_eval_maze_gpu.py are fair: restated whole in
float64 from oracle pieces (eval_maze_cases.rollout64), they hold rows that end by constraint, by success, by the env's horizon
alone and rows that survive, a gate that fires and one that does not, and few (row, step) pairs close enough to eps_safe for
the f32 gate to fall on either side.

As for Navigation, a case with one row has one fate and one gate outcome per step, and a reset = 1 case starts every row in the
reset box left of the first wall, 0.38 from the goal: no success within these T.  So the fates are proven for every reset = 0
case with n >= 17, the horizon's clause for every horizon-3 and horizon-1 case with n >= 17 (reset 0 and 1), both gate outcomes
for every recovery case with n >= 17, and the band bound for every case."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import arg_utils
import eval_maze_cases as MC
from recovery_rl_amd import _lib, fast_update

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, ERANGE = -1, -3
MF = ["--use_recovery", "--MF_recovery"]
MAZE = 2


# ---- ABI ---------------------------------------------------------------------------------------------------------------
def test_symbols_are_declared_exported_and_additive():
    src = open(os.path.join(ROOT, "include", "rrl_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"\bint\s+rrl_eval_rollout_maze\s*\(\s*const\s+rrl_eval_rollout_t\s*\*\s*\w+\s*,\s*int\s+horizon\s*,\s*void\s*\*",
                     code)
    assert re.search(r"\bint\s+rrl_eval_rollout_maze_packed\s*\(\s*int\s+S\s*,\s*const\s+rrl_eval_rollout_t\s*\*\s*\w+\s*,"
                     r"\s*const\s+int\s*\*\s*horizon\s*,\s*void\s*\*", code)
    for name in ("rrl_eval_rollout_maze", "rrl_eval_rollout_maze_packed"):
        assert name in _lib.EXPORTS
    assert _lib.ENV_MAZE == MAZE and re.search(r"RRL_ENV_MAZE\s*=\s*2\b", code)
    lib = _lib.load()
    assert lib.rrl_abi_version() == 8                       # additive: nothing existing changed layout
    assert lib.rrl_eval_rollout_maze.argtypes[:2] == [C.POINTER(_lib.rrl_eval_rollout_t), C.c_int]
    assert lib.rrl_eval_rollout_maze_packed.argtypes[:3] == [C.c_int, C.POINTER(_lib.rrl_eval_rollout_t), C.POINTER(C.c_int)]
    assert len(_lib.rrl_eval_rollout_t._fields_) == 47      # the same descriptor
    row = [l for l in open(os.path.join(ROOT, "INTEGRATION.md")) if l.startswith("| `rrl_eval_rollout_maze`")]
    assert len(row) == 1 and "rrl_eval_rollout_maze_packed" in row[0]


REQUIRED = ("pW1", "pb1", "pW2p", "pb2", "pW3", "pb3", "scale", "bias", "ret", "success", "violation", "steps")
QGROUP = ("qW1", "qb1", "qW2p", "qb2", "qW3", "qb3")
RGROUP = ("rW1", "rb1", "rW2p", "rb2", "rW3", "rb3", "rscale", "rbias", "rlog_std")


def _desc(groups="qr", **fields):
    """A well-formed Maze rrl_eval_rollout_t whose device pointers are dummy non-null integers (validation never follows them)."""
    d = 0x1000
    a = _lib.rrl_eval_rollout_t(n=8, T=101, H=256, d_obs=2, d_act=2, env_kind=MAZE, reset=1, **{k: d for k in REQUIRED})
    for k in (QGROUP if "q" in groups else ()) + (RGROUP if "r" in groups else ()):
        setattr(a, k, d)
    for k, v in fields.items():
        setattr(a, k, v)
    return a


def _solo(lib, a, horizon=100):
    return lib.rrl_eval_rollout_maze(C.byref(a), horizon, None)


def _packed(lib, a, horizon=100, S=2):
    """the descriptor (and horizon) under test as the LAST of S seeds, behind well-formed ones"""
    arr = (_lib.rrl_eval_rollout_t * S)(*([_desc()] * (S - 1) + [a]))
    return lib.rrl_eval_rollout_maze_packed(S, arr, (C.c_int * S)(*([100] * (S - 1) + [horizon])), None)


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
    # a Navigation kind is refused here, as Maze is by rrl_eval_rollout
    for fields in (dict(H=32), dict(H=512), dict(d_obs=3), dict(d_act=1), dict(n=0), dict(n=-4), dict(env_kind=0),
                   dict(env_kind=1), dict(env_kind=-1), dict(env_kind=3), dict(pW2p=0x1004), dict(qW2p=0x1008),
                   dict(rW2p=0x100c), dict(reset=0)):
        assert call(lib, _desc(**fields)) == EINVAL, fields
    for fields in (dict(T=0), dict(T=-1), dict(T=4097), dict(n=2 ** 22 + 1)):
        assert call(lib, _desc(**fields)) == ERANGE, fields
    for horizon in (0, -1, 2 ** 30 + 1):
        assert call(lib, _desc(), horizon) == ERANGE, horizon
    # an invalid field wins over a size or a horizon out of range, whatever the order of the struct
    assert call(lib, _desc(T=5000, H=32)) == EINVAL
    assert call(lib, _desc(n=2 ** 22 + 1, steps=None)) == EINVAL
    assert call(lib, _desc(T=0, qb3=None)) == EINVAL
    for fields in (dict(env_kind=0), dict(ret=None), dict(H=32), dict(rb1=None)):
        assert call(lib, _desc(**fields), 0) == EINVAL, fields
        assert call(lib, _desc(**fields), 2 ** 30 + 1) == EINVAL, fields


def test_packed_entry_checks_its_own_arguments():
    lib = _lib.load()
    one = (_lib.rrl_eval_rollout_t * 17)(*[_desc()] * 17)
    hor = (C.c_int * 17)(*[100] * 17)
    assert lib.rrl_eval_rollout_maze_packed(2, None, hor, None) == EINVAL
    assert lib.rrl_eval_rollout_maze_packed(2, one, None, None) == EINVAL           # a NULL horizon array
    for S in (0, -1, 17):
        assert lib.rrl_eval_rollout_maze_packed(S, one, hor, None) == ERANGE, S
    # every seed is checked, and an invalid field of a later seed wins over a size or horizon out of range of an earlier one
    arr = (_lib.rrl_eval_rollout_t * 3)(_desc(T=0), _desc(), _desc(ret=None))
    assert lib.rrl_eval_rollout_maze_packed(3, arr, hor, None) == EINVAL
    arr = (_lib.rrl_eval_rollout_t * 3)(_desc(), _desc(T=4097), _desc())
    assert lib.rrl_eval_rollout_maze_packed(3, arr, hor, None) == ERANGE
    arr = (_lib.rrl_eval_rollout_t * 3)(_desc(), _desc(), _desc(env_kind=1))
    assert lib.rrl_eval_rollout_maze_packed(3, arr, (C.c_int * 3)(0, 100, 100), None) == EINVAL
    arr = (_lib.rrl_eval_rollout_t * 3)(_desc(), _desc(), _desc())
    assert lib.rrl_eval_rollout_maze_packed(3, arr, (C.c_int * 3)(100, 0, 100), None) == ERANGE
    # S == 1 is the solo entry: the same codes
    assert lib.rrl_eval_rollout_maze_packed(1, arr, (C.c_int * 1)(0), None) == ERANGE
    # the Navigation entries still refuse a Maze descriptor
    assert lib.rrl_eval_rollout(C.byref(_desc()), None) == EINVAL
    assert lib.rrl_eval_rollout_packed(2, arr, None) == EINVAL


# ---- the switches ------------------------------------------------------------------------------------------------------
def _cfg(*flags, env="maze"):
    return arg_utils.get_args(["--env-name", env, "--gamma_safe", "0.5", "--eps_safe", "0.15", "--pos_fraction", "0.3",
                               "--hidden_size", "256", "--num_envs", "128"] + list(flags))


def _set(monkeypatch, name, value):
    if value is None:
        monkeypatch.delenv(name, raising=False)
    else:
        monkeypatch.setenv(name, value)


@pytest.mark.parametrize("fast,maze,flags,want", [
    ("1", "1", MF, "hip"),
    ("1", "1", [], "hip"),                                                   # no recovery policy: the task policy alone
    ("1", "1", MF + ["--Q_sampling_recovery"], "hip"),                       # model-free wins in the module code
    ("1", None, MF, "modules"),                                              # either switch alone, or neither
    ("1", "0", MF, "modules"),
    (None, "1", MF, "modules"),
    ("0", "1", MF, "modules"),
    (None, None, MF, "modules"),
    ("1", "1", ["--use_recovery", "--Q_sampling_recovery"], "modules"),
    ("1", "1", MF + ["--use_constraint_sampling"], "modules"),               # SQRL
    ("1", "1", ["--use_recovery"], "modules"),                               # model-based recovery
    ("1", "1", MF + ["--hidden_size", "32"], "modules"),
    ("1", "1", MF + ["--num_envs", "1"], "modules"),
    ("1", "1", MF + ["--no_fast_path"], "modules"),
])
def test_switch_matrix(monkeypatch, fast, maze, flags, want):
    _set(monkeypatch, "RRL_FAST_EVAL", fast)
    _set(monkeypatch, "RRL_FAST_EVAL_MAZE", maze)
    monkeypatch.setenv("RRL_FAST_BASELINES", "1")           # (so that --use_constraint_sampling alone would keep the fused path)
    assert fast_update.fast_eval_maze_enabled() == (maze == "1")
    assert fast_update.eval_rollout_path(_cfg(*flags)) == want
    if want == "hip":
        monkeypatch.delenv("RRL_FAST_BASELINES")
        monkeypatch.setenv("RRL_W2_FRAG", "0")
        assert fast_update.eval_rollout_path(_cfg(*flags)) == "hip"


@pytest.mark.parametrize("fast", ["1", None])
@pytest.mark.parametrize("env,flags,want", [
    ("navigation1", MF, "hip"), ("navigation2", [], "hip"), ("navigation1", ["--use_recovery"], "modules"),
    ("navigation2", MF + ["--hidden_size", "32"], "modules"), ("navigation1", MF + ["--num_envs", "1"], "modules")])
def test_navigation_answers_do_not_depend_on_the_new_switch(monkeypatch, fast, env, flags, want):
    _set(monkeypatch, "RRL_FAST_EVAL", fast)
    got = []
    for maze in (None, "0", "1"):
        _set(monkeypatch, "RRL_FAST_EVAL_MAZE", maze)
        got.append(fast_update.eval_rollout_path(_cfg(*flags, env=env)))
    assert got == [want if fast == "1" else "modules"] * 3


# ---- fairness of the generated cases -----------------------------------------------------------------------------------
def test_the_case_table_is_the_issues():
    cases = MC.all_cases()
    assert len(cases) == len(set(cases)) == 19 * 2 * 2
    assert {c[:3] for c in cases} == {(n, T, 100) for n in (1, 17, 64, 65, 130) for T in (1, 2, 7)} | \
        {(65, 7, 3), (130, 7, 3), (17, 1, 1), (65, 101, 100)}


def test_start_states_hold_every_fate():
    pos = MC.start_states(130)
    touch = np.array([MC.co.maze_contact(x, y) for x, y in pos], bool)
    d = np.array([MC.co.maze_distance(x, y) for x, y in pos])
    assert touch[2::4].all() and not touch[0::4].any() and not touch[1::4].any() and not touch[3::4].any()
    # next to the goal: a legal move is at most 0.1 * 0.2467 per axis, so sqrt(mean(sq)) stays below 0.005 + 0.0247 < 0.03
    assert (np.hypot(pos[1::4, 0] - 0.25, pos[1::4, 1]) <= 0.005).all() and (d[1::4] < 0.005).all()
    # left of the wall at x = -0.1 (touched from x = -0.13 on), within its y extent and clear of the arena plane y = -0.275
    near = pos[0::4]
    assert ((near[:, 0] < -0.13) & (near[:, 0] > -0.173) & (near[:, 1] > -0.275) & (near[:, 1] < -0.13)).all()
    for n in MC.NS:
        assert MC.start_states(n).shape == (n, 2)


@pytest.mark.parametrize("n,T,horizon,recovery,reset", MC.all_cases())
def test_cases_are_fair(n, T, horizon, recovery, reset):
    r = MC.rollout64(n, T, horizon, recovery, reset)
    pairs = int(r["alive"].sum())
    assert r["alive"][0].all() and pairs >= n and (r["steps"] <= horizon).all()
    if recovery:
        band = int((r["alive"] & (np.abs(r["q"] - MC.eps_safe(n, reset)) <= MC.BAND)).sum())
        assert band <= 0.02 * pairs, (band, pairs)          # the share the GPU test may leave out of the gate comparison
    if recovery and n >= 17:
        # eps_safe is a central split of the first-step q64 of the case's own rows: both outcomes on step 0, reset = 1 included
        assert n // 4 <= r["gate"][0].sum() <= n - n // 4
        assert r["gate"].any() and (r["alive"] & ~r["gate"]).any()
    elif recovery:
        assert n == 1 and r["gate"][0].sum() in (0, 1)
    # a row ends in exactly one way, or not at all within T (a row at the goal may touch the arena plane behind it as well)
    ended = r["constraint"] | r["success"] | r["timeout"]
    assert np.array_equal(ended, ~r["survived"]) and not (r["timeout"] & (r["constraint"] | r["success"])).any()
    if horizon < T or horizon == 1:
        # the clause only Maze has: the env's own horizon ends rows that are neither successes nor violations
        assert not r["survived"].any() and (r["steps"][r["timeout"]] == horizon).all()
        if n >= 17 and horizon < MC.HORIZON:
            assert r["timeout"].any()
    else:
        assert not r["timeout"].any()                       # T < horizon: the clock cannot run out
    if reset == 0 and n >= 17:
        assert r["success"][1::4].all() and (r["steps"][1::4] == 1).all()
        assert r["constraint"][2::4].all() and (r["steps"][2::4] == 1).all()
        far = r["timeout"][3::4] if horizon < 7 else r["survived"][3::4]
        if T <= 7:
            assert far.all()                                # alive through 7 steps, or ended by the horizon with neither flag
        if T >= 2:
            # rows next to the wall are carried in by the executed action, not placed there: some on a later step
            assert r["constraint"][0::4].any() and r["alive"][1][0::4].any()
        if T >= 7:
            assert r["constraint"][0::4].all()
    elif reset == 1:
        # every row starts in the reset box x in -0.22 .. -0.13, more than 0.38 from the goal: no success within these T
        assert not r["success"].any() or T > 7
