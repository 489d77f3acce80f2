"""Q-sampling recovery on the evaluation rollout kernel (rrl_eval_rollout_qs[_packed]), the parts that need no GPU: the ABI
is declared, exported and additive; every descriptor check returns its code before any launch; the path table of
eval_rollout_path over the three switches; and the fairness of the cases of eval_qsample_cases.py, from the float64 rollout
with the regenerated stream-13 candidates, which tests/test_eval_qsample_gpu.py measures the kernels on."""
import ctypes as C
import itertools
import os
import re

import numpy as np
import pytest

import arg_utils
import eval_qsample_cases as QC
from recovery_rl_amd import _lib, fast_update
from test_qsample_act_cpu import BOXES, STREAM_QSAMPLE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, ERANGE = -1, -3
REQUIRED = ("pW1", "pb1", "pW2p", "pb2", "pW3", "pb3", "scale", "bias", "ret", "success", "violation", "steps")
QGROUP = ("qW1", "qb1", "qW2p", "qb2", "qW3", "qb3")
RGROUP = ("rW1", "rb1", "rW2p", "rb2", "rW3", "rb3", "rscale", "rbias", "rlog_std")


# ---- ABI ---------------------------------------------------------------------------------------------------------------
def test_symbols_are_declared_exported_and_additive():
    src = open(os.path.join(ROOT, "include", "rrl_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"\bint\s+rrl_eval_rollout_qs\s*\(\s*const\s+rrl_eval_rollout_qs_t\s*\*\s*\w*\s*,\s*void\s*\*", code)
    assert re.search(r"\bint\s+rrl_eval_rollout_qs_packed\s*\(\s*int\s+\w+\s*,\s*const\s+rrl_eval_rollout_qs_t\s*\*", code)
    assert re.search(r"RRL_STREAM_EVAL_QSAMPLE\s*=\s*13\b", code)
    for name in ("rrl_eval_rollout_qs", "rrl_eval_rollout_qs_packed"):
        assert name in _lib.EXPORTS
        assert name in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert _lib.STREAM_EVAL_QSAMPLE == QC.STREAM_EVAL_QSAMPLE == 13
    lib = _lib.load()
    assert lib.rrl_abi_version() == 8                       # additive: nothing existing changed layout
    assert lib.rrl_eval_rollout_qs.argtypes[0] == C.POINTER(_lib.rrl_eval_rollout_qs_t)
    assert lib.rrl_eval_rollout_qs_packed.argtypes[1] == C.POINTER(_lib.rrl_eval_rollout_qs_t)


def test_struct_layout_follows_the_header_and_the_base_is_unchanged():
    src = open(os.path.join(ROOT, "include", "rrl_hip.h")).read()
    body = re.search(r"typedef struct \{((?:(?!typedef).)*?)\} rrl_eval_rollout_qs_t;", src, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    want = []
    ctypes_of = {"int": C.c_int, "rrl_eval_rollout_t": _lib.rrl_eval_rollout_t}
    for decl in filter(None, (d.strip() for d in body.split(";"))):
        base, rest = re.match(r"(?:const\s+)?(\w+)\s*(.*)", decl, flags=re.S).groups()
        for name in rest.split(","):
            name = name.strip()
            want.append((name.lstrip("* "), C.c_void_p if name.startswith("*") or base.endswith("*") else ctypes_of[base]))
    assert [(n, t) for n, t in _lib.rrl_eval_rollout_qs_t._fields_] == want
    assert [n for n, _ in want] == ["base", "k", "horizon", "lo", "hi", "tr_pick", "tr_q"]
    # the base descriptor stays byte for byte: 7 ints (+ pad), 15 pointers, a float (+ pad), 9 pointers, a float (+ pad),
    # two uint64 and 12 pointers on an LP64 target
    assert C.sizeof(_lib.rrl_eval_rollout_t) == 32 + 15 * 8 + 8 + 9 * 8 + 8 + 16 + 12 * 8 == 352
    assert len(_lib.rrl_eval_rollout_t._fields_) == 47
    assert _lib.rrl_eval_rollout_qs_t.base.offset == 0 and _lib.rrl_eval_rollout_qs_t.k.offset == 352
    assert C.sizeof(_lib.rrl_eval_rollout_qs_t) == 352 + 8 + 4 * 8


def _desc(kind=0, **fields):
    """A well-formed rrl_eval_rollout_qs_t whose device pointers are dummy non-null integers (validation never follows them).
    Fields of the base descriptor and of the Q-sampling struct are told apart by name."""
    d = 0x1000
    base = _lib.rrl_eval_rollout_t(n=8, T=101, H=256, d_obs=2, d_act=2, env_kind=kind, reset=1, eps_safe=0.3,
                                   **{k: d for k in REQUIRED + QGROUP})
    own = dict(k=1000, horizon=100 if kind == 2 else 0, lo=d, hi=d)
    for k, v in fields.items():
        if k in own or k in ("tr_pick", "tr_q"):
            own[k] = v
        else:
            setattr(base, k, v)
    return _lib.rrl_eval_rollout_qs_t(base=base, **own)


def _solo(lib, a):
    return lib.rrl_eval_rollout_qs(C.byref(a), None)


def _packed(lib, a, S=2):
    """the descriptor under test as the LAST of S seeds, behind well-formed ones of its env family"""
    arr = (_lib.rrl_eval_rollout_qs_t * S)(*([_desc(a.base.env_kind if a.base.env_kind == 2 else 0)] * (S - 1) + [a]))
    return lib.rrl_eval_rollout_qs_packed(S, arr, None)


@pytest.mark.parametrize("call", [_solo, _packed])
@pytest.mark.parametrize("kind", [0, 1, 2])
def test_descriptor_validation_without_gpu(call, kind):
    lib = _lib.load()
    # ---- everything rrl_eval_rollout / _maze check on base ----
    for name in REQUIRED:
        assert call(lib, _desc(kind, **{name: None})) == EINVAL, name
    for fields in (dict(H=32), dict(H=512), dict(d_obs=3), dict(d_act=1), dict(n=0), dict(n=-4), dict(env_kind=3),
                   dict(env_kind=-1), dict(pW2p=0x1004), dict(qW2p=0x1008), dict(reset=0)):
        assert call(lib, _desc(kind, **fields)) == EINVAL, fields
    for fields in (dict(T=0), dict(T=-1), dict(T=4097), dict(n=2 ** 22 + 1, k=1)):
        assert call(lib, _desc(kind, **fields)) == ERANGE, fields
    # ---- its own: the box, a Q_risk group that is missing (in part or whole), any pointer of the recovery group ----
    for name in ("lo", "hi") + QGROUP:
        assert call(lib, _desc(kind, **{name: None})) == EINVAL, name
    assert call(lib, _desc(kind, **{name: None for name in QGROUP})) == EINVAL
    for name in RGROUP:
        assert call(lib, _desc(kind, **{name: 0x1000})) == EINVAL, name
    assert call(lib, _desc(kind, **{name: 0x1000 for name in RGROUP})) == EINVAL
    for fields in (dict(k=0), dict(k=-1), dict(k=1025), dict(n=2 ** 22, k=1024), dict(n=2 ** 22, k=1024, T=1)):
        assert call(lib, _desc(kind, **fields)) == ERANGE, fields
    if kind == 2:       # (Navigation ignores the horizon: every Navigation launch of the GPU tests passes 0)
        for horizon in (0, -1, 2 ** 30 + 1):
            assert call(lib, _desc(kind, horizon=horizon)) == ERANGE, horizon
    # ---- an invalid field wins over a size out of range, whatever the order of the struct ----
    assert call(lib, _desc(kind, k=5000, H=32)) == EINVAL
    assert call(lib, _desc(kind, k=0, lo=None)) == EINVAL
    assert call(lib, _desc(kind, T=0, hi=None)) == EINVAL
    assert call(lib, _desc(kind, T=5000, rW1=0x1000)) == EINVAL
    assert call(lib, _desc(kind, n=2 ** 22 + 1, steps=None)) == EINVAL
    assert call(lib, _desc(kind, horizon=-5, k=0, qb3=None)) == EINVAL


def test_entries_check_their_own_arguments():
    lib = _lib.load()
    assert lib.rrl_eval_rollout_qs(None, None) == EINVAL
    one = (_lib.rrl_eval_rollout_qs_t * 17)(*[_desc()] * 17)
    assert lib.rrl_eval_rollout_qs_packed(2, None, None) == EINVAL
    for S in (0, -1, 17):
        assert lib.rrl_eval_rollout_qs_packed(S, one, None) == ERANGE, S
    # every seed is checked, and an invalid field of a later seed wins over a size out of range of an earlier one
    arr = (_lib.rrl_eval_rollout_qs_t * 3)(_desc(k=0), _desc(), _desc(lo=None))
    assert lib.rrl_eval_rollout_qs_packed(3, arr, None) == EINVAL
    arr = (_lib.rrl_eval_rollout_qs_t * 3)(_desc(), _desc(1, k=1025), _desc())
    assert lib.rrl_eval_rollout_qs_packed(3, arr, None) == ERANGE
    # Navigation 1 and 2 go together; Navigation and Maze do not, and that wins over a size out of range too
    for kinds in ((0, 2), (2, 1), (0, 1, 2)):
        arr = (_lib.rrl_eval_rollout_qs_t * len(kinds))(*[_desc(kind) for kind in kinds])
        assert lib.rrl_eval_rollout_qs_packed(len(kinds), arr, None) == EINVAL, kinds
    arr = (_lib.rrl_eval_rollout_qs_t * 2)(_desc(0, k=0), _desc(2))
    assert lib.rrl_eval_rollout_qs_packed(2, arr, None) == EINVAL


# ---- the path table ----------------------------------------------------------------------------------------------------
LINES = {"none": [], "MF": ["--use_recovery", "--MF_recovery"], "QS": ["--use_recovery", "--Q_sampling_recovery"],
         "QS+MF": ["--use_recovery", "--Q_sampling_recovery", "--MF_recovery"],
         "QS+SQRL": ["--use_recovery", "--Q_sampling_recovery", "--use_constraint_sampling"], "MB": ["--use_recovery"]}
SWITCHES = ("RRL_FAST_EVAL", "RRL_FAST_EVAL_MAZE", "RRL_FAST_EVAL_QSAMPLE")


def _cfg(line, env, hidden, num_envs):
    return arg_utils.get_args(["--env-name", env, "--gamma_safe", "0.8", "--eps_safe", "0.3", "--hidden_size", str(hidden),
                               "--num_envs", str(num_envs)] + LINES[line])


def _path(monkeypatch, switches, cfg):
    for name, on in zip(SWITCHES, switches):
        if on:
            monkeypatch.setenv(name, "1")
        else:
            monkeypatch.delenv(name, raising=False)
    return fast_update.eval_rollout_path(cfg)


@pytest.mark.parametrize("env", ["navigation1", "navigation2", "maze"])
@pytest.mark.parametrize("line", list(LINES))
def test_path_table(monkeypatch, line, env):
    monkeypatch.setenv("RRL_FAST_BASELINES", "1")           # (so that --use_constraint_sampling alone would keep the fused path)
    monkeypatch.delenv("RRL_FAST_QSAMPLE", raising=False)   # the evaluation kernel does not depend on the acting switch
    for hidden, num_envs in itertools.product((256, 64), (1, 4)):
        cfg = _cfg(line, env, hidden, num_envs)
        for switches in itertools.product((False, True), repeat=3):
            fast, maze, qs = switches
            got = _path(monkeypatch, switches, cfg)
            base = fast and hidden == 256 and num_envs > 1 and (env != "maze" or maze)
            want = base and (line in ("none", "MF", "QS+MF") or (line == "QS" and qs))
            assert got == ("hip" if want else "modules"), (line, env, hidden, num_envs, switches)
            # with the new switch unset: exactly what it is today -- and the new switch changes the Q-sampling line alone
            if qs and line != "QS":
                assert got == _path(monkeypatch, (fast, maze, False), cfg)
            if not qs and line == "QS":
                assert got == "modules"
    assert fast_update.fast_eval_qsample_enabled() == (os.environ.get("RRL_FAST_EVAL_QSAMPLE") == "1")
    monkeypatch.setenv("RRL_FAST_QSAMPLE", "1")
    assert _path(monkeypatch, (True, True, True), _cfg("QS", env, 256, 4)) == "hip"
    assert _path(monkeypatch, (True, True, False), _cfg("QS", env, 256, 4)) == "modules"


# ---- the candidates ----------------------------------------------------------------------------------------------------
def test_candidates_fill_the_box_and_are_a_stream_of_their_own():
    for box in ("unit", "asym", "maze"):
        lo, hi = (np.asarray(b, np.float32) for b in BOXES[box])
        c = np.concatenate([QC.candidates_row(row, 1000, box, QC.TICK) for row in range(20)])
        assert c.dtype == np.float32 and (c >= lo).all() and (c <= hi).all()
        span = (hi - lo).astype(np.float64)
        assert (np.abs(c.mean(0) - (lo + hi) / 2) < 0.01 * span).all()                  # 20 000 draws: sd = 0.002 span
        assert (c.min(0) < lo + 0.001 * span).all() and (c.max(0) > hi - 0.001 * span).all()
    u13 = QC.uniforms_row(3, 64, QC.STREAM_EVAL_QSAMPLE, QC.SEED, QC.TICK)
    u11 = QC.uniforms_row(3, 64, STREAM_QSAMPLE, QC.SEED, QC.TICK)
    assert 0.0 < u13.min() and u13.max() < 1.0 and len(np.unique(u13)) == u13.size
    assert not np.isin(u13, u11).any()                                                  # the same key on stream 11: other draws
    assert not np.array_equal(u13, QC.uniforms_row(3, 64, QC.STREAM_EVAL_QSAMPLE, QC.SEED, QC.TICK + 1))
    assert not np.array_equal(u13, QC.uniforms_row(4, 64, QC.STREAM_EVAL_QSAMPLE, QC.SEED, QC.TICK))


# ---- fairness of the cases ---------------------------------------------------------------------------------------------
def test_the_case_table_is_the_issues():
    nav = QC.nav_cases()
    assert len(nav) == len(set(nav)) == 48 * 2 * 2 * 2
    assert {(n, T, k) for _, n, T, k, _, _ in nav} == \
        {(n, T, k) for n in (1, 17, 65) for T in (1, 2, 7) for k in (1, 17, 64, 65, 130)} | {(17, 2, 1000), (3, 1, 1024), (65, 101, 17)}
    assert {box for *_, box in nav} == {"unit", "asym"} and {r for *_, r, _ in nav} == {0, 1}
    maze = QC.maze_cases()
    assert {h for _, _, _, h, _ in maze} == {100, 3} and {r for *_, r in maze} == {0, 1}
    assert {(n, T, k) for n, T, k, _, _ in maze} <= {(n, T, k) for _, n, T, k, _, _ in nav}


def _tiles(mask):
    """[T, n] -> [T, tiles]: how many rows of each 16-row tile are set"""
    T, n = mask.shape
    pad = np.zeros((T, -n % 16), bool)
    return np.concatenate([mask, pad], 1).reshape(T, -1, 16).sum(2)


def _fair(r, n, T, reset, navigation):
    assert r["alive"][0].all()
    if n < 17 or T < 2:
        return
    live = r["alive"]
    # the gate is mixed: (row, step) pairs gated and live pairs not gated, at least a quarter of the rows each on step 0
    assert r["gate"].any() and (live & ~r["gate"]).any()
    assert n // 4 <= r["gate"][0].sum() <= n - n // 4
    # the executed action of a gated pair is its pick among the candidates, inside the box; no pick elsewhere
    assert ((r["pick"] >= 0) == r["gate"]).all()
    # some tile serves two or more gated rows in one step (the ascending-row loop) ...
    assert (_tiles(r["gate"]) >= 2).any()
    if reset == 0:
        # ... rows end by constraint, by success, and survive (start_states places every fate in every four rows; after a
        # reset every Navigation row starts 46 steps from the goal, so success is out of reach there -- eval_cases)
        assert r["constraint"].any() and r["success"].any()
        assert r["survived"].any() or not navigation


@pytest.mark.parametrize("kind,n,T,k,reset,box", QC.nav_cases())
def test_navigation_cases_are_fair(kind, n, T, k, reset, box):
    _fair(QC.rollout64(kind, n, T, k, reset, box), n, T, reset, True)


@pytest.mark.parametrize("n,T,k,horizon,reset", QC.maze_cases())
def test_maze_cases_are_fair(n, T, k, horizon, reset):
    _fair(QC.rollout64("maze", n, T, k, reset, "maze", horizon), n, T, reset, False)


def test_some_tile_has_no_gated_row_in_a_step():
    """Over the table: a step in which a tile with live rows has no gated one (the whole candidate phase is skipped), in the
    several-tile cases of both families."""
    hits = 0
    for kind, n, T, k, reset, box in QC.nav_cases():
        if n == 65 and T >= 2 and k == 17 and box == "unit":
            r = QC.rollout64(kind, n, T, k, reset, box)
            hits += int(((_tiles(r["gate"]) == 0) & (_tiles(r["alive"]) > 0)).any())
    assert hits >= 1
