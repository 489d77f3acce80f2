"""SQRL on the evaluation rollout kernel (rrl_eval_rollout_sqrl[_packed]), the parts that need no GPU: the ABI is declared,
exported and additive; every descriptor check returns its code before any launch; the path table of eval_rollout_path over
the four switches; the fairness of the cases of eval_sqrl_cases.py, from the float64 rollout with the regenerated draws of
streams 14 / 15, which tests/test_eval_sqrl_gpu.py measures the kernels on; and the agreement of that restatement with
SAC._sqrl_action on CPU modules."""
import ctypes as C
import itertools
import os
import re

import numpy as np
import pytest
import torch

import arg_utils
import eval_sqrl_cases as SC
from oracle import c_oracle as co
from recovery_rl_amd import _lib, fast_update
from test_sqrl_act_cpu import STREAM_SQRL, STREAM_SQRL_PICK, left_out_cap

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, ERANGE = -1, -3
REQUIRED = ("pW1", "pb1", "pW2p", "pb2", "pW3", "pb3", "scale", "bias", "ret", "success", "violation", "steps")
QGROUP = ("qW1", "qb1", "qW2p", "qb2", "qW3", "qb3")
RGROUP = ("rW1", "rb1", "rW2p", "rb2", "rW3", "rb3", "rscale", "rbias", "rlog_std")
OWN_TRACES = ("tr_head", "tr_pick", "tr_cstar", "tr_nsafe", "tr_q")


# ---- ABI ---------------------------------------------------------------------------------------------------------------
def test_symbols_are_declared_exported_and_additive():
    src = open(os.path.join(ROOT, "include", "rrl_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"\bint\s+rrl_eval_rollout_sqrl\s*\(\s*const\s+rrl_eval_rollout_sqrl_t\s*\*\s*\w*\s*,\s*void\s*\*", code)
    assert re.search(r"\bint\s+rrl_eval_rollout_sqrl_packed\s*\(\s*int\s+\w+\s*,\s*const\s+rrl_eval_rollout_sqrl_t\s*\*", code)
    assert re.search(r"RRL_STREAM_EVAL_SQRL\s*=\s*14\b", code) and re.search(r"RRL_STREAM_EVAL_SQRL_PICK\s*=\s*15\b", code)
    for name in ("rrl_eval_rollout_sqrl", "rrl_eval_rollout_sqrl_packed"):
        assert name in _lib.EXPORTS
        assert name in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert (_lib.STREAM_EVAL_SQRL, _lib.STREAM_EVAL_SQRL_PICK) == (SC.STREAM_EVAL_SQRL, SC.STREAM_EVAL_SQRL_PICK) == (14, 15)
    lib = _lib.load()
    assert lib.rrl_abi_version() == 8                       # additive: nothing existing changed layout
    assert lib.rrl_eval_rollout_sqrl.argtypes[0] == C.POINTER(_lib.rrl_eval_rollout_sqrl_t)
    assert lib.rrl_eval_rollout_sqrl_packed.argtypes[1] == C.POINTER(_lib.rrl_eval_rollout_sqrl_t)


def test_struct_layout_follows_the_header_and_the_base_is_unchanged():
    src = open(os.path.join(ROOT, "include", "rrl_hip.h")).read()
    body = re.search(r"typedef struct \{((?:(?!typedef).)*?)\} rrl_eval_rollout_sqrl_t;", src, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    want = []
    ctypes_of = {"int": C.c_int, "rrl_eval_rollout_t": _lib.rrl_eval_rollout_t}
    for decl in filter(None, (d.strip() for d in body.split(";"))):
        base, rest = re.match(r"(?:const\s+)?(\w+\s*\*?)\s*(.*)", decl, flags=re.S).groups()
        for name in rest.split(","):
            name = name.strip()
            want.append((name.lstrip("* "), C.c_void_p if name.startswith("*") or base.endswith("*") else ctypes_of[base.strip()]))
    assert [(n, t) for n, t in _lib.rrl_eval_rollout_sqrl_t._fields_] == want
    assert [n for n, _ in want] == ["base", "k", "horizon"] + list(OWN_TRACES)
    assert C.sizeof(_lib.rrl_eval_rollout_t) == 352 and len(_lib.rrl_eval_rollout_t._fields_) == 47
    assert _lib.rrl_eval_rollout_sqrl_t.base.offset == 0 and _lib.rrl_eval_rollout_sqrl_t.k.offset == 352
    assert C.sizeof(_lib.rrl_eval_rollout_sqrl_t) == 352 + 8 + 5 * 8


def _desc(kind=0, **fields):
    """A well-formed rrl_eval_rollout_sqrl_t whose device pointers are dummy non-null integers (validation never follows
    them).  Fields of the base descriptor and of the SQRL struct are told apart by name."""
    d = 0x1000
    base = _lib.rrl_eval_rollout_t(n=8, T=101, H=256, d_obs=2, d_act=2, env_kind=kind, reset=1, eps_safe=0.3,
                                   **{k: d for k in REQUIRED + QGROUP})
    own = dict(k=100, horizon=100 if kind == 2 else 0)
    for k, v in fields.items():
        if k in own or k in OWN_TRACES:
            own[k] = v
        else:
            setattr(base, k, v)
    return _lib.rrl_eval_rollout_sqrl_t(base=base, **own)


def _solo(lib, a):
    return lib.rrl_eval_rollout_sqrl(C.byref(a), None)


def _packed(lib, a, S=2):
    """the descriptor under test as the LAST of S seeds, behind well-formed ones of its env family"""
    arr = (_lib.rrl_eval_rollout_sqrl_t * S)(*([_desc(a.base.env_kind if a.base.env_kind == 2 else 0)] * (S - 1) + [a]))
    return lib.rrl_eval_rollout_sqrl_packed(S, arr, None)


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
    # ---- its own: a Q_risk group that is missing (in part or whole), any pointer of the recovery group ----
    for name in QGROUP:
        assert call(lib, _desc(kind, **{name: None})) == EINVAL, name
    assert call(lib, _desc(kind, **{name: None for name in QGROUP})) == EINVAL
    for name in RGROUP:
        assert call(lib, _desc(kind, **{name: 0x1000})) == EINVAL, name
    assert call(lib, _desc(kind, **{name: 0x1000 for name in RGROUP})) == EINVAL
    for fields in (dict(k=0), dict(k=-1), dict(k=129), dict(k=1000)):
        assert call(lib, _desc(kind, **fields)) == ERANGE, fields
    # (n k >= 2^32 cannot be reached with n <= 2^22 and k <= 128: each of the two bounds fires first)
    assert call(lib, _desc(kind, n=2 ** 22 + 1, k=128)) == ERANGE
    if kind == 2:       # (Navigation ignores the horizon: every Navigation launch of the GPU tests passes 0)
        for horizon in (0, -1, 2 ** 30 + 1):
            assert call(lib, _desc(kind, horizon=horizon)) == ERANGE, horizon
    # ---- an invalid field wins over a size out of range, whatever the order of the struct ----
    assert call(lib, _desc(kind, k=5000, H=32)) == EINVAL
    assert call(lib, _desc(kind, k=0, qW1=None)) == EINVAL
    assert call(lib, _desc(kind, T=5000, rW1=0x1000)) == EINVAL
    assert call(lib, _desc(kind, n=2 ** 22 + 1, steps=None)) == EINVAL
    assert call(lib, _desc(kind, horizon=-5, k=0, qb3=None)) == EINVAL


def test_entries_check_their_own_arguments():
    lib = _lib.load()
    assert lib.rrl_eval_rollout_sqrl(None, None) == EINVAL
    one = (_lib.rrl_eval_rollout_sqrl_t * 17)(*[_desc()] * 17)
    assert lib.rrl_eval_rollout_sqrl_packed(2, None, None) == EINVAL
    for S in (0, -1, 17):
        assert lib.rrl_eval_rollout_sqrl_packed(S, one, None) == ERANGE, S
    # every seed is checked, and an invalid field of a later seed wins over a size out of range of an earlier one
    arr = (_lib.rrl_eval_rollout_sqrl_t * 3)(_desc(k=0), _desc(), _desc(qW1=None))
    assert lib.rrl_eval_rollout_sqrl_packed(3, arr, None) == EINVAL
    arr = (_lib.rrl_eval_rollout_sqrl_t * 3)(_desc(), _desc(1, k=129), _desc())
    assert lib.rrl_eval_rollout_sqrl_packed(3, arr, None) == ERANGE
    # Navigation 1 and 2 go together; Navigation and Maze do not, and that wins over a size out of range too
    for kinds in ((0, 2), (2, 1), (0, 1, 2)):
        arr = (_lib.rrl_eval_rollout_sqrl_t * len(kinds))(*[_desc(kind) for kind in kinds])
        assert lib.rrl_eval_rollout_sqrl_packed(len(kinds), arr, None) == EINVAL, kinds
    arr = (_lib.rrl_eval_rollout_sqrl_t * 2)(_desc(0, k=0), _desc(2))
    assert lib.rrl_eval_rollout_sqrl_packed(2, arr, None) == EINVAL


# ---- the path table ----------------------------------------------------------------------------------------------------
LINES = {"none": [], "MF": ["--use_recovery", "--MF_recovery"], "QS": ["--use_recovery", "--Q_sampling_recovery"],
         "SQRL": ["--use_constraint_sampling"], "SQRL+MF": ["--use_constraint_sampling", "--use_recovery", "--MF_recovery"],
         "MB": ["--use_recovery"]}
SWITCHES = ("RRL_FAST_EVAL", "RRL_FAST_EVAL_MAZE", "RRL_FAST_EVAL_QSAMPLE", "RRL_FAST_EVAL_SQRL")


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
    monkeypatch.setenv("RRL_FAST_BASELINES", "1")           # (so that --use_constraint_sampling keeps the fused path)
    monkeypatch.delenv("RRL_FAST_SQRL", raising=False)      # the evaluation kernel does not depend on the acting switch
    for hidden, num_envs in itertools.product((256, 64), (1, 4)):
        cfg = _cfg(line, env, hidden, num_envs)
        for switches in itertools.product((False, True), repeat=4):
            fast, maze, qs, sq = switches
            got = _path(monkeypatch, switches, cfg)
            base = fast and hidden == 256 and num_envs > 1 and (env != "maze" or maze)
            parent = base and (line in ("none", "MF") or (line == "QS" and qs))          # eval_rollout_path before this switch
            want = parent or (base and line == "SQRL" and sq)
            assert got == ("hip" if want else "modules"), (line, env, hidden, num_envs, switches)
            if not sq:
                assert got == ("hip" if parent else "modules")
            elif line != "SQRL":                            # the switch moves the SQRL line alone
                assert got == _path(monkeypatch, (fast, maze, qs, False), cfg)
    assert fast_update.fast_eval_sqrl_enabled() == (os.environ.get("RRL_FAST_EVAL_SQRL") == "1")
    for acting in ("1", "0"):
        monkeypatch.setenv("RRL_FAST_SQRL", acting)
        assert _path(monkeypatch, (True, True, False, True), _cfg("SQRL", env, 256, 4)) == "hip"
        assert _path(monkeypatch, (True, True, True, False), _cfg("SQRL", env, 256, 4)) == "modules"
    monkeypatch.delenv("RRL_FAST_BASELINES", raising=False)  # without the fused update path there is no fast agent to read
    assert _path(monkeypatch, (True, True, True, True), _cfg("SQRL", env, 256, 4)) == "modules"


# ---- the draws ---------------------------------------------------------------------------------------------------------
def test_draws_are_streams_of_their_own():
    t = SC.TICK
    e14 = SC.noise(5, 16, t)
    assert e14.dtype == np.float32 and e14.shape == (5, 16, 2)
    for r in (0, 17, 79):                                    # normals() is normal2() row by row: row = env row * k + c
        assert e14.reshape(-1, 2)[r].tobytes() == np.asarray(co.normal2(SC.SEED, r, SC.STREAM_EVAL_SQRL, t), np.float32).tobytes()
    e9 = co.normals(SC.SEED, 80, STREAM_SQRL, t).astype(np.float32)
    assert not np.isin(e14.reshape(-1), e9.reshape(-1)).any()                           # the same key on stream 9: other draws
    assert not np.array_equal(e14, SC.noise(5, 16, t + 1))
    u15, u10 = SC.uniforms(64, t), SC.uniforms(64, t, SC.SEED, STREAM_SQRL_PICK)
    assert 0.0 < u15.min() and u15.max() < 1.0 and len(np.unique(u15)) == 64
    assert not np.isin(u15, u10).any()
    assert not np.array_equal(u15, SC.uniforms(64, t + 1))
    # keyed by the env row alone: the draws of rows 0 .. 15 do not depend on n
    assert np.array_equal(SC.noise(65, 100, t)[:16], SC.noise(16, 100, t)) and np.array_equal(SC.uniforms(65, t)[:16], SC.uniforms(16, t))


# ---- fairness of the cases ---------------------------------------------------------------------------------------------
def test_the_case_table_is_the_issues():
    nav = SC.nav_cases()
    mixed = [c for c in nav if c[5] == "mixed"]
    assert len(nav) == len(set(nav)) and len(mixed) == 64 * 2 * 2
    assert {(n, T, k) for _, n, T, k, _, _ in mixed} == \
        {(n, T, k) for n in (1, 17, 65) for T in (1, 2, 7) for k in (1, 16, 17, 64, 65, 100, 128)} | {(65, 101, 17)}
    assert {r for *_, r, _ in mixed} == {0, 1}
    for kind in ("navigation1", "navigation2"):             # two more per kind: nothing safe, everything safe
        assert sorted(c[5] for c in nav if c[0] == kind and c[5] != "mixed") == ["all_safe", "none_safe"]
    assert SC.eps_safe("navigation1", 17, 2, 100, 0, "none_safe") == 0.0 and SC.eps_safe("navigation1", 65, 7, 17, 1, "all_safe") == 1.0
    maze = SC.maze_cases()
    assert {h for _, _, _, h, _, _ in maze} == {100, 3} and {r for *_, r, _ in maze} == {0, 1}
    assert {m for *_, m in maze} == set(SC.MODES)
    # the two changes to the agents, and nothing else: stacked head rows, action columns of Q_risk's first layers x 10
    for kind in ("navigation1", "navigation2", "maze"):
        w, w0 = SC.weights32(kind), (SC.MC.weights32() if kind == "maze" else SC.EC.weights32(kind))
        assert w["pW3"].shape == (4, 256) and np.array_equal(w["pW3"][:2], w0["pW3"]) and np.array_equal(w["pb3"][:2], w0["pb3"])
        assert np.array_equal(w["qW1"][:, :, :2], w0["qW1"][:, :, :2])
        assert np.array_equal(w["qW1"][:, :, 2:], (w0["qW1"][:, :, 2:] * np.float32(10)).astype(np.float32))
        assert all(np.array_equal(w[name], w0[name]) for name in w0 if name not in ("pW3", "pb3", "qW1"))


def _fair(r, n, T, k, mode):
    live = r["alive"]
    assert live[0].all()
    # the condition the threshold rule has to meet: at most 2 % of the live (row, step) pairs are ambiguous (left_out_cap)
    amb, pairs = int((r["ambiguous"] & live).sum()), int(live.sum())
    assert amb <= left_out_cap(pairs) and SC.ambiguous_share_ok(r), (amb, pairs)
    ns = r["n_safe"][live]
    if mode == "none_safe":
        assert (ns == 0).all() and (r["cstar"][live] == -1).all()
    elif mode == "all_safe":
        assert (ns == k).all() and (r["cstar"][live] == r["pick"][live]).all()
    assert ((r["pick"][live] >= 0) & (r["pick"][live] < k)).all()
    return r["constraint"].any(), r["success"].any(), r["survived"].any()


@pytest.mark.parametrize("kind,n,T,k,reset,mode", SC.nav_cases())
def test_navigation_cases_are_fair(kind, n, T, k, reset, mode):
    r = SC.rollout64(kind, n, T, k, reset, mode)
    ends = _fair(r, n, T, k, mode)
    if n >= 17 and reset == 0:
        # rows end by constraint, by success, and survive (start_states places every fate in every four rows; after a reset
        # every Navigation row starts 46 steps from the goal, so success is out of reach there -- eval_cases)
        assert all(ends), ends
    if (kind, n, k, reset, mode) == ("navigation1", 65, 100, 0, "mixed"):
        ns = r["n_safe"][0]
        counts = [int((ns == 0).sum()), int(((ns > 0) & (ns < k)).sum()), int((ns == k).sum())]
        assert min(counts) >= 8, counts                      # each of the three branches of the pick, on step 0


@pytest.mark.parametrize("n,T,k,horizon,reset,mode", SC.maze_cases())
def test_maze_cases_are_fair(n, T, k, horizon, reset, mode):
    r = SC.rollout64("maze", n, T, k, reset, mode, horizon)
    cons, succ, surv = _fair(r, n, T, k, mode)
    if n >= 17 and reset == 0 and mode == "mixed":
        assert cons and succ
        assert surv == (horizon > T)                         # the horizon of 3 ends every row before T = 7


def test_rows_end_every_way_over_the_cases_with_several_rows():
    ends = np.zeros(3, bool)
    for kind, n, T, k, reset, mode in SC.nav_cases():
        if n >= 17:
            r = SC.rollout64(kind, n, T, k, reset, mode)
            now = np.array([r["constraint"].any(), r["success"].any(), r["survived"].any()])
            assert now.any()
            ends |= now
    assert ends.all()


def test_some_step_has_dead_and_live_rows_in_one_tile_and_a_tile_with_none():
    """What the flattening has to get right: tiles whose live rows are a strict subset (the s-th live row is not row s), and a
    tile that has left the step loop while others go on."""
    partial = gone = False
    for kind, n, T, k, reset, mode in SC.nav_cases():
        if n == 65 and T == 7 and reset == 0 and mode == "mixed":
            a = SC.rollout64(kind, n, T, k, reset, mode)["alive"]
            tiles = np.concatenate([a, np.zeros((T, 15), bool)], 1).reshape(T, 5, 16).sum(2)
            partial |= bool(((tiles > 0) & (tiles < 16))[:, :4].any())
            gone |= bool(((tiles == 0).any(1) & (tiles > 0).any(1)).any())
    assert partial and gone


# ---- the restatement against the modules --------------------------------------------------------------------------------
def _modules_agree(kind, r, n, T, k, eps_s):
    ag = SC.agent(kind)
    ag.eps_safe = eps_s
    for j in range(T):
        live = r["alive"][j]
        keep = live & ~r["ambiguous"][j]
        if not keep.any():
            continue
        # `draw` is the position in the safe list; where nothing is safe the modules take their own argmin
        draw = np.where(r["n_safe"][j] > 0, r["pick"][j], 0)
        got = ag._sqrl_action(torch.tensor(r["obs"][j]), safe_samples=k,
                              eps=torch.tensor(SC.noise(n, k, SC.TICK + int(r["reset"]) + j)), draw=draw).numpy()
        want = r["real64"][j]
        assert np.allclose(got[keep], want[keep], rtol=1e-5, atol=1e-6), (j, np.abs(got - want)[keep].max())


@pytest.mark.parametrize("kind,n,T,k,reset,mode", SC.nav_cases())
def test_restatement_reproduces_sqrl_action_on_cpu_modules(kind, n, T, k, reset, mode):
    r = dict(SC.rollout64(kind, n, T, k, reset, mode), reset=reset)
    _modules_agree(kind, r, n, T, k, SC.eps_safe(kind, n, T, k, reset, mode))


@pytest.mark.parametrize("n,T,k,horizon,reset,mode", SC.maze_cases())
def test_restatement_reproduces_sqrl_action_on_cpu_modules_maze(n, T, k, horizon, reset, mode):
    r = dict(SC.rollout64("maze", n, T, k, reset, mode, horizon), reset=reset)
    _modules_agree("maze", r, n, T, k, SC.eps_safe("maze", n, T, k, reset, mode, horizon))
