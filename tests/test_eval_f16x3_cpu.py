"""f16x3 candidate scoring on the evaluation rollout kernels (rrl_eval_rollout_qs_f16x3 / rrl_eval_rollout_sqrl_f16x3 and their
packed forms), the parts that need no GPU: the ABI is declared, exported and additive; every malformed descriptor of
test_eval_qsample_cpu.py / test_eval_sqrl_cpu.py gets the f32 entry's code, and the stream beside the descriptor is checked as
an invalid field; eval_scoring over the path tables of those two files; the LDS carve-ups parsed out of the sources."""
import ctypes as C
import itertools
import os
import re

import pytest

import test_eval_qsample_cpu as TQC
import test_eval_sqrl_cpu as TSC
from recovery_rl_amd import _lib, fast_update

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, ERANGE = -1, -3
W2H = 0x2000                                  # a well-formed stream pointer (validation never follows it)
LINES = {"qs": (TQC, _lib.rrl_eval_rollout_qs_t, "rrl_eval_rollout_qs"),
         "sqrl": (TSC, _lib.rrl_eval_rollout_sqrl_t, "rrl_eval_rollout_sqrl")}


# ---- ABI ---------------------------------------------------------------------------------------------------------------
def test_symbols_are_declared_exported_and_additive():
    src = open(os.path.join(ROOT, "include", "rrl_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    lib = _lib.load()
    vp = C.c_void_p
    for line, (_, T, f32) in LINES.items():
        solo, packed = f32 + "_f16x3", f32 + "_f16x3_packed"
        t = T.__name__
        assert re.search(r"\bint\s+%s\s*\(\s*const\s+%s\s*\*\s*\w+\s*,\s*const\s+float\s*\*\s*\w+\s*,\s*void\s*\*\s*\w+\s*\)\s*;"
                         % (solo, t), code), solo
        assert re.search(r"\bint\s+%s\s*\(\s*int\s+\w+\s*,\s*const\s+%s\s*\*\s*\w+\s*,\s*const\s+float\s*\*\s*const\s*\*\s*\w+\s*,"
                         r"\s*void\s*\*\s*\w+\s*\)\s*;" % (packed, t), code), packed
        for name in (solo, packed):
            assert name in _lib.EXPORTS and name in integration, name
        assert getattr(lib, solo).argtypes == [C.POINTER(T), vp, vp]
        assert getattr(lib, packed).argtypes == [C.c_int, C.POINTER(T), C.POINTER(vp), vp]
    assert lib.rrl_abi_version() == 8                       # additive: nothing existing changed layout
    assert C.sizeof(_lib.rrl_eval_rollout_qs_t) == 352 + 8 + 4 * 8
    assert C.sizeof(_lib.rrl_eval_rollout_sqrl_t) == 352 + 8 + 5 * 8


# ---- descriptor validation -----------------------------------------------------------------------------------------------
def _streams(S, last=W2H):
    return (C.c_void_p * S)(*([W2H] * (S - 1) + [last]))


def _both(line, packed):
    """call(lib, a) of the existing validation tests: the f32 entry's code, after asserting that the f16x3 entry with a
    well-formed stream gives the same one (solo, or as the last of S = 2 behind a well-formed seed of its env family)"""
    mod, T, f32 = LINES[line]

    def call(lib, a):
        if not packed:
            want = getattr(lib, f32)(C.byref(a), None)
            got = getattr(lib, f32 + "_f16x3")(C.byref(a), W2H, None)
        else:
            arr = (T * 2)(mod._desc(a.base.env_kind if a.base.env_kind == 2 else 0), a)
            want = getattr(lib, f32 + "_packed")(2, arr, None)
            got = getattr(lib, f32 + "_f16x3_packed")(2, arr, _streams(2), None)
        assert got == want, (line, packed, got, want)
        return got
    return call


@pytest.mark.parametrize("packed", [False, True])
@pytest.mark.parametrize("kind", [0, 1, 2])
@pytest.mark.parametrize("line", list(LINES))
def test_malformed_descriptors_get_the_f32_entrys_code(line, kind, packed):
    """Every malformed descriptor the two existing files build (NULL required pointers, H, d_obs, d_act, n, T, k, the Maze
    horizon, a recovery group given, a missing Q_risk group): their own assertions, on a call that compares the two entries"""
    LINES[line][0].test_descriptor_validation_without_gpu(_both(line, packed), kind)


@pytest.mark.parametrize("kind", [0, 1, 2])
@pytest.mark.parametrize("line", list(LINES))
def test_the_stream_is_an_invalid_field(line, kind):
    mod, T, f32 = LINES[line]
    lib = _lib.load()
    solo, packed = getattr(lib, f32 + "_f16x3"), getattr(lib, f32 + "_f16x3_packed")
    good = mod._desc(kind)
    for bad in (None, W2H + 4, W2H + 8):
        assert solo(C.byref(good), bad, None) == EINVAL, bad
        assert solo(C.byref(mod._desc(kind, k=5000)), bad, None) == EINVAL, bad          # ... and wins over an out-of-range k
        assert solo(C.byref(mod._desc(kind, T=0)), bad, None) == EINVAL, bad
        arr = (T * 2)(mod._desc(kind), mod._desc(kind))
        assert packed(2, arr, _streams(2, bad), None) == EINVAL, bad
        arr = (T * 2)(mod._desc(kind, k=5000), mod._desc(kind))
        assert packed(2, arr, _streams(2, bad), None) == EINVAL, bad
    assert solo(C.byref(mod._desc(kind, k=5000)), W2H, None) == ERANGE
    assert solo(None, W2H, None) == EINVAL
    arr = (T * 2)(mod._desc(kind), mod._desc(kind))
    assert packed(2, arr, None, None) == EINVAL and packed(2, None, _streams(2), None) == EINVAL


@pytest.mark.parametrize("line", list(LINES))
def test_packed_entries_check_their_own_arguments(line):
    mod, T, f32 = LINES[line]
    packed = getattr(_lib.load(), f32 + "_f16x3_packed")
    one = (T * 17)(*[mod._desc()] * 17)
    for S in (0, -1, 17):
        assert packed(S, one, _streams(17), None) == ERANGE, S
    # Navigation 1 and 2 go together; Navigation and Maze do not, and that wins over a size out of range
    for kinds in ((0, 2), (2, 1), (0, 1, 2)):
        arr = (T * len(kinds))(*[mod._desc(kind) for kind in kinds])
        assert packed(len(kinds), arr, _streams(len(kinds)), None) == EINVAL, kinds
    arr = (T * 2)(mod._desc(0, k=0), mod._desc(2))
    assert packed(2, arr, _streams(2), None) == EINVAL
    # an invalid field of a later seed wins over a size out of range of an earlier one
    arr = (T * 3)(mod._desc(k=0), mod._desc(), mod._desc(qW1=None))
    assert packed(3, arr, _streams(3), None) == EINVAL
    arr = (T * 3)(mod._desc(), mod._desc(1, k=5000), mod._desc())
    assert packed(3, arr, _streams(3), None) == ERANGE


# ---- the path table ----------------------------------------------------------------------------------------------------
ALL_LINES = dict(TQC.LINES, **TSC.LINES)
OLD = ("RRL_FAST_EVAL", "RRL_FAST_EVAL_MAZE", "RRL_FAST_EVAL_QSAMPLE", "RRL_FAST_EVAL_SQRL")
NEW = ("RRL_EVAL_QSAMPLE_F16X3", "RRL_EVAL_SQRL_F16X3")


def _set(monkeypatch, names, values):
    for name, on in zip(names, values):
        if on:
            monkeypatch.setenv(name, "1")
        else:
            monkeypatch.delenv(name, raising=False)


@pytest.mark.parametrize("env", ["navigation1", "navigation2", "maze"])
@pytest.mark.parametrize("line", list(ALL_LINES))
def test_path_table(monkeypatch, line, env):
    """eval_scoring is "f16x3" only with all three switches of the line set and eval_rollout_path == "hip"; eval_rollout_path
    returns what it returned without the new switches, for every row; the acting switches do not enter."""
    monkeypatch.setenv("RRL_FAST_BASELINES", "1")
    for name in ("RRL_FAST_SQRL", "RRL_FAST_QSAMPLE", "RRL_SQRL_F16X3", "RRL_QSAMPLE_F16X3"):
        monkeypatch.delenv(name, raising=False)
    for hidden, num_envs in itertools.product((256, 64), (1, 4)):
        cfg = TSC._cfg(line, env, hidden, num_envs) if line in TSC.LINES else TQC._cfg(line, env, hidden, num_envs)
        for old in itertools.product((False, True), repeat=4):
            _set(monkeypatch, OLD, old)
            _set(monkeypatch, NEW, (False, False))
            before = fast_update.eval_rollout_path(cfg)
            assert fast_update.eval_scoring(cfg) == "f32"
            fast, maze, qs, sq = old
            for new in itertools.product((False, True), repeat=2):
                _set(monkeypatch, NEW, new)
                assert fast_update.eval_rollout_path(cfg) == before, (line, env, old, new)
                want = before == "hip" and ((line == "QS" and fast and qs and new[0]) or (line == "SQRL" and fast and sq and new[1]))
                assert fast_update.eval_scoring(cfg) == ("f16x3" if want else "f32"), (line, env, hidden, num_envs, old, new)
    # independent of the acting switches, either way
    _set(monkeypatch, OLD, (True,) * 4)
    _set(monkeypatch, NEW, (True, True))
    cfg = TSC._cfg("SQRL", env, 256, 4)
    for acting in ("0", "1"):
        monkeypatch.setenv("RRL_SQRL_F16X3", acting)
        monkeypatch.setenv("RRL_QSAMPLE_F16X3", acting)
        assert fast_update.eval_scoring(cfg) == "f16x3" and fast_update.eval_scoring(TQC._cfg("QS", env, 256, 4)) == "f16x3"
    _set(monkeypatch, NEW, (False, False))
    assert fast_update.eval_scoring(cfg) == "f32" and fast_update.eval_scoring(TQC._cfg("QS", env, 256, 4)) == "f32"


# ---- LDS and constants -------------------------------------------------------------------------------------------------
def _constants(text, scope=None):
    """{name: expression} of the `constexpr int name = expr;` declarations of a source (of `struct scope { .. }` when given)"""
    if scope:
        text = re.search(r"struct %s \{(.*?)\n\};" % scope, text, flags=re.S).group(1)
    text = re.sub(r"//[^\n]*", "", text)
    out = {}
    for decl in re.findall(r"constexpr int ([^;]+);", text):
        for part in decl.split(","):
            name, expr = part.split("=")
            out[name.strip()] = expr.strip()
    return out


def _value(name, *tables, env=None):
    env = dict(env or {})
    for t in tables:
        if name in t:
            expr = re.sub(r"\b(?:rrl_tile::|Tile::)", "", t[name])
            names = set(re.findall(r"[A-Za-z_]\w*", expr))
            scope = {n: _value(n, *tables, env=env) for n in names if n not in env}
            return int(eval(expr, {}, dict(env, **scope)))          # integer arithmetic on the names resolved above
    raise KeyError(name)


def test_lds_of_the_new_carve_ups():
    src = lambda f: open(os.path.join(_lib.CSRC, f)).read()
    tile, f16, ev = _constants(src("mfma_tile.hpp")), src("mfma_tile_f16x3.hpp"), src("eval_kernels.hip")
    f16_ns = _constants(re.sub(r"struct TileF16x3 \{.*", "", f16, flags=re.S))
    f16_tile = _constants(f16, "TileF16x3")
    roll = _constants(re.sub(r"\nstruct \w+[^\n]*\{.*?\n\};", "", ev, flags=re.S))      # the file's own, outside any struct
    # the f16x3 tile's prefix: the names the carve-ups see as Tile::
    T16 = {n: _value(n, f16_tile, f16_ns, tile) for n in ("kOffAct", "kOffXs", "kOffQpart", "kOffOwn")}
    assert T16["kOffXs"] * 4 == 67584 and T16["kOffOwn"] == T16["kOffXs"] + 64 * 4 + 2 * 8 * 64
    T32 = {n: _value(n, tile) for n in ("kOffXs", "kOffOwn")}
    assert T32["kOffXs"] * 4 == 66560
    sizes = {}
    for form, scope in (("qs", "QsLds"), ("sqrl", "SqLds")):
        own = _constants(ev, scope)
        for name, T in (("f16x3", T16), ("f32", T32)):
            env = dict(T, kRows=_value("kRows", roll, tile), kMaxK=_value("kMaxK", roll), kSqMaxK=_value("kSqMaxK", roll))
            sizes[form, name] = _value("kBytes", own, env=env)
    assert sizes["qs", "f32"] == 84368 and sizes["sqrl", "f32"] == 105424           # 82.4 KB and 103.0 KB: the f32 forms'
    assert sizes["qs", "f16x3"] == sizes["qs", "f32"] + 1024 and sizes["sqrl", "f16x3"] == sizes["sqrl", "f32"] + 1024
    assert max(sizes.values()) < 160 * 1024                                          # one workgroup of a gfx950 CU's LDS
    assert 2 * min(sizes.values()) > 160 * 1024                                      # ... and no second one: as the f32 forms
    # the policy stack's regions (kLdsFloats, the four-output partial sums) end before the f16x3 tile's xs
    stack = {n: _value(n, roll, tile) for n in ("kLdsFloats", "kOffPart", "kWaves")}
    assert stack["kLdsFloats"] <= T16["kOffXs"]
    assert stack["kOffPart"] + 4 * stack["kWaves"] * 16 <= T16["kOffXs"]
    # ... and the kernels are built on them: every form's trait declares the carve-up of its own tile as its LDS and its
    # occupancy (two waves per SIMD for the four candidate forms, four for the base form) ...
    for name in ("kLdsFloats <= Tile::kOffXs", "kOffPart + 4 * kWaves * kRows <= Tile::kOffXs"):
        assert name in ev, name
    forms = dict(re.findall(r"\nstruct (NoQs|QsOn|QsOnH|SqOn|SqOnH) \{(.*?)\n\};", ev, flags=re.S))
    for form, (tile, lds) in {"QsOn": ("TileF32", "QsLds"), "QsOnH": ("TileF16x3", "QsLds"), "SqOn": ("TileF32", "SqLds"),
                              "SqOnH": ("TileF16x3", "SqLds")}.items():
        own = _constants(forms[form])
        assert re.findall(r"using Tile = (\w+);", forms[form]) == [tile], form
        assert own["kLds"] == lds + "<Tile>::kBytes" and own["kWavesPerEu"] == "2", form
    base = _constants(forms["NoQs"])
    assert base["kLds"] == "kLdsBytes" and base["kWavesPerEu"] == "4" and "Tile" not in forms["NoQs"]
    # ... and the two kernel templates and the one launch take both from that declaration and from nowhere else
    assert len(re.findall(r"__global__", re.sub(r"//[^\n]*", "", ev))) == 2
    assert re.findall(r"amdgpu_waves_per_eu\(([^)]*)\)", ev) == ["Form::kWavesPerEu, Form::kWavesPerEu"] * 2
    assert not re.search(r"amdgpu_waves_per_eu\(\s*\d", ev)
    assert re.findall(r"hipLaunchKernelGGL\(kernel, [^,]*, dim3\(kThreads\), ([^,]*),", ev) == ["Form::kLds"]
    assert ev.count("hipLaunchKernelGGL") == 1 and len(re.findall(r"grant_lds\(kernel, ([^,]*),", ev)) == 1
