"""SQRL acting with f16x3 scores (RRL_SQRL_F16X3=1: rrl_w2_pack_f16x3, rrl_sqrl_act_f16x3, rrl_sqrl_act_f16x3_packed), the
parts that need no GPU: the ABI, the switch, what FastActor.act_sqrl issues and records, what seed packing builds from it --
and the fairness of the case table tests/test_sqrl_f16x3_gpu.py measures the kernel on: the emulated chain passes the
project's bars at every shape, and each mistake an f16x3 kernel can make breaks the rule on a case of the table."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import arg_utils
import sqrl_f16x3_cases as SC
from recovery_rl_amd import _lib, fast_update, packed
from recovery_rl_amd.experiment import run_packed
from test_sqrl_act_cpu import EINVAL, ERANGE, KS, MODES, NS, SQRL, _cfg, _desc, case, left_out_cap, make_agent, restate_pick, weights64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("rrl_sqrl_act_f16x3", "rrl_sqrl_act_f16x3_packed")


# ---- ABI ---------------------------------------------------------------------------------------------------------------
def test_symbols_are_declared_exported_and_additive():
    code = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rrl_hip.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+rrl_w2_pack_f16x3\s*\(\s*int\s+G\s*,\s*int\s+H\s*,\s*const\s+float\s*\*\s*W2\s*,\s*float\s*\*\s*W2h\s*,"
                     r"\s*void\s*\*\s*stream\s*\)", code)
    assert re.search(r"\bint\s+rrl_sqrl_act_f16x3\s*\(\s*const\s+rrl_sqrl_act_t\s*\*", code)
    assert re.search(r"\bint\s+rrl_sqrl_act_f16x3_packed\s*\(\s*int\s+S\s*,\s*const\s+rrl_sqrl_act_t\s*\*", code)
    lib = _lib.load()
    for name in ("rrl_w2_pack_f16x3",) + ENTRIES:
        assert name in _lib.EXPORTS and getattr(lib, name).argtypes is not None
        assert name in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "sqrl_f16x3_kernels.hip" in _lib.HIP_SOURCES
    assert lib.rrl_abi_version() == 8                       # additive: nothing existing changed layout
    assert lib.rrl_sqrl_act_f16x3.argtypes[0] == C.POINTER(_lib.rrl_sqrl_act_t)
    assert lib.rrl_sqrl_act_f16x3_packed.argtypes[:2] == [C.c_int, C.POINTER(_lib.rrl_sqrl_act_t)]


def _calls(lib):
    """name -> rc of one descriptor, for the two f16x3 entries and the two f32 entries beside them"""
    return {"rrl_sqrl_act": lambda a: lib.rrl_sqrl_act(None if a is None else C.byref(a), None),
            "rrl_sqrl_act_f16x3": lambda a: lib.rrl_sqrl_act_f16x3(None if a is None else C.byref(a), None),
            "rrl_sqrl_act_packed": lambda a: lib.rrl_sqrl_act_packed(1, None if a is None else C.byref(a), None),
            "rrl_sqrl_act_f16x3_packed": lambda a: lib.rrl_sqrl_act_f16x3_packed(1, None if a is None else C.byref(a), None)}


def test_descriptor_validation_is_the_f32_entries_matrix():
    """The matrix of tests/test_sqrl_act_cpu.py on all four entries: the same code from each, EINVAL before ERANGE."""
    calls = _calls(_lib.load())
    matrix = [(None, EINVAL)]
    matrix += [(_desc(**{name: None}), EINVAL)
               for name in ("obs", "head", "scale", "bias", "W1", "b1", "W2p", "b2", "W3", "b3", "action")]
    matrix += [(_desc(**f), EINVAL) for f in (dict(n=0), dict(n=-4), dict(H=32), dict(H=512), dict(d_obs=3), dict(d_act=1),
                                              dict(n_part=0), dict(n_part=5), dict(W2p=0x1004), dict(W2p=0x1008))]
    matrix += [(_desc(**f), ERANGE) for f in (dict(k=0), dict(k=-1), dict(k=129), dict(n=2 ** 31 - 1, k=3),
                                              dict(n=2 ** 25, k=128))]
    matrix += [(_desc(k=500, H=32), EINVAL)]                 # an invalid field wins over a size out of range
    for a, want in matrix:
        got = {name: f(a) for name, f in calls.items()}
        assert set(got.values()) == {want}, got


def test_packed_entry_checks_every_seed_before_anything_else():
    lib = _lib.load()
    two = lambda *d: (_lib.rrl_sqrl_act_t * len(d))(*d)
    for fn in (lib.rrl_sqrl_act_packed, lib.rrl_sqrl_act_f16x3_packed):
        assert fn(0, two(_desc()), None) == EINVAL and fn(17, two(_desc()), None) == EINVAL and fn(2, None, None) == EINVAL
        assert fn(2, two(_desc(), _desc(obs=None)), None) == EINVAL
        assert fn(2, two(_desc(), _desc(k=129)), None) == ERANGE
        assert fn(2, two(_desc(k=129), _desc(H=32)), None) == ERANGE         # seed 0's code comes first
        assert fn(2, two(_desc(k=100), _desc(k=64)), None) == EINVAL          # one k per call, refused before any launch
        assert fn(3, two(_desc(k=16), _desc(k=16), _desc(k=17)), None) == EINVAL


def test_w2_pack_f16x3_validation():
    lib = _lib.load()
    d = 0x1000
    assert lib.rrl_w2_pack_f16x3(2, 16, d, d, None) == EINVAL          # H % 32
    assert lib.rrl_w2_pack_f16x3(2, 48, d, d, None) == EINVAL
    assert lib.rrl_w2_pack_f16x3(2, 0, d, d, None) == EINVAL and lib.rrl_w2_pack_f16x3(0, 256, d, d, None) == EINVAL
    assert lib.rrl_w2_pack_f16x3(2, 256, None, d, None) == EINVAL and lib.rrl_w2_pack_f16x3(2, 256, d, None, None) == EINVAL
    assert lib.rrl_w2_pack_f16x3(2, 256, d, d + 8, None) == EINVAL     # 16-byte alignment of the stream


def test_f16x3_kernels_are_f16_mfma_code_at_four_waves_per_simd_without_scratch(tmp_path):
    """The sixteen acting kernels of the built library: layer 2 on v_mfma_f32_16x16x32_f16 (layer 1 on the f32 shape), within
    the 128 VGPRs of amdgpu_waves_per_eu(4, 4), nothing in scratch."""
    from isa_util import kernel_table
    table = {k: v for k, v in kernel_table(_lib.SO_PATH, str(tmp_path)).items() if "vgpr" in v and "sqrl_act_f16x3" in k}
    assert len(table) == 16, sorted(table)
    for name, v in table.items():
        count = lambda prefix: sum(n for op, n in v["ins"].items() if op.startswith(prefix))
        assert v["vgpr"] <= 128 and v["scratch"] == 0, (name, v["vgpr"], v["scratch"])
        assert count("v_mfma_f32_16x16x32_f16") >= 24 and 0 < count("v_mfma_f32_16x16x4_f32") <= 16, name
        assert count("scratch_") == 0, name


# ---- the switch --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f16x3,baselines,sqrl,flags,want", [
    ("1", "1", "1", SQRL, "f16x3"),
    ("1", "1", "1", ["--use_constraint_sampling"], "f16x3"),
    (None, "1", "1", SQRL, "f32"),                                                 # opt-in
    ("0", "1", "1", SQRL, "f32"),
    ("1", "1", None, SQRL, "f32"),                                                 # ignored where the pass is not the kernel's
    ("1", None, "1", SQRL, "f32"),
    ("1", "1", "1", SQRL + ["--use_recovery", "--MF_recovery"], "f32"),            # with a recovery policy
    ("1", "1", "1", SQRL + ["--hidden_size", "32"], "f32"),                        # other hidden widths
    ("1", "1", "1", ["--DGD_constraints", "--nu", "5000", "--update_nu"], "f32"),  # LR: no constraint sampling
])
def test_switch_matrix(monkeypatch, f16x3, baselines, sqrl, flags, want):
    for name, val in (("RRL_SQRL_F16X3", f16x3), ("RRL_FAST_BASELINES", baselines), ("RRL_FAST_SQRL", sqrl)):
        if val is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, val)
    monkeypatch.delenv("RRL_W2_FRAG", raising=False)
    assert fast_update.sqrl_f16x3_enabled() == (f16x3 == "1")
    assert fast_update.sqrl_scoring(_cfg(*flags)) == want
    # the switch does not move the path decision
    monkeypatch.delenv("RRL_SQRL_F16X3", raising=False)
    path = fast_update.sqrl_acting_path(_cfg(*flags))
    monkeypatch.setenv("RRL_SQRL_F16X3", "1")
    assert fast_update.sqrl_acting_path(_cfg(*flags)) == path and (want == "f32" or path == "hip")


def _recorded(monkeypatch, f16x3):
    """FastActor.act_sqrl with the library's calls recorded (nothing runs) -> (names, tape, actor, fast, action)."""
    real, names = _lib.load(), []

    class Recorder:
        def __getattr__(self, name):
            if name in ("rrl_mlp3_is_split", "rrl_abi_version", "rrl_last_hip_error"):
                return getattr(real, name)
            fn = lambda *args: names.append(name[4:]) or 0
            fn.__name__ = name
            return fn

    monkeypatch.setattr(_lib, "_lib", Recorder())
    monkeypatch.setattr(_lib, "current_stream", lambda: 0)
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: False)
    fast = make_agent("cpu").enable_fast_path(256)
    actor = fast_update.FastActor(fast, 128)
    fast.qrisk.w2p = torch.empty(2 * 256 * 256)
    actor.sqrl_seed = 77
    actor.sqrl_f16x3 = f16x3
    tape = []
    fast_update.set_tape(tape)
    try:
        out = actor.act_sqrl(torch.zeros(128, 2), 0.3)
    finally:
        fast_update.set_tape(None)
    return names, tape, actor, fast, out


def test_act_sqrl_under_the_switch_packs_w2_then_launches_the_f16x3_kernel(monkeypatch):
    names, tape, actor, fast, out = _recorded(monkeypatch, True)
    assert out is actor.task_action
    assert names == ["w2_pack", "mlp3_forward_multi", "w2_pack_f16x3", "sqrl_act_f16x3"]
    assert [op[0] for op in tape] == ["forward", "call", "sqrl_f16x3"]
    W2 = fast.qrisk.p["W2"]
    assert actor.sqrl_w2h is not None and actor.sqrl_w2h.numel() == 2 * 256 * 256 and actor.sqrl_w2h.dtype == torch.float32
    assert tape[1][1].__name__ == "rrl_w2_pack_f16x3"
    assert tape[1][2] == (2, 256, W2.data_ptr(), actor.sqrl_w2h.data_ptr())          # the LIVE W2, every pass
    a = tape[2][1]
    assert isinstance(a, _lib.rrl_sqrl_act_t) and (a.n, a.k, a.H, a.d_obs, a.d_act) == (128, 100, 256, 2, 2)
    assert a.W2p == actor.sqrl_w2h.data_ptr() != fast.qrisk.w2p.data_ptr()
    assert a.W1 == fast.qrisk.p["W1"].data_ptr() and a.action == actor.task_action.data_ptr()
    assert (a.seed, a.counter, a.counter_inc, a.counter_dev) == (77, 0, 1, actor.sqrl_tick.data_ptr())
    head, n_part, ps = actor.pol.parts
    assert (a.head, a.n_part, a.part_stride) == (head.data_ptr(), n_part, ps)
    # the second pass re-uses the buffer and packs again
    w2h = actor.sqrl_w2h
    del names[:]
    actor.act_sqrl(torch.zeros(128, 2), 0.3)
    assert actor.sqrl_w2h is w2h and names[-2:] == ["w2_pack_f16x3", "sqrl_act_f16x3"]


def test_act_sqrl_without_the_switch_is_todays_sequence(monkeypatch):
    names, tape, actor, fast, _ = _recorded(monkeypatch, False)
    assert names == ["w2_pack", "mlp3_forward_multi", "sqrl_act"] and [op[0] for op in tape] == ["forward", "sqrl"]
    assert tape[1][1].W2p == fast.qrisk.w2p.data_ptr() and actor.sqrl_w2h is None
    assert fast_update.FastActor(fast, 8).sqrl_f16x3 is False                      # off unless the loop sets it


def test_packed_stages_of_the_f16x3_tape(monkeypatch):
    """Kind "sqrl_f16x3" becomes one rrl_sqrl_act_f16x3_packed stage over the seeds' descriptors; the pack calls ride as the
    per-seed "call" stage in front of it."""
    names, tape, actor, fast, _ = _recorded(monkeypatch, True)
    loop = packed.PackedLoop.__new__(packed.PackedLoop)
    loop.S, loop.lib, loop.tapes = 2, _lib.load(), [tape, tape]
    stages = loop._build_stages()
    assert [ops[0][0] for _, _, ops in stages] == ["forward", "call", "sqrl_f16x3"]
    fn, (S, args), _ = stages[2]
    assert fn.__name__ == "rrl_sqrl_act_f16x3_packed" and S == 2 and args[1].W2p == actor.sqrl_w2h.data_ptr()
    fn, (calls,), _ = stages[1]
    assert fn == loop._call_each and [c[0].__name__ for c in calls] == ["rrl_w2_pack_f16x3"] * 2
    loop.stages = stages
    assert loop.launches == 1 + 2 + 1


@pytest.mark.parametrize("env,match", [
    ({"RRL_FAST_BASELINES": "1", "RRL_FAST_SQRL": "1", "RRL_SQRL_F16X3": "1"}, "use_constraint_sampling"),   # no RRL_PACK_SQRL
    ({"RRL_FAST_BASELINES": "1", "RRL_PACK_SQRL": "1", "RRL_SQRL_F16X3": "1"}, "RRL_FAST_SQRL"),
    ({"RRL_FAST_SQRL": "1", "RRL_PACK_SQRL": "1", "RRL_SQRL_F16X3": "1"}, "RRL_FAST_BASELINES"),
])
def test_run_packed_refuses_what_it_refuses_without_the_switch(monkeypatch, tmp_path, env, match):
    for name in ("RRL_FAST_BASELINES", "RRL_FAST_SQRL", "RRL_PACK_SQRL", "RRL_SQRL_F16X3"):
        monkeypatch.delenv(name, raising=False)
    for name, val in env.items():
        monkeypatch.setenv(name, val)
    cfg = arg_utils.get_args(["--env-name", "navigation1", "--cuda", "--num_envs", "128", "--seeds_per_gpu", "2",
                              "--gamma_safe", "0.8", "--eps_safe", "0.3", "--logdir", str(tmp_path)] + SQRL)
    with pytest.raises(ValueError, match=match):
        run_packed(cfg)
    assert not os.listdir(tmp_path)


def test_run_packed_keeps_the_seed_limit_under_the_switch(monkeypatch, tmp_path):
    for name in ("RRL_FAST_BASELINES", "RRL_FAST_SQRL", "RRL_PACK_SQRL", "RRL_SQRL_F16X3"):
        monkeypatch.setenv(name, "1")
    cfg = arg_utils.get_args(["--env-name", "navigation1", "--cuda", "--num_envs", "128", "--seeds_per_gpu", "9",
                              "--gamma_safe", "0.8", "--eps_safe", "0.3", "--logdir", str(tmp_path)] + SQRL)
    with pytest.raises(ValueError, match="at most 8 seeds"):
        run_packed(cfg)


# ---- the emulated restatement and the fairness of the case table ------------------------------------------------------
@pytest.fixture(scope="module")
def agent():
    return make_agent("cpu")


@pytest.fixture(scope="module")
def table(agent):
    """Per shape: the case, the float64 and f32 emulations -- computed once for the tests below."""
    W = weights64(agent)
    out = {}
    for n, k in SC.SHAPES:
        c = case(agent, n, k)
        out[n, k] = (c, SC.emulate(W, c, np.float64), SC.emulate(W, c, np.float32))
    return W, out


def test_split16_is_the_documented_split():
    v = np.array([0.0, 1.0, 0.1, 3.14159, 1e-3, 2.0 ** -20, 70000.0, 65504.0, 65520.0, np.nan], np.float32)
    hi, lo = SC.split16(v, np.float32)
    assert hi[6] == hi[7] == hi[8] == 65504.0 and lo[6] == lo[7] == lo[8] == 0.0 and np.isnan(hi[9])
    assert np.array_equal(hi[:6], v[:6].astype(np.float16).astype(np.float32))
    assert np.all(np.abs(v[:6] - (hi[:6] + lo[:6])) <= np.maximum(2.0 ** -22 * np.abs(v[:6]), 2.0 ** -25))
    assert lo[5] == 0.0                                     # 2^-20 is an f16 (subnormal) value itself
    assert 0.0 < abs(lo[4]) < 2.0 ** -14 and SC.split16(v, np.float32, flush=True)[1][4] == 0.0     # 1e-3: a subnormal lo
    h, lo_open = SC.split16(v, np.float32, clamp=False)
    assert np.isinf(h[6]) and not np.isfinite(lo_open[6])


@pytest.mark.parametrize("n,k", SC.SHAPES)
def test_emulated_chain_stays_inside_the_projects_bars(table, n, k):
    """Both emulations at every shape: z within 1e-4 of scale and q within 1e-5 of the plain float64 chain, and the float64
    emulation's decisions are the plain chain's on every non-ambiguous row, under the cap, in the three modes."""
    _, cases = table
    c, e64, e32 = cases[n, k]
    z64, scale = c["scores"]["z"], float(np.abs(c["scores"]["z"]).max())
    for name, e in (("float64", e64), ("f32", e32)):
        dz, dq = SC.deviation(e["z"], z64), float(np.abs(e["q"] - c["scores"]["q"]).max())
        print("n=%d k=%d %s emulation: z error %.3e (scale %.3e), q error %.3e" % (n, k, name, dz, scale, dq))
        assert dz <= 1e-4 * scale and dq <= 1e-5
    for mode in MODES:
        want = c["pick"][mode]
        keep = ~want["ambiguous"]
        assert (~keep).sum() <= left_out_cap(n), (mode, int((~keep).sum()))         # a condition on the table
        got = restate_pick(e64["q"], c["scores"]["logp"], c["u"], c["thr"][mode])
        for name in ("n_safe", "cstar", "pick"):
            assert np.array_equal(got[name][keep], want[name][keep]), (mode, name)


@pytest.mark.parametrize("mutation", SC.MUTATIONS)
def test_each_mutation_breaks_the_rule_on_a_case_of_the_table(agent, table, mutation):
    """A kernel that drops a cross product, flushes subnormal lo values or forgets the clamp computes the mutated f32
    emulation (up to summation order); the rule of the GPU test refuses it on at least one case, and by a margin."""
    W, cases = table
    seen = []
    for (n, k), (c, e64, e32) in cases.items():
        z64 = c["scores"]["z"]
        dev = SC.deviation(SC.emulate(W, c, np.float32, mutation)["z"], z64)
        if dev > 2 * SC.bound(z64, e32["z"]):
            seen.append((n, k))
    sat = SC.saturation_case(agent)
    assert sat["saturated"] > 0.1
    z64, z32 = SC.emulate(W, sat)["z"], SC.emulate(W, sat, np.float32)["z"]
    assert np.isfinite(z64).all() and SC.deviation(z32, z64) <= SC.bound(z64, z32) / SC.FACTOR
    if SC.deviation(SC.emulate(W, sat, np.float32, mutation)["z"], z64) > 2 * SC.bound(z64, z32):
        seen.append("saturation")
    print(mutation, "seen on", seen)
    if mutation == "no_clamp":
        assert seen == ["saturation"]                       # nothing else reaches the f16 range
    else:
        assert len(seen) >= len(SC.SHAPES)                  # the cross products and the subnormal lo matter at every shape
