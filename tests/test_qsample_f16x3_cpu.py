"""Q-sampling recovery acting with f16x3 scores (RRL_QSAMPLE_F16X3=1: rrl_qsample_act_f16x3, rrl_qsample_act_gated_f16x3,
rrl_qsample_act_f16x3_packed), the parts that need no GPU: the ABI, the switch, what FastActor.act_qsample issues and records,
what seed packing builds from it, what --resume refuses -- and the fairness of the case table tests/test_qsample_f16x3_gpu.py
measures the kernels on (tests/qsample_f16x3_cases.py): the float64 emulation alone is inside rules Z and Q on every case, the
bound is not its floor alone, and each mistake an f16x3 kernel can make breaks rule Z on a case of the table."""
import ctypes as C
import os
import re
import types

import numpy as np
import pytest
import torch

import qsample_f16x3_cases as QC
import sqrl_f16x3_cases as SC
from recovery_rl_amd import _lib, checkpoint, fast_update
from recovery_rl_amd.packed import PackedLoop
from test_qsample_act_cpu import EINVAL, ERANGE, QS, _cfg, _desc, make_agent

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("rrl_qsample_act_f16x3", "rrl_qsample_act_gated_f16x3", "rrl_qsample_act_f16x3_packed")
# what the parent exported: every one of them is still there
PARENT_EXPORTS = ("rrl_abi_version", "rrl_w2_pack", "rrl_recovery_select", "rrl_sqrl_scratch_floats", "rrl_sqrl_act",
                  "rrl_sqrl_act_packed", "rrl_qsample_scratch_floats", "rrl_qsample_act", "rrl_qsample_act_gated",
                  "rrl_qsample_act_packed", "rrl_eval_rollout", "rrl_eval_rollout_packed", "rrl_eval_rollout_maze",
                  "rrl_eval_rollout_maze_packed", "rrl_eval_rollout_qs", "rrl_eval_rollout_qs_packed", "rrl_eval_rollout_sqrl",
                  "rrl_eval_rollout_sqrl_packed", "rrl_w2_pack_f16x3", "rrl_sqrl_act_f16x3", "rrl_sqrl_act_f16x3_packed")
PARENT_SITES = ["HiddenBackward", "StackForward", "HeadBackward", "BackwardPair", "Adam", "AdamDuals", "PolicyHeads", "RcpoPenalty",
                "ReplayDraw", "NavStep", "MazeStep", "SqrlAct", "QsampleAct", "EvalRollout", "EvalRolloutMaze", "EvalRolloutQs",
                "EvalRolloutSqrl", "SqrlActF16x3"]


# ---- ABI ---------------------------------------------------------------------------------------------------------------
def test_symbols_are_declared_exported_and_additive():
    code = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rrl_hip.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+rrl_qsample_act_f16x3\s*\(\s*const\s+rrl_qsample_act_t\s*\*\s*\w+\s*,\s*void\s*\*\s*stream\s*\)", code)
    assert re.search(r"\bint\s+rrl_qsample_act_gated_f16x3\s*\(\s*const\s+rrl_qsample_act_t\s*\*\s*\w+\s*,\s*const\s+"
                     r"rrl_qsample_gate_t\s*\*\s*\w+\s*,\s*void\s*\*\s*stream\s*\)", code)
    assert re.search(r"\bint\s+rrl_qsample_act_f16x3_packed\s*\(\s*int\s+S\s*,\s*const\s+rrl_qsample_act_t\s*\*\s*\w+\s*,\s*const\s+"
                     r"rrl_qsample_gate_t\s*\*\s*\w+\s*,\s*void\s*\*\s*stream\s*\)", code)
    lib = _lib.load()
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in ENTRIES:
        assert name in _lib.EXPORTS and getattr(lib, name).argtypes is not None and getattr(lib, name).restype == C.c_int
        assert name in integration
    for name in PARENT_EXPORTS:
        assert name in _lib.EXPORTS and getattr(lib, name) is not None, name
    assert "qsample_f16x3_kernels.hip" in _lib.HIP_SOURCES and "qsample_kernels.hip" in _lib.HIP_SOURCES
    assert lib.rrl_abi_version() == 8                       # additive: nothing existing changed layout
    A, G = C.POINTER(_lib.rrl_qsample_act_t), C.POINTER(_lib.rrl_qsample_gate_t)
    assert lib.rrl_qsample_act_f16x3.argtypes == [A, C.c_void_p]
    assert lib.rrl_qsample_act_gated_f16x3.argtypes == [A, G, C.c_void_p]
    assert lib.rrl_qsample_act_f16x3_packed.argtypes == [C.c_int, A, G, C.c_void_p]


def test_pack_site_is_appended():
    src = open(os.path.join(_lib.CSRC, "pack.hpp")).read()
    body = re.search(r"enum class Site : int \{(.*?)\};", src, flags=re.S).group(1)
    names = [n.split("=")[0].strip() for n in body.split(",") if n.strip()]
    assert names == PARENT_SITES + ["QsampleActF16x3", "EvalRolloutQsF16x3", "EvalRolloutSqrlF16x3"]
    assert re.search(r"HiddenBackward\s*=\s*1\b", body)


def _gate(**fields):
    d = 0x1000
    g = _lib.rrl_qsample_gate_t(z=d, n_part=2, part_stride=16, eps_safe=0.3, task_action=d, ld_task=4, task_out=d, recovery_out=d)
    for k, v in fields.items():
        setattr(g, k, v)
    return g


def test_descriptor_validation_is_the_f32_entries_matrix():
    """The matrices of tests/test_qsample_act_cpu.py and tests/test_packed_qsample_cpu.py on the f16x3 entries beside the f32
    ones: the same code from each, before anything is launched (there is no device here to launch on)."""
    lib = _lib.load()
    ref = lambda a: None if a is None else C.byref(a)
    solo = {"f32": lambda a: lib.rrl_qsample_act(ref(a), None), "f16x3": lambda a: lib.rrl_qsample_act_f16x3(ref(a), None),
            "f32 packed": lambda a: lib.rrl_qsample_act_packed(1, ref(a), None, None),
            "f16x3 packed": lambda a: lib.rrl_qsample_act_f16x3_packed(1, ref(a), None, None)}
    matrix = [(None, EINVAL)]
    matrix += [(_desc(**{name: None}), EINVAL) for name in ("obs", "lo", "hi", "W1", "b1", "W2p", "b2", "W3", "b3", "scratch", "action")]
    matrix += [(_desc(**f), EINVAL) for f in (dict(n=0), dict(n=-4), dict(H=32), dict(H=512), dict(d_obs=3), dict(d_act=1),
                                              dict(W2p=0x1004), dict(W2p=0x1008), dict(k=5000, H=32), dict(k=0, scratch=None))]
    matrix += [(_desc(**f), ERANGE) for f in (dict(k=0), dict(k=-1), dict(k=1025), dict(n=2 ** 31 - 1, k=3), dict(n=2 ** 22, k=1024))]
    for a, want in matrix:
        got = {name: f(a) for name, f in solo.items()}
        assert set(got.values()) == {want}, got
    gated = {"f32": lib.rrl_qsample_act_gated, "f16x3": lib.rrl_qsample_act_gated_f16x3}
    gmatrix = [(_desc(), None, EINVAL), (None, _gate(), EINVAL), (_desc(mask=0x1000), _gate(), EINVAL), (_desc(H=32), _gate(), EINVAL),
               (_desc(k=1025), _gate(), ERANGE), (_desc(k=1025), _gate(n_part=5), EINVAL), (_desc(k=0, mask=0x1000), _gate(), EINVAL)]
    gmatrix += [(_desc(), _gate(**f), EINVAL) for f in (dict(z=None), dict(task_action=None), dict(recovery_out=None), dict(n_part=0),
                                                      dict(n_part=5), dict(ld_task=0), dict(ld_task=3))]
    for a, g, want in gmatrix:
        got = {name: fn(ref(a), ref(g), None) for name, fn in gated.items()}
        assert set(got.values()) == {want}, got
    arr = lambda typ, items: (typ * len(items))(*items)
    A, G = _lib.rrl_qsample_act_t, _lib.rrl_qsample_gate_t
    for fn in (lib.rrl_qsample_act_packed, lib.rrl_qsample_act_f16x3_packed):
        for S in (0, -1, 17):
            assert fn(S, arr(A, [_desc()] * 17), arr(G, [_gate()] * 17), None) == EINVAL
        assert fn(3, None, arr(G, [_gate()] * 3), None) == EINVAL
        for at in range(3):                                 # one bad seed refuses the call, wherever it sits
            for fields, code in ((dict(k=1025), ERANGE), (dict(H=128), EINVAL), (dict(obs=None), EINVAL), (dict(mask=0x1000), EINVAL)):
                bad = [_desc() for _ in range(3)]
                bad[at] = _desc(**fields)
                assert fn(3, arr(A, bad), arr(G, [_gate()] * 3), None) == code, (at, fields)
        n = (2 ** 31 - 1) // 16 // 2 + 1                    # more than INT32_MAX / 16 score workgroups
        assert fn(2, arr(A, [_desc(), _desc(n=n, k=129)]), arr(G, [_gate()] * 2), None) == ERANGE
    assert lib.rrl_qsample_scratch_floats(4096, 1000) == 4 * 4096 * 8          # one scratch size for both families


def test_score_kernels_are_f16_mfma_code_at_four_waves_per_simd_without_scratch(tmp_path):
    """The two new score kernels of the built library: layer 2 on v_mfma_f32_16x16x32_f16 (layer 1 on the f32 shape), within the
    128 VGPRs of amdgpu_waves_per_eu(4, 4), nothing in scratch; the fold kernels exist once, for both families."""
    from isa_util import kernel_table
    table = {k: v for k, v in kernel_table(_lib.SO_PATH, str(tmp_path)).items() if "vgpr" in v and "qsample" in k}
    new = {k: v for k, v in table.items() if "qsample_score_f16x3" in k}
    assert len(new) == 2 and any("pack_kernel" in k for k in new), sorted(table)
    assert len([k for k in table if "qsample_fold" in k]) == 2
    for name, v in new.items():
        count = lambda prefix: sum(n for op, n in v["ins"].items() if op.startswith(prefix))
        assert v["vgpr"] <= 128 and v["scratch"] == 0 and count("scratch_") == 0, (name, v["vgpr"], v["scratch"])
        assert count("v_mfma_f32_16x16x32_f16") >= 24 and 0 < count("v_mfma_f32_16x16x4_f32") <= 20, name
        assert count("flat_load") == 0, name


# ---- the switch --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f16x3,fast,flags,frag,want", [
    ("1", "1", QS, None, "f16x3"),
    ("1", "1", QS + ["--hidden_size", "256"], None, "f16x3"),
    (None, "1", QS, None, "f32"),                                                  # opt-in
    ("0", "1", QS, None, "f32"),
    ("1", None, QS, None, "f32"),                                                  # the switch alone: the pass is not the kernels'
    ("1", "0", QS, None, "f32"),
    ("1", "1", QS + ["--MF_recovery"], None, "f32"),                               # model-free recovery wins
    ("1", "1", QS + ["--hidden_size", "32"], None, "f32"),                         # other hidden widths
    ("1", "1", QS + ["--hidden_size", "512"], None, "f32"),
    ("1", "1", QS, "0", "f32"),                                                    # RRL_W2_FRAG=0
    ("1", "1", ["--use_recovery"], None, "f32"),                                   # model-based recovery
    ("1", "1", QS + ["--no_fast_path"], None, "f32"),
])
def test_switch_matrix(monkeypatch, f16x3, fast, flags, frag, want):
    for name, val in (("RRL_QSAMPLE_F16X3", f16x3), ("RRL_FAST_QSAMPLE", fast), ("RRL_W2_FRAG", frag)):
        if val is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, val)
    assert fast_update.qsample_f16x3_enabled() == (f16x3 == "1")
    cfg = _cfg(*flags)
    assert fast_update.qsample_scoring(cfg) == want
    # the switch does not move the path decision, and f16x3 exists on the kernel path only
    monkeypatch.delenv("RRL_QSAMPLE_F16X3", raising=False)
    path = fast_update.qsample_acting_path(cfg)
    monkeypatch.setenv("RRL_QSAMPLE_F16X3", "1")
    assert fast_update.qsample_acting_path(cfg) == path and (want == "f32" or path == "hip")
    assert fast_update.qsample_scoring(cfg) == ("f16x3" if path == "hip" else "f32")


# ---- the tape ----------------------------------------------------------------------------------------------------------
@pytest.fixture
def recorded(monkeypatch):
    """The library's calls recorded (nothing runs), as tests/test_qsample_act_cpu.py does."""
    real, calls = _lib.load(), []

    class Recorder:
        def __getattr__(self, name):
            if name in ("rrl_mlp3_is_split", "rrl_abi_version", "rrl_last_hip_error", "rrl_qsample_scratch_floats"):
                return getattr(real, name)
            fn = lambda *args: calls.append((name[4:], args)) or 0
            fn.__name__ = name
            return fn

    monkeypatch.setattr(_lib, "_lib", Recorder())
    monkeypatch.setattr(_lib, "current_stream", lambda: 0)
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: False)
    fast = make_agent("cpu").enable_fast_path(256)
    for net in (fast.qrisk, fast.policy):                   # (a CPU FlatNet keeps no fragment-order copy)
        net.w2p = torch.empty(net.p["W2"].numel())
    return fast, calls


def _taped(fn):
    tape = []
    fast_update.set_tape(tape)
    try:
        out = fn()
    finally:
        fast_update.set_tape(None)
    return out, tape


@pytest.mark.parametrize("gated", (False, True))
def test_act_qsample_under_the_switch_packs_w2_then_launches_the_f16x3_kernels(recorded, gated):
    fast, calls = recorded
    n = 128
    obs = torch.zeros(n, 2)
    # the parent's pass first: the same actor state, switch off
    plain = fast_update.FastActor(fast, n)
    assert plain.qsample_f16x3 is False and plain.qsample_w2h is None              # off unless the loop sets it
    del calls[:]
    _, tape32 = _taped(lambda: plain.act_qsample(obs, 0.3, gated=gated))
    names32 = [c[0] for c in calls]
    assert tape32[-1][0] == "qsample" and "qsample_f16x3" not in [op[0] for op in tape32] and plain.qsample_w2h is None
    assert names32[-1] == ("qsample_act_gated" if gated else "qsample_act") and "w2_pack_f16x3" not in names32
    assert tape32[-1][1].W2p == fast.qrisk.w2p.data_ptr()

    actor = fast_update.FastActor(fast, n)
    actor.qsample_seed = 77
    actor.qsample_f16x3 = True
    fast._actor_noise_fresh = False
    del calls[:]
    out, tape = _taped(lambda: actor.act_qsample(obs, 0.3, gated=gated))
    assert out[0] is actor.task_action and out[1] is actor.real_action and out[2] is actor.recovery
    names = [c[0] for c in calls]
    entry = "qsample_act_gated_f16x3" if gated else "qsample_act_f16x3"
    assert names[:-2] == names32[:-1] and names[-2:] == ["w2_pack_f16x3", entry]
    kinds = [op[0] for op in tape]
    assert kinds[:-2] == [op[0] for op in tape32][:-1] and kinds[-2:] == ["call", "qsample_f16x3"]
    W2, w2h = fast.qrisk.p["W2"], actor.qsample_w2h
    assert w2h is not None and w2h.numel() == W2.numel() == 2 * 256 * 256 and w2h.dtype == torch.float32
    _, fn, args, keep = tape[-2]
    assert fn.__name__ == "rrl_w2_pack_f16x3" and args == (2, 256, W2.data_ptr(), w2h.data_ptr())      # the LIVE W2, every pass
    assert keep[0] is W2 and keep[1] is w2h
    a = tape[-1][1]
    assert isinstance(a, _lib.rrl_qsample_act_t) and (a.n, a.k, a.H, a.d_obs, a.d_act) == (n, 1000, 256, 2, 2)
    assert a.W2p == w2h.data_ptr() != fast.qrisk.w2p.data_ptr()
    assert a.W1 == fast.qrisk.p["W1"].data_ptr() and a.action == actor.real_action.data_ptr()
    assert (a.seed, a.counter, a.counter_inc, a.counter_dev) == (77, 0, 1, actor.qsample_tick.data_ptr())
    assert a.scratch == actor._qsample_scratch.data_ptr() and actor._qsample_scratch.numel() == 4 * n * 8
    if gated:
        assert len(tape[-1]) == 3 and isinstance(tape[-1][2], _lib.rrl_qsample_gate_t) and not a.mask
        assert tape[-1][2].recovery_out == actor.recovery.data_ptr()
        last = calls[-1][1]
        assert C.addressof(last[0]._obj) == C.addressof(a) and C.addressof(last[1]._obj) == C.addressof(tape[-1][2])
    else:
        assert len(tape[-1]) == 2 and a.mask == actor.recovery.data_ptr()
    # the second pass re-uses the buffer and packs again
    del calls[:]
    actor.act_qsample(obs, 0.3, gated=gated)
    assert actor.qsample_w2h is w2h and [c[0] for c in calls][-2:] == ["w2_pack_f16x3", entry]


def test_vector_loop_hands_the_switch_to_its_actor(monkeypatch):
    """VectorLoop.qsample_f16x3 (read once, when the loop is built) is what qsample_actor() gives the FastActor."""
    from recovery_rl_amd import experiment
    made = []

    class Actor:
        def __init__(self, fast, n):
            self.qsample_f16x3 = False
            made.append(self)

    monkeypatch.setattr(fast_update, "FastActor", Actor)
    for built in (True, False):
        loop = types.SimpleNamespace(_actor=None, agent=types.SimpleNamespace(fast=object()), n=4, cfg=types.SimpleNamespace(seed=5),
                                     qsample_f16x3=built)
        actor = experiment.VectorLoop.qsample_actor(loop)
        assert actor is made[-1] and actor.qsample_f16x3 is built and actor.qsample_seed == 5


# ---- stages ----------------------------------------------------------------------------------------------------------------
def test_build_stages_maps_qsample_f16x3_to_one_packed_stage():
    S = 3
    packed = PackedLoop([types.SimpleNamespace(qsample_hip=True) for _ in range(S)])
    descs = [_desc(n=3 + s, k=1000 - s) for s in range(S)]
    gates = [_gate(n_part=1 + s) for s in range(S)]
    pack = packed.lib.rrl_w2_pack_f16x3
    packed.tapes = [[("call", pack, (2, 256, 0x1000 + s, 0x2000), ()), ("qsample_f16x3", descs[s], gates[s])] for s in range(S)]
    stages = packed._build_stages()
    assert [ops[0][0] for _, _, ops in stages] == ["call", "qsample_f16x3"]
    fn, (calls,), _ = stages[0]
    assert fn == packed._call_each and [c[0] for c in calls] == [pack] * S         # every seed's pack stays a per-seed call
    assert [c[1][2] for c in calls] == [0x1000 + s for s in range(S)]
    fn, args, ops = stages[1]
    assert fn == packed.lib.rrl_qsample_act_f16x3_packed and args[0] == S and len(args) == 3 and len(ops) == S
    assert isinstance(args[1], _lib.rrl_qsample_act_t * S) and isinstance(args[2], _lib.rrl_qsample_gate_t * S)
    assert [(a.n, a.k) for a in args[1]] == [(3 + s, 1000 - s) for s in range(S)] and [g.n_part for g in args[2]] == [1, 2, 3]
    packed.stages = stages
    assert packed.launches == S + 1
    # the f32 kind keeps its entry
    packed.tapes = [[("qsample", descs[s], gates[s])] for s in range(S)]
    assert packed._build_stages()[0][0] == packed.lib.rrl_qsample_act_packed
    # the mask form has no packed stage: the message is the f32 kind's
    messages = []
    for kind in ("qsample", "qsample_f16x3"):
        packed.tapes = [[(kind, descs[s])] for s in range(S)]
        with pytest.raises(_lib.RRLError, match="RRL_PACK_QSAMPLE=1") as err:
            packed._build_stages()
        messages.append(str(err.value))
    assert messages[0] == messages[1]
    # the seed limit is the f32 kind's
    with pytest.raises(ValueError, match="at most 8 seeds"):
        PackedLoop([types.SimpleNamespace(qsample_hip=True, qsample_f16x3=True) for _ in range(9)])


# ---- checkpoints -----------------------------------------------------------------------------------------------------------
class _Reached(Exception):
    pass


def _resume(monkeypatch, written, run_f16x3):
    """load_experiment_state's validation on a checkpoint whose loop state says `written` (None: no key) in a run whose loop
    has qsample_f16x3 = run_f16x3; _Reached: everything was accepted and the first buffer would be overwritten."""
    def reached(*a):
        raise _Reached()
    monkeypatch.setattr(checkpoint, "load_agent_state", reached)
    monkeypatch.setattr(checkpoint, "capacity_fits", lambda sd, cap: True)
    loop = {"qsample_tick": torch.zeros(2, dtype=torch.int64)}
    if written is not None:
        loop["qsample_scoring"] = written
    sd = {"format": checkpoint.FORMAT, "env_name": "navigation1", "env": {"num_envs": 4}, "memory": {}, "recovery_memory": {},
          "agent": {"flat": {}}, "loop": loop}
    exp = types.SimpleNamespace(exp_cfg=types.SimpleNamespace(env_name="navigation1"), env=types.SimpleNamespace(num_envs=4),
                                memory=types.SimpleNamespace(capacity=1), recovery_memory=types.SimpleNamespace(capacity=1),
                                agent=types.SimpleNamespace(fast=object()), recovery_policy=None,
                                loop=types.SimpleNamespace(qsample_hip=True, qsample_f16x3=run_f16x3, sqrl_hip=False))
    checkpoint.load_experiment_state(exp, sd)


def test_resume_refuses_the_other_scoring_in_both_directions(monkeypatch):
    with pytest.raises(ValueError, match=r"written with f16x3 scoring, this run takes f32 scoring \(RRL_QSAMPLE_F16X3=1"):
        _resume(monkeypatch, "f16x3", False)
    with pytest.raises(ValueError, match=r"written with f32 scoring, this run takes f16x3 scoring \(RRL_QSAMPLE_F16X3=1"):
        _resume(monkeypatch, "f32", True)
    with pytest.raises(ValueError, match="written with f32 scoring, this run takes f16x3"):
        _resume(monkeypatch, None, True)                    # an absent key means f32
    for written, run in ((None, False), ("f32", False), ("f16x3", True)):
        with pytest.raises(_Reached):
            _resume(monkeypatch, written, run)


def test_loop_state_records_the_scoring():
    tick, z = torch.zeros(2, dtype=torch.int64), torch.zeros(1)
    for f16x3, want in ((True, "f16x3"), (False, "f32")):
        loop = types.SimpleNamespace(stats=z, reward_sums=z, ep_reward=z, total_numsteps=0, updates=0, host_updates=[0, 0],
                                     num_constraint_violations=0, episode_log=None, qsample_hip=True, qsample_f16x3=f16x3,
                                     sqrl_hip=False, qsample_actor=lambda: types.SimpleNamespace(qsample_tick=tick))
        assert checkpoint.loop_state(loop)["qsample_scoring"] == want
    loop.qsample_hip = False                                # the module path keeps no tick and names no scoring
    assert "qsample_scoring" not in checkpoint.loop_state(loop)


# ---- the fairness of the case table ------------------------------------------------------------------------------------------
def test_case_table_is_the_issues():
    assert len(QC.CASES) == 25 and len(set(QC.CASES)) == 25
    assert {(n, k) for n, k, box in QC.CASES if box == "unit"} == {(n, k) for n in (1, 3, 65) for k in (1, 16, 17, 128, 129, 1000, 1024)}
    for box in ("maze", "asym"):
        assert sorted((n, k) for n, k, b in QC.CASES if b == box) == [(3, 129), (3, 1000)]
    assert SC.FACTOR == 4.0


@pytest.mark.parametrize("n,k,box", QC.CASES)
def test_the_reference_alone_is_inside_the_rules_and_the_bound_is_not_its_floor(n, k, box):
    """The float64 emulation itself satisfies rules Z and Q on every case (so a kernel that computed it exactly would pass),
    and on every case with at least a tile of rows the f32 emulation's deviation is positive: the bound is not the floor alone."""
    c = QC.table_case(n, k, box)
    z64 = c["z"]
    B = SC.bound(z64, c["e32"]["z"])
    d64, d32 = SC.deviation(c["e64"]["z"], z64), SC.deviation(c["e32"]["z"], z64)
    floor = SC.FACTOR * 2.0 ** -23 * float(np.abs(z64).max())
    print("n=%d k=%d %s: bound %.3e (floor %.3e), float64 emulation %.3e, f32 emulation %.3e, scale %.3e"
          % (n, k, box, B, floor, d64, d32, float(np.abs(z64).max())))
    assert d64 <= B
    assert QC.rule_q_holds(c["q"], QC.argmin_first(c["e64"]["q"]), B)
    assert float(np.abs(c["e64"]["q"] - c["q"]).max()) <= B / 4        # the Lipschitz step of rule Q, on the reference
    if k >= 16:
        assert d32 > 0 and B >= floor


# which case sees which mutation (deviation of the mutated f32 emulation above 2 x the case's bound); measured here, asserted below:
#   act_lo_w_hi_dropped, act_hi_w_lo_dropped   every case of the table (the cross products carry 11 of the 22 bits)
#   subnormal_lo_flushed                        every case as drawn -- W2's lo parts (|w| < 1/16) are subnormal f16 values -- so no
#                                               `maze` case had to be scaled
#   no_clamp                                    the saturation case only: nothing else reaches the f16 range
SEEN_BY_ALL = ("act_lo_w_hi_dropped", "act_hi_w_lo_dropped", "subnormal_lo_flushed")


@pytest.mark.parametrize("mutation", SC.MUTATIONS)
def test_each_mutation_breaks_rule_z_on_a_case_of_the_table(mutation):
    seen = []
    for n, k, box in QC.CASES:
        c = QC.table_case(n, k, box)
        dev = SC.deviation(QC.emulate(QC.weights(box), c["obs"], c["cand"], np.float32, mutation)["z"], c["z"])
        if dev > 2 * SC.bound(c["z"], c["e32"]["z"]):
            seen.append((n, k, box))
    sat = QC.saturation_case()
    print("saturation case: %.3f of the layer-1 activations above 65504" % sat["saturated"])
    assert sat["saturated"] > 0
    z64, z32 = sat["z"], sat["e32"]["z"]
    assert np.isfinite(z64).all() and SC.deviation(z32, z64) <= SC.bound(z64, z32) / SC.FACTOR
    dev = SC.deviation(QC.emulate(QC.weights("unit"), sat["obs"], sat["cand"], np.float32, mutation)["z"], z64)
    if dev > 2 * SC.bound(z64, z32):
        seen.append("saturation")
    print(mutation, "seen on", seen)
    assert seen, mutation
    if mutation == "no_clamp":
        assert seen == ["saturation"]
    else:
        assert [s for s in seen if s != "saturation"] == list(QC.CASES)
        assert (3, 129, "maze") in seen and (3, 1000, "maze") in seen
