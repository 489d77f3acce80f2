"""Seed packing for Q-sampling recovery (RRL_PACK_QSAMPLE=1), the parts that need no GPU: the two new symbols, the checks of a
gate and of a packed call before any launch, what run_packed refuses, the launches of the gated acting pass and what they
leave on the tape, and the stage PackedLoop builds from it."""
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
from test_qsample_act_cpu import QS, make_agent

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, ERANGE = -1, -3


# ---- ABI -----------------------------------------------------------------------------------------------------------------
def test_exports_and_declarations():
    for name in ("rrl_qsample_act_gated", "rrl_qsample_act_packed"):
        assert name in _lib.EXPORTS
    src = open(os.path.join(ROOT, "include", "rrl_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"\bint\s+rrl_qsample_act_gated\s*\(\s*const\s+rrl_qsample_act_t\s*\*\s*\w+\s*,\s*const\s+rrl_qsample_gate_t\s*\*", code)
    assert re.search(r"\bint\s+rrl_qsample_act_packed\s*\(\s*int\s+S\s*,\s*const\s+rrl_qsample_act_t\s*\*\s*\w+\s*,\s*const\s+"
                     r"rrl_qsample_gate_t\s*\*", code)
    lib = _lib.load()
    assert lib.rrl_abi_version() == 8                       # additive: nothing existing changed layout
    assert lib.rrl_qsample_act_gated.argtypes[:2] == [C.POINTER(_lib.rrl_qsample_act_t), C.POINTER(_lib.rrl_qsample_gate_t)]
    assert lib.rrl_qsample_act_packed.argtypes[:3] == [C.c_int, C.POINTER(_lib.rrl_qsample_act_t),
                                                       C.POINTER(_lib.rrl_qsample_gate_t)]
    for doc in ("INTEGRATION.md", "README.md", "DESIGN.md"):
        assert "rrl_qsample_act_packed" in open(os.path.join(ROOT, doc)).read(), doc


def test_gate_layout_follows_the_header():
    src = open(os.path.join(ROOT, "include", "rrl_hip.h")).read()
    body = re.search(r"typedef struct \{((?:(?!typedef).)*?)\} rrl_qsample_gate_t;", src, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    want = []
    for decl in filter(None, (d.strip() for d in body.split(";"))):
        base, rest = re.match(r"(?:const\s+)?(long long|\w+)\s*(.*)", decl, flags=re.S).groups()
        name = rest.strip()
        want.append((name.lstrip("* "), C.c_void_p if name.startswith("*") else
                     {"int": C.c_int, "long long": C.c_longlong, "float": C.c_float}[base]))
    assert [(n, t) for n, t in _lib.rrl_qsample_gate_t._fields_] == want


def _desc(**fields):
    d = 0x1000
    a = _lib.rrl_qsample_act_t(n=8, k=1000, H=256, d_obs=2, d_act=2, obs=d, lo=d, hi=d, W1=d, b1=d, W2p=d, b2=d, W3=d, b3=d,
                               scratch=d, action=d)
    for k, v in fields.items():
        setattr(a, k, v)
    return a


def _gate(**fields):
    d = 0x1000
    g = _lib.rrl_qsample_gate_t(z=d, n_part=2, part_stride=16, eps_safe=0.3, task_action=d, ld_task=4, task_out=d, recovery_out=d)
    for k, v in fields.items():
        setattr(g, k, v)
    return g


BAD_GATES = (dict(z=None), dict(task_action=None), dict(recovery_out=None), dict(n_part=0), dict(n_part=5), dict(n_part=-1),
             dict(ld_task=0), dict(ld_task=1), dict(ld_task=3), dict(ld_task=-2))


def test_gate_validation_without_gpu():
    """Every refusal returns before anything is launched (there is no device here to launch on)."""
    lib = _lib.load()
    assert lib.rrl_qsample_act_gated(C.byref(_desc()), None, None) == EINVAL
    assert lib.rrl_qsample_act_gated(None, C.byref(_gate()), None) == EINVAL
    for fields in BAD_GATES:
        assert lib.rrl_qsample_act_gated(C.byref(_desc()), C.byref(_gate(**fields)), None) == EINVAL, fields
    assert lib.rrl_qsample_act_gated(C.byref(_desc(mask=0x1000)), C.byref(_gate()), None) == EINVAL       # both given
    # the descriptor's own checks, same codes; an invalid field wins over a size out of range
    assert lib.rrl_qsample_act_gated(C.byref(_desc(H=32)), C.byref(_gate()), None) == EINVAL
    assert lib.rrl_qsample_act_gated(C.byref(_desc(k=1025)), C.byref(_gate()), None) == ERANGE
    assert lib.rrl_qsample_act_gated(C.byref(_desc(k=1025)), C.byref(_gate(n_part=5)), None) == EINVAL
    assert lib.rrl_qsample_act_gated(C.byref(_desc(k=0, mask=0x1000)), C.byref(_gate()), None) == EINVAL


def test_packed_validation_without_gpu():
    lib = _lib.load()
    arr = lambda typ, items: (typ * len(items))(*items)
    A, G = _lib.rrl_qsample_act_t, _lib.rrl_qsample_gate_t
    good, gates = [_desc() for _ in range(3)], [_gate() for _ in range(3)]
    for S in (0, -1, 17):
        assert lib.rrl_qsample_act_packed(S, arr(A, [_desc()] * 17), arr(G, [_gate()] * 17), None) == EINVAL, S
    assert lib.rrl_qsample_act_packed(3, None, arr(G, gates), None) == EINVAL
    for at in range(3):                                     # one bad seed refuses the call, wherever it sits
        for fields, code in ((dict(k=1025), ERANGE), (dict(H=128), EINVAL), (dict(obs=None), EINVAL), (dict(mask=0x1000), EINVAL)):
            bad = list(good)
            bad[at] = _desc(**fields)
            assert lib.rrl_qsample_act_packed(3, arr(A, bad), arr(G, gates), None) == code, (at, fields)
        for fields in BAD_GATES:
            bad = list(gates)
            bad[at] = _gate(**fields)
            assert lib.rrl_qsample_act_packed(3, arr(A, good), arr(G, bad), None) == EINVAL, (at, fields)
    # without gates a mask is what the stand-alone call takes: only the descriptor's checks apply
    bad = [_desc(mask=0x1000), _desc(mask=0x1000), _desc(mask=0x1000, k=0)]
    assert lib.rrl_qsample_act_packed(3, arr(A, bad), None, None) == ERANGE
    # a seed with more than INT32_MAX / 16 workgroups (n k stays below 2^32)
    n = (2 ** 31 - 1) // 16 // 2 + 1
    assert lib.rrl_qsample_act_packed(2, arr(A, [_desc(), _desc(n=n, k=129)]), arr(G, gates[:2]), None) == ERANGE
    assert lib.rrl_qsample_act_packed(1, arr(A, [_desc(k=2000)]), arr(G, gates[:1]), None) == ERANGE     # S == 1: the gated call
    assert lib.rrl_qsample_act_packed(1, arr(A, [_desc()]), arr(G, [_gate(n_part=5)]), None) == EINVAL


# ---- what run_packed refuses -----------------------------------------------------------------------------------------------
def _packed_cfg(tmp, *more, seeds=2, hidden=256):
    return arg_utils.get_args(["--env-name", "navigation1", "--cuda", "--num_envs", "128", "--seeds_per_gpu", str(seeds),
                               "--hidden_size", str(hidden), "--gamma_safe", "0.8", "--eps_safe", "0.3", "--logdir", str(tmp)]
                              + QS + list(more))


def test_switch_is_opt_in(monkeypatch):
    monkeypatch.delenv("RRL_PACK_QSAMPLE", raising=False)
    assert not fast_update.pack_qsample_enabled()
    monkeypatch.setenv("RRL_PACK_QSAMPLE", "0")
    assert not fast_update.pack_qsample_enabled()
    monkeypatch.setenv("RRL_PACK_QSAMPLE", "1")
    assert fast_update.pack_qsample_enabled()


def test_run_packed_refusal_matrix(monkeypatch, tmp_path):
    monkeypatch.delenv("RRL_W2_FRAG", raising=False)
    # switch off: today's message, with or without the acting kernels
    monkeypatch.delenv("RRL_PACK_QSAMPLE", raising=False)
    for fast in ("1", None):
        monkeypatch.setenv("RRL_FAST_QSAMPLE", "1") if fast else monkeypatch.delenv("RRL_FAST_QSAMPLE")
        with pytest.raises(ValueError, match="model-based recovery and --Q_sampling_recovery run one seed at a time"):
            run_packed(_packed_cfg(tmp_path))
    # switch on: each missing piece alone, by name
    monkeypatch.setenv("RRL_PACK_QSAMPLE", "1")
    monkeypatch.delenv("RRL_FAST_QSAMPLE", raising=False)
    with pytest.raises(ValueError, match="RRL_PACK_QSAMPLE=1 packs --Q_sampling_recovery only with .*set RRL_FAST_QSAMPLE=1"):
        run_packed(_packed_cfg(tmp_path))
    monkeypatch.setenv("RRL_FAST_QSAMPLE", "1")
    with pytest.raises(ValueError, match=r"RRL_PACK_QSAMPLE=1 .*--hidden_size 256 .*got 128"):
        run_packed(_packed_cfg(tmp_path, hidden=128))
    with pytest.raises(ValueError, match="RRL_PACK_QSAMPLE=1 .*without --MF_recovery"):
        run_packed(_packed_cfg(tmp_path, "--MF_recovery"))
    with pytest.raises(ValueError, match=r"RRL_PACK_QSAMPLE=1 .*at most 8 seeds per GPU .*got 9"):
        run_packed(_packed_cfg(tmp_path, seeds=9))
    with pytest.raises(ValueError, match="RRL_PACK_QSAMPLE=1 .*no --no_fast_path"):
        run_packed(_packed_cfg(tmp_path, "--no_fast_path"))
    monkeypatch.setenv("RRL_W2_FRAG", "0")
    with pytest.raises(ValueError, match="RRL_PACK_QSAMPLE=1 .*RRL_W2_FRAG not 0"):
        run_packed(_packed_cfg(tmp_path))
    monkeypatch.delenv("RRL_W2_FRAG")
    # what stays refused with everything in place: env_shard, checkpoints; model-based recovery whatever the switch says
    with pytest.raises(ValueError, match="env_shard"):
        run_packed(_packed_cfg(tmp_path, "--dp_mode", "env_shard"))
    with pytest.raises(ValueError, match="checkpoints"):
        run_packed(_packed_cfg(tmp_path, "--checkpoint_every", "10"))
    mb = _packed_cfg(tmp_path)
    mb.Q_sampling_recovery = False
    with pytest.raises(ValueError, match="model-free recovery policy only"):
        run_packed(mb)
    assert not os.listdir(tmp_path)                         # nothing was written


# ---- the gated acting pass -------------------------------------------------------------------------------------------------
@pytest.fixture
def recorded(monkeypatch):
    """The library's calls recorded (nothing runs), as tests/test_qsample_act_cpu.py does."""
    real, calls = _lib.load(), []

    class Recorder:
        def __getattr__(self, name):
            if name in ("rrl_mlp3_is_split", "rrl_abi_version", "rrl_last_hip_error", "rrl_qsample_scratch_floats"):
                return getattr(real, name)
            return lambda *args: calls.append((name[4:], args)) or 0

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


@pytest.mark.parametrize("fuse_heads", (True, False))
def test_gated_act_qsample_tapes_forward_forward_qsample(recorded, fuse_heads):
    fast, calls = recorded
    fast.fuse_heads = fuse_heads
    n = 128
    actor = fast_update.FastActor(fast, n)
    assert fast.grouped and actor.pol.split and actor.qr.split
    actor.qsample_seed = 77
    obs = torch.zeros(n, 2)
    del calls[:]
    out, tape = _taped(lambda: actor.act_qsample(obs, 0.3, gated=True))
    assert out[0] is actor.task_action and out[1] is actor.real_action and out[2] is actor.recovery
    names = [c[0] for c in calls if c[0] != "w2_pack"]
    middle = [] if fuse_heads else ["policy_heads_fwd_multi"]
    assert names == ["normal_fill", "mlp3_forward_multi"] + middle + ["mlp3_forward_multi", "qsample_act_gated"]
    assert "recovery_select" not in names
    kinds = [op[0] for op in tape]
    assert kinds == ["unsupported", "forward"] + (["heads"] if middle else []) + ["forward", "qsample"]
    assert tape[0][1] == "rrl_normal_fill"                  # the stand-alone pass's own noise fill; in the loop the update's fill
    # the Q_risk forward: one stack on xa, the task head evaluated by the stack when the heads are fused
    stack = tape[-2][1][0]
    assert tape[-2][2] == 1 and stack.x == actor.xa.data_ptr() and bool(stack.use_in_head) == fuse_heads
    _, a, g = tape[-1]
    assert isinstance(a, _lib.rrl_qsample_act_t) and isinstance(g, _lib.rrl_qsample_gate_t)
    assert (a.n, a.k, a.H, a.d_obs, a.d_act) == (n, 1000, 256, 2, 2) and not a.mask
    assert (a.seed, a.counter, a.counter_inc, a.counter_dev) == (77, 0, 1, actor.qsample_tick.data_ptr())
    assert a.obs == obs.data_ptr() and a.action == actor.real_action.data_ptr() and a.W2p == fast.qrisk.w2p.data_ptr()
    assert a.scratch == actor._qsample_scratch.data_ptr() and not (a.cand_in or a.q or a.z or a.cand or a.pick)
    # the gate reads Q_risk's partial last-layer sums and the task action where the stack left it
    z, n_part, ps = actor.qr.parts
    assert z is actor.qr.scratch and n_part == actor.qr.nsplit >= 1 and not actor.qr.finalize
    assert (g.z, g.n_part, g.part_stride) == (z.data_ptr(), n_part, ps)
    assert g.task_action == actor.xa[:, 2:4].data_ptr() == actor.xa.data_ptr() + 8 and g.ld_task == 4
    assert g.task_out == actor.task_action.data_ptr() and g.recovery_out == actor.recovery.data_ptr()
    assert abs(g.eps_safe - 0.3) < 1e-7
    # the library got exactly these two blocks
    last = calls[-1][1]
    assert C.addressof(last[0]._obj) == C.addressof(a) and C.addressof(last[1]._obj) == C.addressof(g)
    # in the loop the noise is the tail of the update's fill: nothing unsupported is left
    fast._actor_noise_fresh = True
    _, tape = _taped(lambda: actor.act_qsample(obs, 0.3, gated=True))
    assert [op[0] for op in tape] == kinds[1:]


def test_without_the_switch_act_qsample_is_todays_six_calls(recorded):
    fast, calls = recorded
    n = 128
    actor = fast_update.FastActor(fast, n)
    obs = torch.zeros(n, 2)
    fast._actor_noise_fresh = False
    del calls[:]
    _, tape = _taped(lambda: actor.act_qsample(obs, 0.3))
    names = [c[0] for c in calls if c[0] not in ("w2_pack", "normal_fill")]
    assert names == ["mlp3_forward", "policy_heads_fwd_multi", "mlp3_forward", "recovery_select", "qsample_act"]
    assert [c[0] for c in calls].count("normal_fill") == 1 and len(names) + 1 == 6
    kinds = [op[0] for op in tape]
    assert kinds.count("unsupported") == 3 and kinds[-1] == "qsample" and len(tape[-1]) == 2      # no gate on the tape
    assert tape[-1][1].mask == actor.recovery.data_ptr()


def test_vector_loop_uses_the_form_it_was_built_with(monkeypatch):
    """VectorLoop.act asks for the gated form when the loop was built under RRL_PACK_QSAMPLE=1 (qsample_gated, read once at
    construction) -- whatever the variable holds later."""
    from recovery_rl_amd.experiment import VectorLoop
    seen = []
    actor = types.SimpleNamespace(act_qsample=lambda obs, eps, gated=False: seen.append(gated) or (1, 2, 3))
    obs = torch.zeros(4, 2)
    for built, later in ((False, "1"), (True, "0"), (True, None)):
        loop = types.SimpleNamespace(cfg=types.SimpleNamespace(eps_safe=0.3), agent=types.SimpleNamespace(fast=object()), n=4,
                                     qsample_hip=True, qsample_gated=built, sqrl_hip=False, qsample_actor=lambda: actor)
        monkeypatch.delenv("RRL_PACK_QSAMPLE", raising=False) if later is None else monkeypatch.setenv("RRL_PACK_QSAMPLE", later)
        assert VectorLoop.act(loop, obs) == (1, 2, 3)
        assert seen[-1] is built


def test_random_phase_draws_its_candidates_from_the_loops_own_generator():
    """The random-action phase of a loop built under the switch: the 1000 candidates per env come from the loop's generator,
    inside the action box, and torch's global generator is not touched -- a packed seed's start does not depend on its
    neighbours."""
    from recovery_rl_amd.experiment import VectorLoop
    n, got = 4, []
    lo, hi = torch.tensor([-1.0, 0.25]), torch.tensor([0.5, 2.0])

    def select_action(obs, candidates=None, eps=None):
        got.append(candidates)
        return torch.zeros(n, 2) if candidates is None else candidates[:, 0]
    qr = types.SimpleNamespace(get_value=lambda obs, a: torch.ones(n, 1), select_action=select_action, policy=None)
    cfg = types.SimpleNamespace(eps_safe=0.3, use_recovery=True, MF_recovery=False, Q_sampling_recovery=True,
                                use_constraint_sampling=False)

    def make(gated, seed):
        rng = torch.Generator().manual_seed(seed)
        return types.SimpleNamespace(cfg=cfg, agent=types.SimpleNamespace(fast=object(), safety_critic=qr), n=n, qsample_hip=True,
                                     qsample_gated=gated, sqrl_hip=False, action_rng=rng, device="cpu",
                                     env=types.SimpleNamespace(sample_actions=lambda generator=None: torch.zeros(n, 2)),
                                     qsample_actor=lambda: types.SimpleNamespace(qsample_box=(lo, hi)))
    obs = torch.zeros(n, 2)
    torch.manual_seed(123)
    before = torch.get_rng_state()
    _, real, rec = VectorLoop.act(make(True, 7), obs, random_actions=True)
    assert torch.equal(torch.get_rng_state(), before)
    cand = got[-1]
    assert cand.shape == (n, 1000, 2) and bool(((cand >= lo) & (cand <= hi)).all()) and bool(rec.all())
    assert torch.equal(real, cand[:, 0])
    VectorLoop.act(make(True, 7), obs, random_actions=True)
    assert torch.equal(got[-1], cand)                       # the loop's seed decides
    VectorLoop.act(make(True, 8), obs, random_actions=True)
    assert not torch.equal(got[-1], cand)
    VectorLoop.act(make(False, 7), obs, random_actions=True)
    assert got[-1] is None                                  # without the switch: select_action's own draw, as before


# ---- stages ----------------------------------------------------------------------------------------------------------------
def test_build_stages_maps_qsample_to_one_packed_stage():
    S = 3
    loops = [types.SimpleNamespace(qsample_hip=True) for _ in range(S)]
    packed = PackedLoop(loops)
    descs = [_desc(n=3 + s, k=1000 - s) for s in range(S)]
    gates = [_gate(n_part=1 + s) for s in range(S)]
    packed.tapes = [[("qsample", descs[s], gates[s])] for s in range(S)]
    stages = packed._build_stages()
    assert len(stages) == 1
    fn, args, ops = stages[0]
    assert fn == packed.lib.rrl_qsample_act_packed and args[0] == S and len(args) == 3 and len(ops) == S
    assert isinstance(args[1], _lib.rrl_qsample_act_t * S) and isinstance(args[2], _lib.rrl_qsample_gate_t * S)
    assert [(a.n, a.k) for a in args[1]] == [(3 + s, 1000 - s) for s in range(S)]
    assert [g.n_part for g in args[2]] == [1, 2, 3]
    packed.stages = stages
    assert packed.launches == 1                              # one entry, as "sqrl"
    # the mask form has no packed stage: the pass in front of it is not on the tape either
    packed.tapes = [[("qsample", descs[s])] for s in range(S)]
    with pytest.raises(_lib.RRLError, match="RRL_PACK_QSAMPLE=1"):
        packed._build_stages()


def test_nine_qsample_loops_are_refused_before_any_net_gives_up_its_w2_copy():
    net = types.SimpleNamespace(w2p=object())
    fast = types.SimpleNamespace(**{name: net for name in fast_update.FLAT_NETS})
    loop = types.SimpleNamespace(qsample_hip=True, agent=types.SimpleNamespace(fast=fast))
    with pytest.raises(ValueError, match=r"rrl_qsample_act_packed\) packs at most 8 seeds"):
        PackedLoop([loop] * 9)
    assert net.w2p is not None
    assert PackedLoop([loop] * 8).S == 8
