"""What the acting passes of the SQRL and Q-sampling lines record and call, in order, in each of their six forms, and the packed
entry each of the four tape kinds becomes (no GPU: the library's calls are recorded, nothing runs).  The lists are read off the
code as it stood before FastActor's launch tails and PackedLoop's stage branches were folded into fast_update.ACT_ENTRIES."""
import pytest
import torch

from recovery_rl_amd import _lib, fast_update, packed
from test_sqrl_act_cpu import make_agent

N = 128


@pytest.fixture
def recorded(monkeypatch):
    """A FastUpdater on the CPU and the list every library call AND every tape record is appended to, in order."""
    real, events = _lib.load(), []

    class Recorder:
        def __getattr__(self, name):
            if name in ("rrl_mlp3_is_split", "rrl_abi_version", "rrl_last_hip_error", "rrl_qsample_scratch_floats"):
                return getattr(real, name)
            fn = lambda *args: events.append(("call", name)) or 0
            fn.__name__ = name
            return fn

    monkeypatch.setattr(_lib, "_lib", Recorder())
    monkeypatch.setattr(_lib, "current_stream", lambda: 0)
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: False)
    fast = make_agent("cpu").enable_fast_path(256)
    for net in (fast.qrisk, fast.policy):                   # (a CPU FlatNet keeps no fragment-order copy)
        net.w2p = torch.empty(net.p["W2"].numel())
    return fast, events


def _run(fast, events, line, gated, f16x3):
    """-> (the interleaved sequence of ("tape", kind) and ("call", entry), the tape)"""
    actor = fast_update.FastActor(fast, N)
    setattr(actor, line + "_f16x3", f16x3)
    real = fast_update.record
    tape = []
    fast_update.set_tape(tape)
    fast_update.record = lambda kind, *p: (events.append(("tape", kind)), real(kind, *p))[1]
    del events[:]
    try:
        if line == "sqrl":
            actor.act_sqrl(torch.zeros(N, 2), 0.3)
        else:
            actor.act_qsample(torch.zeros(N, 2), 0.3, gated=gated)
    finally:
        fast_update.record = real
        fast_update.set_tape(None)
    return list(events), tape


def _launch(kind, entry):
    return [("tape", kind), ("call", entry)]


W2 = [("call", "rrl_w2_pack")]                           # a fragment-order W2 copy made current (eager: before every use)
FORWARD = W2 + _launch("forward", "rrl_mlp3_forward_multi")
NOISE = _launch("unsupported", "rrl_normal_fill")
EAGER_FORWARD = _launch("unsupported", "rrl_mlp3_forward")
PACK = _launch("call", "rrl_w2_pack_f16x3")
# what precedes the acting launch: SQRL -- Q_risk's W2 copy, the task policy's forward; Q-sampling with the mask -- act_gate's
# eager forwards, head launch and select; with the gate in the launch -- the task policy's forward and Q_risk's, the task head
# evaluated by the stack, both of a kind the tape packs
HEADS = {
    ("sqrl", False): W2 + FORWARD,
    ("qsample", False): W2 + NOISE + EAGER_FORWARD + _launch("heads", "rrl_policy_heads_fwd_multi") + EAGER_FORWARD
    + [("call", "rrl_recovery_select")],
    ("qsample", True): W2 + NOISE + FORWARD + FORWARD,
}
# the acting launch itself, behind its pack call where it scores in f16x3
TAILS = {
    ("sqrl", False, False): _launch("sqrl", "rrl_sqrl_act"),
    ("sqrl", False, True): PACK + _launch("sqrl_f16x3", "rrl_sqrl_act_f16x3"),
    ("qsample", False, False): _launch("qsample", "rrl_qsample_act"),
    ("qsample", False, True): PACK + _launch("qsample_f16x3", "rrl_qsample_act_f16x3"),
    ("qsample", True, False): _launch("qsample", "rrl_qsample_act_gated"),
    ("qsample", True, True): PACK + _launch("qsample_f16x3", "rrl_qsample_act_gated_f16x3"),
}


@pytest.mark.parametrize("line,gated,f16x3", sorted(TAILS))
def test_the_sequence_of_tape_records_and_library_calls(recorded, line, gated, f16x3):
    fast, events = recorded
    seq, tape = _run(fast, events, line, gated, f16x3)
    assert seq == HEADS[line, gated] + TAILS[line, gated, f16x3]
    # the blocks the acting launch was recorded with: the descriptor, and the gate where it is in the launch
    assert len(tape[-1]) == (3 if gated else 2)
    assert isinstance(tape[-1][1], _lib.rrl_sqrl_act_t if line == "sqrl" else _lib.rrl_qsample_act_t)
    if gated:
        assert isinstance(tape[-1][2], _lib.rrl_qsample_gate_t)
    if f16x3:
        assert tape[-2][0] == "call" and tape[-2][1].__name__ == "rrl_w2_pack_f16x3" and len(tape[-2]) == 4


def test_the_table_is_the_six_forms_and_the_four_kinds():
    assert set(fast_update.ACT_ENTRIES) == set(TAILS)
    for form, (kind, entry) in fast_update.ACT_ENTRIES.items():
        assert TAILS[form][-2:] == _launch(kind, entry), form
    assert fast_update.ACT_PACKED == {"sqrl": "rrl_sqrl_act_packed", "sqrl_f16x3": "rrl_sqrl_act_f16x3_packed",
                                      "qsample": "rrl_qsample_act_packed", "qsample_f16x3": "rrl_qsample_act_f16x3_packed"}


@pytest.mark.parametrize("kind,entry,blocks", [
    ("sqrl", "rrl_sqrl_act_packed", (_lib.rrl_sqrl_act_t,)),
    ("sqrl_f16x3", "rrl_sqrl_act_f16x3_packed", (_lib.rrl_sqrl_act_t,)),
    ("qsample", "rrl_qsample_act_packed", (_lib.rrl_qsample_act_t, _lib.rrl_qsample_gate_t)),
    ("qsample_f16x3", "rrl_qsample_act_f16x3_packed", (_lib.rrl_qsample_act_t, _lib.rrl_qsample_gate_t)),
])
def test_the_packed_stage_of_each_kind(kind, entry, blocks):
    S = 3
    loop = packed.PackedLoop.__new__(packed.PackedLoop)
    loop.S, loop.lib = S, _lib.load()
    loop.tapes = [[(kind,) + tuple(t(n=5 + s) if t is not _lib.rrl_qsample_gate_t else t(n_part=1 + s) for t in blocks)]
                  for s in range(S)]
    (fn, args, ops), = loop._build_stages()
    assert fn == getattr(loop.lib, entry) and fn.__name__ == entry
    assert args[0] == S and len(args) == 1 + len(blocks) and len(ops) == S
    for arr, t in zip(args[1:], blocks):
        assert isinstance(arr, t * S)
    assert [a.n for a in args[1]] == [5, 6, 7]
    if len(blocks) == 2:
        assert [g.n_part for g in args[2]] == [1, 2, 3]
    else:
        return
    # the mask form of the Q-sampling call has no packed stage
    loop.tapes = [[(kind, blocks[0](n=5))] for s in range(S)]
    with pytest.raises(_lib.RRLError, match=r"launch kind 'qsample' packs with the gate in the launch only \(RRL_PACK_QSAMPLE=1\)"):
        loop._build_stages()
