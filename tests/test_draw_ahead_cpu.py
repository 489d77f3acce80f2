"""Host-side validity rules of keys drawn ahead (replay_memory.DrawAhead) and the ABI of the two entry points: no device."""
import ctypes as C

from recovery_rl_amd import _lib
from recovery_rl_amd.replay_memory import DrawAhead


def test_keys_are_usable_after_exactly_the_step_they_were_drawn_for():
    a = DrawAhead()
    assert not a.ready(256) and not a.take(256)
    a.selected(256, 4096)
    assert not a.ready(256)                       # the step has not pushed its rows yet
    a.stepped(4096)
    assert a.ready(256) and not a.ready(128)      # ... for the batch size they were drawn for only
    assert a.take(256) and a.pending is None and not a.take(256)


def test_anything_else_drops_them():
    a = DrawAhead()
    a.selected(256, 4096)
    a.stepped(64)                                 # another number of rows than they were drawn for (num_envs changed)
    assert a.pending is None
    a.selected(256, 4096)
    a.stepped(4096)
    a.stepped(4096)                               # a second step before the draw
    assert a.pending is None
    a.selected(256, 4096)
    a.stepped(4096)
    a.drop()                                      # eager push / sample / draw, checkpoint load
    assert not a.ready(256)
    a.stepped(4096)                               # a step without a selection
    assert a.pending is None
    a.selected(256, 4096)
    a.stepped(4096)
    assert not a.take(128) and a.pending is None  # a draw of another size consumes the tick: the keys are gone


def test_entry_points_validate_before_any_launch():
    lib = _lib.load()
    assert lib.rrl_draw_select(None, None) == -1
    assert lib.rrl_mlp3_forward_riders(None, None, None) == -1
    sel = _lib.rrl_draw_ahead_t(None, 0, None)
    assert lib.rrl_draw_select(C.byref(sel), None) == -1
    assert C.sizeof(_lib.rrl_draw_ahead_t) == 24 and _lib.AHEAD_META == 8


def test_rider_hosts_keep_the_forward_kernels_budget(tmp_path):
    """The forward that hosts the rider workgroups stays at four waves per SIMD (<= 128 VGPRs) without scratch, like the
    forward kernels it stands beside: a host that paid for its riders with occupancy or spills would be the wrong host."""
    import os
    from isa_util import kernel_table
    if not os.path.exists(_lib.SO_PATH):
        _lib.build()
    table = {k: v for k, v in kernel_table(_lib.SO_PATH, str(tmp_path)).items() if "vgpr" in v}
    hosts = {k: v for k, v in table.items() if "mlp3_fwd_split_riders_kernel" in k}
    assert len(hosts) == 2
    for k, v in hosts.items():
        assert v["vgpr"] <= 128 and v["scratch"] == 0, (k, v)
