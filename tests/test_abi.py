"""CPU suite: the C-ABI library builds for gfx950, loads, and exports every symbol that
include/rrl_hip.h declares.  No compute calls (no GPU here)."""
import ctypes
import os
import re

from recovery_rl_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared():
    src = open(os.path.join(ROOT, "include", "rrl_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(rrl_[a-z0-9_]+)\s*\(", src)))


def test_library_builds_and_exports_every_declared_symbol():
    _lib.build()
    assert os.path.exists(_lib.SO_PATH)
    lib = ctypes.CDLL(_lib.SO_PATH)
    names = _declared()
    assert len(names) >= 10
    for name in names:
        assert hasattr(lib, name), name
    assert sorted(_lib.EXPORTS) == names


def test_loader_declares_signatures_and_abi_version():
    lib = _lib.load()
    assert lib.rrl_abi_version() >= 1
    assert lib.rrl_nav_offline_rollouts(0, 20000) == 2000
    assert lib.rrl_nav_offline_rollouts(1, 20000) == 666 + 4 * 500
    assert lib.rrl_nav_offline_rollouts(7, 10) < 0            # unknown env kind -> error code


def test_argument_validation_without_gpu():
    lib = _lib.load()
    # null pointers / bad kinds are rejected before any launch
    assert lib.rrl_nav_step(9, 4, None, None, None, 0, 0, None, 0, None, None, None, None, None, None,
                            None, None, 100, 0, None) == -1
    assert lib.rrl_nav_step(0, 4, None, None, None, 0, 0, None, 0, None, None, None, None, None, None,
                            None, None, 100, 0, None) == -1
    assert lib.rrl_counter_add(None, 1, None) == -1


def _step_push_struct(gate=False, log=False, **fields):
    """A well-formed rrl_step_push_t whose device pointers are dummy non-null integers (validation never follows them; the
    two ring descriptions and the head description are host structs and real), then `fields` on top."""
    d = 0x1000
    a = _lib.rrl_step_push_t()
    a.n, a.pos, a.t, a.obs, a.task_action, a.ld_task, a.real_action, a.recovery = 8, d, d, d, d, 2, d, d
    a.horizon, a.auto_reset, a.stats, a.reward_sums, a.ep_reward = 100, 1, d, d, d
    a.memory = ctypes.pointer(_lib.rrl_replay_t(s=d, a=d, r=d, s2=d, m=d, cap=100, state=d))
    a.recovery_memory = ctypes.pointer(_lib.rrl_replay_t(s=d, a=d, r=d, s2=d, m=d, cap=100, state=d, pos_cnt=d))
    if gate:
        a.sel_z, a.sel_n_part, a.sel_part_stride, a.sel_eps_safe, a.sel_rec_action = d, 1, 0, 0.3, d
        a.real_action_out, a.recovery_out = d, d
    if log:
        a.log_rec_i32, a.log_rec_f64, a.log_cap, a.log_state = d, d, 64, d
        a.log_len, a.log_ret, a.log_viol, a.log_rec = d, d, d, d
    for k, v in fields.items():
        setattr(a, k, v)
    return a


def _stoch_head(**fields):
    d = 0x1000
    h = _lib.rrl_policy_head_t(kind=_lib.HEAD_STOCH, B=8, head=d, n_part=1, scale=d, bias=d, log_std=d)
    for k, v in fields.items():
        setattr(h, k, v)
    return ctypes.pointer(h)


def _ring(cap, pinned):
    d = 0x1000
    return ctypes.pointer(_lib.rrl_replay_t(s=d, a=d, r=d, s2=d, m=d, cap=cap, state=d, pinned=pinned))


def test_step_push_struct_validation_without_gpu():
    """What rrl_nav_step_push_x / rrl_maze_step_push_x (and the packed entry points with one seed, which forward to them)
    answer to a malformed rrl_step_push_t: every call returns before any launch.  The codes, and which of RRL_ERANGE /
    RRL_EINVAL wins when several things are wrong (sizes of n and of the status word's horizon, then required fields, then
    the gate, then the rings, then the episode log), are those of ABI version 4, recorded from that library."""
    lib = _lib.load()
    OK, EINVAL, ERANGE = 0, -1, -3
    S = _step_push_struct
    table = [
        ("NULL struct", None, EINVAL),
        ("n < 0", S(n=-1), ERANGE),
        ("n > 2^32 - 1", S(n=1 << 32), ERANGE),
        ("pos missing", S(pos=None), EINVAL),
        ("obs missing", S(obs=None), EINVAL),
        ("task_action missing", S(task_action=None), EINVAL),
        ("memory missing", S(memory=None), EINVAL),
        ("stats missing", S(stats=None), EINVAL),
        ("reward_sums missing", S(reward_sums=None), EINVAL),
        ("ep_reward missing", S(ep_reward=None), EINVAL),
        ("neither t nor status", S(t=None), EINVAL),
        ("status, horizon 0", S(status=0x1000, horizon=0), ERANGE),
        ("status, horizon 4096", S(status=0x1000, horizon=4096), ERANGE),
        ("status without t, horizon 4096", S(t=None, status=0x1000, horizon=4096), ERANGE),
        ("ld_task odd", S(ld_task=3), EINVAL),
        ("ld_task 1", S(ld_task=1), EINVAL),
        ("ld_task 0", S(ld_task=0), EINVAL),
        ("real_action missing, no gate", S(real_action=None), EINVAL),
        ("gate, real_action_out missing", S(gate=True, real_action_out=None), EINVAL),
        ("gate, recovery_out missing", S(gate=True, recovery_out=None), EINVAL),
        ("gate, sel_n_part 0", S(gate=True, sel_n_part=0), EINVAL),
        ("gate, sel_n_part 5", S(gate=True, sel_n_part=5), EINVAL),
        ("gate, neither sel_rec_action nor sel_rec_head", S(gate=True, sel_rec_action=None), EINVAL),
        ("gate, sel_rec_head of the wrong kind", S(gate=True, sel_rec_action=None,
                                                   sel_rec_head=_stoch_head(kind=_lib.HEAD_GAUSS)), EINVAL),
        ("gate, sel_rec_head without log_std", S(gate=True, sel_rec_action=None, sel_rec_head=_stoch_head(log_std=None)), EINVAL),
        ("gate, sel_rec_head with n_part 5", S(gate=True, sel_rec_action=None, sel_rec_head=_stoch_head(n_part=5)), EINVAL),
        ("n > cap - pinned of memory", S(memory=_ring(100, 93)), ERANGE),
        ("n > cap - pinned of recovery_memory", S(recovery_memory=_ring(7, 0)), ERANGE),
        ("pinned < 0 in memory", S(memory=_ring(100, -1)), ERANGE),
        ("pinned < 0 in recovery_memory", S(recovery_memory=_ring(100, -1)), ERANGE),
        ("log_state, log_rec_i32 missing", S(log=True, log_rec_i32=None), EINVAL),
        ("log_state, log_rec_f64 missing", S(log=True, log_rec_f64=None), EINVAL),
        ("log_state, log_cap 0", S(log=True, log_cap=0), EINVAL),
        ("log_state, log_len missing", S(log=True, log_len=None), EINVAL),
        ("log_state, log_ret missing", S(log=True, log_ret=None), EINVAL),
        ("log_state, log_viol missing", S(log=True, log_viol=None), EINVAL),
        ("log_state, log_rec missing", S(log=True, log_rec=None), EINVAL),
        # several things wrong: the first check in the order above answers
        ("n < 0 and pos missing", S(n=-1, pos=None), ERANGE),
        ("horizon 0 with status and pos missing", S(status=0x1000, horizon=0, pos=None), ERANGE),
        ("pos missing and ring too small", S(pos=None, memory=_ring(4, 0)), EINVAL),
        ("gate incomplete and ring too small", S(gate=True, sel_n_part=0, memory=_ring(4, 0)), EINVAL),
        ("ring too small and log companion missing", S(log=True, log_len=None, memory=_ring(4, 0)), ERANGE),
        ("n == 0 does not excuse a missing field", S(n=0, pos=None), EINVAL),
        # n == 0 with everything valid: nothing to do, no launch
        ("n == 0", S(n=0), OK),
        ("n == 0, status instead of t", S(n=0, t=None, status=0x1000, horizon=4095), OK),
        ("n == 0, gate with a recovery action", S(n=0, gate=True), OK),
        ("n == 0, gate with a recovery head", S(n=0, gate=True, sel_rec_action=None, sel_rec_head=_stoch_head()), OK),
        ("n == 0, episode log", S(n=0, log=True), OK),
        ("n == 0, no recovery_memory", S(n=0, recovery_memory=None), OK),
    ]
    for what, a, want in table:
        assert want != OK or a.n == 0, what          # only an empty step may pass: nothing here reaches a launch
        arg = None if a is None else ctypes.byref(a)
        for kind in (0, 1):                         # RRL_ENV_NAV1, RRL_ENV_NAV2
            assert lib.rrl_nav_step_push_x(kind, arg, None) == want, ("nav", kind, what)
            assert lib.rrl_nav_step_push_packed(1, kind, arg, None) == want, ("nav packed", kind, what)
        assert lib.rrl_maze_step_push_x(arg, None) == want, ("maze", what)
        assert lib.rrl_maze_step_push_packed(1, arg, None) == want, ("maze packed", what)
    # the env kind is looked at before the struct
    for kind in (-1, 2, 9):
        assert lib.rrl_nav_step_push_x(kind, ctypes.byref(S(n=0)), None) == EINVAL
        assert lib.rrl_nav_step_push_x(kind, ctypes.byref(S(n=-1)), None) == EINVAL
        assert lib.rrl_nav_step_push_packed(1, kind, ctypes.byref(S(n=0)), None) == EINVAL


def _with(struct, **fields):
    """`struct` with `fields` on top; a dotted name reaches into a nested struct (loss__kind -> .loss.kind)."""
    for k, v in fields.items():
        obj, names = struct, k.split("__")
        for name in names[:-1]:
            obj = getattr(obj, name)
        setattr(obj, names[-1], v)
    return struct


def _head_bwd(**fields):
    """A well-formed rrl_head_bwd_t on a plain dOut tensor (loss.kind = -1); device pointers are dummy non-null integers."""
    d = 0x1000
    loss = _lib.rrl_loss_t(kind=-1, n_part=1, out=d)
    return _with(_lib.rrl_head_bwd_t(loss, 2, 64, 32, 1, d, d, d, d, d), **fields)


def _gauss_head_bwd(**fields):
    """The same with the loss description of a tanh-Gaussian policy head (one head, four outputs)."""
    d = 0x1000
    loss = _lib.rrl_loss_t(kind=_lib.LOSS_GAUSS_HEAD, n_part=1, out=d, v0=d, v1=d, d_action=d, ld=4, n_heads=2)
    return _with(_lib.rrl_head_bwd_t(loss, 1, 64, 32, 4, d, d, d, d, d), **fields)


def _hidden_bwd(**fields):
    d = 0x1000
    return _with(_lib.rrl_hidden_bwd_t(2, 64, 32, d, d, d, d, d, d, _lib.rrl_first_layer_t()), **fields)


def _input_bwd(**fields):
    d = 0x1000
    return _with(_lib.rrl_input_bwd_t(2, 64, 32, 4, 4, d, d, d, d, d, d), **fields)


def _adam_seg(**fields):
    d = 0x1000
    return _with(_lib.rrl_adam_seg_t(n=1 << 17, p=d, g=d, m=d, v=d, step_dev=d), **fields)


def test_backward_and_adam_descriptor_validation_without_gpu():
    """What the descriptor entry points of the stack backward and of the optimiser step (and the packed ones with one seed,
    which forward to them) answer to a malformed descriptor: every call returns before any launch.  The codes are those
    of ABI version 5, recorded from that library (where the positional forms still stood beside these).
    Every case is rejected whatever else the descriptor holds, so nothing here can reach a launch on a machine with a GPU.
    The partial-gradient count of an Adam segment is bounded by 64, not by the 4 of a stack output's partial sums: n_part
    = 5 is rejected below for its companion fields (part_elems = 0) and is valid with them, 65 is never valid."""
    lib = _lib.load()
    EINVAL, ERANGE = -1, -3
    d = 0x1000
    first = lambda **f: _with(_lib.rrl_first_layer_t(x=d, W1=d, ldx=4, din=4, first_part=d, first_stride=512, dx_part=d), **f)
    heads = [
        ("h2 missing", _head_bwd(h2=None), EINVAL),
        ("W3 missing", _head_bwd(W3=None), EINVAL),
        ("loss.out (dOut) missing", _head_bwd(loss__out=None), EINVAL),
        ("B 1025", _head_bwd(B=1025), ERANGE),
        ("B 0", _head_bwd(B=0), ERANGE),
        ("dout 5", _head_bwd(dout=5), ERANGE),
        ("loss kind 7", _head_bwd(loss__kind=7), ERANGE),
        ("loss kind -2", _head_bwd(loss__kind=-2), ERANGE),
        ("loss n_part 5", _gauss_head_bwd(loss__n_part=5), ERANGE),
        ("loss n_part 0", _gauss_head_bwd(loss__n_part=0), ERANGE),
        ("G, dout not the loss kind's", _gauss_head_bwd(G=2), EINVAL),
        ("da_group 2", _gauss_head_bwd(loss__da_group=2), ERANGE),
        ("da_group 4 with da_parts 6", _gauss_head_bwd(loss__da_group=4, loss__da_parts=6), ERANGE),
        ("da_parts 17", _gauss_head_bwd(loss__da_parts=17), ERANGE),
        # several things wrong: pointers before sizes, sizes before the loss description
        ("h2 missing and B 1025", _head_bwd(h2=None, B=1025), EINVAL),
        ("B 1025 and loss kind 7", _head_bwd(B=1025, loss__kind=7), ERANGE),
        ("loss kind 7 and the wrong G", _gauss_head_bwd(loss__kind=7, G=2), ERANGE),
    ]
    hidden = [
        ("dh2 (the link to the head stage) missing", _hidden_bwd(dh2=None), EINVAL),
        ("h1 missing", _hidden_bwd(h1=None), EINVAL),
        ("W2 missing", _hidden_bwd(W2=None), EINVAL),
        ("dW2 without db2", _hidden_bwd(db2=None), EINVAL),
        ("db2 without dW2", _hidden_bwd(dW2=None), EINVAL),
        ("G 65536", _hidden_bwd(G=65536), ERANGE),
        ("B 0", _hidden_bwd(B=0), ERANGE),
        ("dh1 missing without first", _hidden_bwd(dh1=None), EINVAL),
        ("first.x with din 5", _hidden_bwd(B=128, H=128, first=first(din=5)), EINVAL),
        ("first.x with din 0", _hidden_bwd(B=128, H=128, first=first(din=0)), EINVAL),
        ("first.x without W1", _hidden_bwd(B=128, H=128, first=first(W1=None)), EINVAL),
        ("first.x with neither first_part nor dx_part", _hidden_bwd(B=128, H=128, first=first(first_part=None, dx_part=None)),
         EINVAL),
        ("first.x on ragged tiles", _hidden_bwd(first=first()), ERANGE),
        ("first.x on unaligned dh2", _hidden_bwd(B=128, H=128, dh2=d + 4, first=first()), ERANGE),
        ("dh2 missing and G 65536", _hidden_bwd(dh2=None, G=65536), EINVAL),
    ]
    inputs = [
        ("dh1 missing", _input_bwd(dh1=None), EINVAL),
        ("x missing", _input_bwd(x=None), EINVAL),
        ("W1 missing", _input_bwd(W1=None), EINVAL),
        ("din 5", _input_bwd(din=5), ERANGE),
        ("din 0", _input_bwd(din=0), ERANGE),
        ("x missing and din 5", _input_bwd(x=None, din=5), EINVAL),
    ]
    one = ctypes.c_int * 1
    ptrs = lambda T, arr: (ctypes.POINTER(T) * 1)(ctypes.cast(arr, ctypes.POINTER(T)))

    def arr(T, x):
        a = (T * 5)()                # five slots: a count of 5 is refused before any member is read, but stays in bounds
        a[0] = x
        return a

    H, D, I, A = _lib.rrl_head_bwd_t, _lib.rrl_hidden_bwd_t, _lib.rrl_input_bwd_t, _lib.rrl_adam_seg_t
    good_h, good_d = arr(H, _head_bwd()), arr(D, _hidden_bwd())
    for what, x, want in heads:
        a = arr(H, x)
        assert lib.rrl_mlp_head_backward_multi(1, a, None) == want, ("head", what)
        assert lib.rrl_mlp_backward_pair_multi(1, a, good_d, None) == want, ("pair", what)
        assert lib.rrl_mlp_head_backward_multi_packed(1, one(1), ptrs(H, a), None) == want, ("head packed", what)
        assert lib.rrl_mlp_backward_pair_multi_packed(1, one(1), ptrs(H, a), ptrs(D, good_d), None) == want, ("pair packed", what)
    for what, x, want in hidden:
        a = arr(D, x)
        assert lib.rrl_mlp_hidden_backward_multi(1, a, None) == want, ("hidden", what)
        assert lib.rrl_mlp_backward_pair_multi(1, good_h, a, None) == want, ("pair", what)
        assert lib.rrl_mlp_hidden_backward_multi_packed(1, one(1), ptrs(D, a), None) == want, ("hidden packed", what)
        assert lib.rrl_mlp_backward_pair_multi_packed(1, one(1), ptrs(H, good_h), ptrs(D, a), None) == want, ("pair packed", what)
    for what, x, want in inputs:
        assert lib.rrl_mlp_input_backward_multi(1, arr(I, x), None) == want, ("input", what)
    # the head stage answers before the hidden stage
    assert lib.rrl_mlp_backward_pair_multi(1, arr(H, _head_bwd(B=1025)), arr(D, _hidden_bwd(dh2=None)), None) == ERANGE
    # the member count is looked at before any member: 1 .. 4
    good_i = arr(I, _input_bwd())
    for n in (0, 5, -1):
        assert lib.rrl_mlp_head_backward_multi(n, good_h, None) == EINVAL
        assert lib.rrl_mlp_hidden_backward_multi(n, good_d, None) == EINVAL
        assert lib.rrl_mlp_input_backward_multi(n, good_i, None) == EINVAL
        assert lib.rrl_mlp_backward_pair_multi(n, good_h, good_d, None) == EINVAL
        assert lib.rrl_mlp_head_backward_multi_packed(1, one(n), ptrs(H, good_h), None) == EINVAL
        assert lib.rrl_mlp_hidden_backward_multi_packed(1, one(n), ptrs(D, good_d), None) == EINVAL
        assert lib.rrl_mlp_backward_pair_multi_packed(1, one(n), ptrs(H, good_h), ptrs(D, good_d), None) == EINVAL
    for fn in (lib.rrl_mlp_head_backward_multi, lib.rrl_mlp_hidden_backward_multi, lib.rrl_mlp_input_backward_multi):
        assert fn(1, None, None) == EINVAL
    assert lib.rrl_mlp_backward_pair_multi(1, None, good_d, None) == EINVAL
    assert lib.rrl_mlp_backward_pair_multi(1, good_h, None, None) == EINVAL

    part = dict(g_part=d, n_part=4, part_stride=512, part_elems=256)
    w2 = dict(w2p=d, target=d, target_w2p=d, w2_off=0, w2_heads=2)
    segs = [
        ("p missing", _adam_seg(p=None)),
        ("g missing", _adam_seg(g=None)),
        ("m missing", _adam_seg(m=None)),
        ("v missing", _adam_seg(v=None)),
        ("step_dev missing", _adam_seg(step_dev=None)),
        ("n 0", _adam_seg(n=0)),
        ("g_part with n_part 5 and no part_elems", _adam_seg(g_part=d, n_part=5)),
        ("g_part with n_part 0", _adam_seg(**dict(part, n_part=0))),
        ("g_part with n_part 65", _adam_seg(**dict(part, n_part=65))),
        ("g_part with part_elems 0", _adam_seg(**dict(part, part_elems=0))),
        ("g_part with part_elems > n", _adam_seg(**dict(part, part_elems=1 << 18))),
        ("g_part with part_elems 6", _adam_seg(**dict(part, part_elems=6))),
        ("g_part with part_stride 510", _adam_seg(**dict(part, part_stride=510))),
        ("g_part unaligned", _adam_seg(**dict(part, g_part=d + 4))),
        ("w2p unaligned", _adam_seg(**dict(w2, w2p=d + 4))),
        ("target_w2p unaligned", _adam_seg(**dict(w2, target_w2p=d + 8))),
        ("w2p with unaligned parameters", _adam_seg(**dict(w2, p=d + 4))),
        ("w2p with w2_off 2", _adam_seg(**dict(w2, w2_off=2))),
        ("w2p with w2_heads 0", _adam_seg(**dict(w2, w2_heads=0))),
        ("w2p past the end of the segment", _adam_seg(**dict(w2, w2_heads=3))),
    ]
    lr = (ctypes.c_float * 1)(3e-4)
    dual = (_lib.rrl_dual_t * 1)(_lib.rrl_dual_t(stat=d, loss_in=d, loss_out=d))
    for what, x in segs:
        a = (A * 1)(x)
        assert lib.rrl_adam_step_multi(1, a, 3e-4, 0.9, 0.999, 1e-8, None) == EINVAL, ("adam", what)
        assert lib.rrl_adam_step_multi_duals(1, a, 1, dual, 3e-4, 0.9, 0.999, 1e-8, None) == EINVAL, ("adam duals", what)
        assert lib.rrl_adam_step_multi_packed(1, one(1), ptrs(A, a), lr, 0.9, 0.999, 1e-8, None) == EINVAL, ("adam packed", what)
    good = (A * 1)(_adam_seg())
    for n in (0, 13, -1):                       # 1 .. RRL_ADAM_MAX_SEGS
        assert lib.rrl_adam_step_multi(n, good, 3e-4, 0.9, 0.999, 1e-8, None) == EINVAL
        assert lib.rrl_adam_step_multi_packed(1, one(n), ptrs(A, good), lr, 0.9, 0.999, 1e-8, None) == EINVAL
    assert lib.rrl_adam_step_multi(1, None, 3e-4, 0.9, 0.999, 1e-8, None) == EINVAL


def _draw(ring=None, **fields):
    """A well-formed uniform rrl_draw_t of 64 rows on a 4096-row ring; device pointers are dummy non-null integers.  `ring`:
    fields of the rrl_replay_t on top (the ring is a host struct and real)."""
    d = 0x1000
    rb = _with(_lib.rrl_replay_t(s=d, a=d, r=d, s2=d, m=d, cap=4096, state=d, pos_cnt=d), **(ring or {}))
    draw = _lib.rrl_draw_t(ctypes.pointer(rb), _lib.DRAW_UNIFORM, 0, 64, 1, 0, d, 1, d, d, d, d, d, d, None, None, None)
    return _with(draw, **fields)


def _head(kind=_lib.HEAD_GAUSS, **fields):
    d = 0x1000
    h = _lib.rrl_policy_head_t(kind=kind, B=8, head=d, n_part=1, eps=d, scale=d, bias=d, action=d, ld_action=2, log_std=d)
    return _with(h, **fields)


def test_draw_and_policy_head_descriptor_validation_without_gpu():
    """What rrl_sample_multi, rrl_draw_select and rrl_policy_heads_fwd_multi (and rrl_sample_multi_packed with one seed,
    which forwards) answer to a malformed rrl_draw_t / rrl_policy_head_t: every call returns before any launch.  The codes
    are those of ABI version 6, recorded from that library (where the positional forms still stood beside these).  Order
    for a draw: the noise arguments of the launch, then per draw the ring and the outputs, the batch size, the mode's own
    bounds.  No case is well formed, so nothing here can reach a launch on a machine with a GPU: the valid capacity bound
    of the stratified mode is shown by a second draw that is refused for another reason with another code."""
    lib = _lib.load()
    EINVAL, ERANGE = -1, -3
    U, ST, DEMO = _lib.DRAW_UNIFORM, _lib.DRAW_STRATIFIED, _lib.DRAW_DEMO_SHARE
    d = 0x1000
    draws = [
        ("ring missing", _draw(rb=None), EINVAL),
        ("ring without state", _draw(ring=dict(state=None)), EINVAL),
        ("ring without rewards", _draw(ring=dict(r=None)), EINVAL),
        ("ring with cap 0", _draw(ring=dict(cap=0)), EINVAL),
        ("output s2 missing", _draw(s2=None), EINVAL),
        ("output m missing", _draw(m=None), EINVAL),
        ("n_pos < 0", _draw(n_pos=-1, n_neg=65), ERANGE),
        ("n_neg < 0", _draw(n_pos=65, n_neg=-1), ERANGE),
        ("B == 0", _draw(n_neg=0), ERANGE),
        ("B == 1025", _draw(n_pos=1, n_neg=1024), ERANGE),
        ("uniform, cap 2^31", _draw(ring=dict(cap=1 << 31)), ERANGE),
        ("demo share, cap 2^31", _draw(stratified=DEMO, ring=dict(cap=1 << 31)), ERANGE),
        ("demo share, pinned == cap", _draw(stratified=DEMO, ring=dict(pinned=4096)), ERANGE),
        ("demo share, pinned < 0", _draw(stratified=DEMO, ring=dict(pinned=-1)), ERANGE),
        ("stratified == 3", _draw(stratified=3), EINVAL),
        ("stratified == -1", _draw(stratified=-1), EINVAL),
        ("stratified without pos_cnt", _draw(stratified=ST, ring=dict(pos_cnt=None)), EINVAL),
        ("stratified, cap 2^21 + 1", _draw(stratified=ST, ring=dict(cap=(1 << 21) + 1)), ERANGE),
        # several things wrong: pointers before the batch size, the batch size before the mode
        ("output missing and B == 0", _draw(s=None, n_neg=0), EINVAL),
        ("stratified without pos_cnt and B == 1025", _draw(stratified=ST, ring=dict(pos_cnt=None), n_neg=1025), ERANGE),
        ("stratified == 3 and B == 0", _draw(stratified=3, n_neg=0), ERANGE),
        ("stratified without pos_cnt and cap 2^21 + 1", _draw(stratified=ST, ring=dict(pos_cnt=None, cap=(1 << 21) + 1)), EINVAL),
    ]
    noise = (0, 0, 0, None, 0, None)                 # noise_pairs, seed, counter, counter_dev, counter_inc, out
    keys = ctypes.c_void_p(d)

    def sample(first, second, nz=noise):
        a, b = (None if x is None else ctypes.byref(x) for x in (first, second))
        args = _lib.rrl_sample_args_t(None if first is None else ctypes.pointer(first),
                                      None if second is None else ctypes.pointer(second), *nz)
        rc = lib.rrl_sample_multi(a, b, *nz, None)
        assert lib.rrl_sample_multi_packed(1, ctypes.byref(args), None) == rc
        return rc

    refused = _draw(stratified=3)                   # RRL_EINVAL: behind a first draw that passes, the launch answers this
    for what, x, want in draws:
        assert sample(x, None) == want, ("first", what)
        assert sample(x, refused) == want, ("first before a refused second", what)
        if want != EINVAL:
            assert sample(_draw(stratified=ST, ring=dict(cap=1 << 21)), x) == want, ("second", what)
        sel = _lib.rrl_draw_ahead_t(ctypes.pointer(x), 64, keys)
        assert lib.rrl_draw_select(ctypes.byref(sel), None) == (want if x.stratified == U else EINVAL), ("select", what)
    # the valid bounds pass: the second draw's code comes back, not RRL_ERANGE
    for what, x in [("stratified, cap 2^21", _draw(stratified=ST, ring=dict(cap=1 << 21))),
                    ("stratified, B == 1024", _draw(stratified=ST, n_pos=512, n_neg=512)),
                    ("uniform, cap 2^31 - 1", _draw(ring=dict(cap=(1 << 31) - 1))),
                    ("demo share, pinned == cap - 1", _draw(stratified=DEMO, ring=dict(pinned=4095)))]:
        assert sample(x, refused) == EINVAL, what
    # the launch's own arguments are looked at before any draw
    assert sample(None, None) == EINVAL
    assert sample(None, _draw()) == EINVAL
    for first in (_draw(), _draw(n_neg=0)):
        assert sample(first, None, (-1, 0, 0, None, 0, ctypes.c_void_p(d))) == EINVAL, "noise_pairs < 0"
        assert sample(first, None, (1 << 32, 0, 0, None, 0, ctypes.c_void_p(d))) == EINVAL, "noise_pairs 2^32"
        assert sample(first, None, (8, 0, 0, None, 0, None)) == EINVAL, "noise_pairs > 0 without noise_out"
    # rrl_draw_select: its own fields, then the mode, then the draw
    good = ctypes.pointer(_draw())
    assert lib.rrl_draw_select(None, None) == EINVAL
    assert lib.rrl_draw_select(ctypes.byref(_lib.rrl_draw_ahead_t(None, 64, keys)), None) == EINVAL
    assert lib.rrl_draw_select(ctypes.byref(_lib.rrl_draw_ahead_t(good, 64, None)), None) == EINVAL
    assert lib.rrl_draw_select(ctypes.byref(_lib.rrl_draw_ahead_t(good, -1, keys)), None) == EINVAL
    for mode in (ST, DEMO):
        sel = _lib.rrl_draw_ahead_t(ctypes.pointer(_draw(stratified=mode)), 64, keys)
        assert lib.rrl_draw_select(ctypes.byref(sel), None) == EINVAL, "select of a non-uniform draw"

    G, SH = _lib.HEAD_GAUSS, _lib.HEAD_STOCH
    heads = [
        ("head missing", _head(head=None)),
        ("scale missing", _head(scale=None)),
        ("bias missing", _head(bias=None)),
        ("action missing", _head(action=None)),
        ("B == 0", _head(B=0)),
        ("B < 0", _head(B=-8)),
        ("n_part 0", _head(n_part=0)),
        ("n_part 5", _head(n_part=5)),
        ("Gaussian without eps", _head(eps=None)),
        ("Gaussian with obs_in but no obs_out", _head(obs_in=d)),
        ("stochastic: head missing", _head(SH, head=None)),
        ("stochastic: n_part 5", _head(SH, n_part=5)),
        ("stochastic without log_std", _head(SH, log_std=None)),
        ("kind == 2", _head(kind=2)),
        ("kind == -1", _head(kind=-1)),
    ]
    P = _lib.rrl_policy_head_t

    def arr(*members):
        a = (P * 5)()                # five slots: a count of 5 is refused before any member is read, but stays in bounds
        for k, x in enumerate(members):
            a[k] = x
        return a

    for what, x in heads:
        assert lib.rrl_policy_heads_fwd_multi(1, arr(x), None) == EINVAL, what
        assert lib.rrl_policy_heads_fwd_multi(2, arr(_head(), x), None) == EINVAL, ("behind a good member", what)
        assert lib.rrl_policy_heads_fwd_multi(2, arr(x, _head(SH, eps=None)), None) == EINVAL, ("before a good member", what)
    for n in (0, 5, -1):             # 1 .. 4 members
        assert lib.rrl_policy_heads_fwd_multi(n, arr(_head()), None) == EINVAL
    assert lib.rrl_policy_heads_fwd_multi(1, None, None) == EINVAL


def _plan_cost(**fields):
    """A well-formed rrl_plan_cost_t of the supported shape (5 members, 20 particles); dummy non-null device pointers."""
    d = 0x1000
    return _with(_lib.rrl_plan_cost_t(packed=d, hq=256, he=200, n_nets=5, npart=20, f16x3=0, M=3, pop=40, plan_hor=5,
                                      cur_obs=d, ac_seqs=d, noise=d, seed=1, counter_dev=d, counter_inc=1, scratch=d,
                                      costs=d), **fields)


def _cem(**fields):
    d = 0x1000
    return _with(_lib.rrl_cem_t(M=3, pop=40, dim=10, mean=d, var=d, lb=d, ub=d, epsilon=1e-3, sticky=1, active=d, seed=1,
                                counter_dev=d, counter_inc=1, samples=d, num_elites=4, alpha=0.25, costs=d), **fields)


def _cem_set(**fields):
    d = 0x1000
    return _with(_lib.rrl_cem_set_t(n=64, mask=d, dim=10, du=2, prev_sol=d, init_var=d, obs=d, idx=d, count=d, mean=d,
                                    var=d, cur_obs=d, active=d, action=d), **fields)


def _loss(kind, **fields):
    """A well-formed rrl_loss_t of `kind` for rrl_loss_dout: the operands the header assigns to the kind, nothing else."""
    d = 0x1000
    L = _lib
    operands = {L.LOSS_SAC_CRITIC: dict(out_t=d, v0=d, v1=d, v2=d, alpha=d, loss=d),
                L.LOSS_SAC_POLICY: dict(v0=d, alpha=d, loss=d),
                L.LOSS_QRISK_CRITIC: dict(out_t=d, v0=d, v1=d, loss=d),
                L.LOSS_QRISK_POLICY: dict(loss=d),
                L.LOSS_DGD_QRISK: dict(loss=d, f0=0.5),
                L.LOSS_GAUSS_HEAD: dict(v0=d, v1=d, d_action=d, ld=4, n_heads=2),
                L.LOSS_STOCH_HEAD: dict(v0=d, v1=d, v2=d, d_action=d, ld=4, n_heads=2, loss=d)}
    return _with(_lib.rrl_loss_t(kind=kind, n_part=1, out=d, **operands.get(kind, {})), **fields)


def test_planner_cem_and_loss_descriptor_validation_without_gpu():
    """What rrl_plan_cost, rrl_plan_pack, rrl_cem_sample / update / begin / finish and rrl_loss_dout answer to a malformed
    descriptor: every call returns before any launch (dummy non-null device pointers are never followed).  The codes are
    those of ABI version 7, recorded on a machine without a GPU by calling that library's positional entries (the _f16x3 /
    _n forms where the descriptor sets f16x3 / m_dev; the seven rrl_*_grad / rrl_*_head_bwd entries for the seven kinds)
    with the same values.  Three answers have no positional counterpart: a NULL descriptor, kind == -1 / an unknown kind
    (RRL_EINVAL: nothing to compute / RRL_ERANGE as in rrl_head_bwd_t), and da_parts > 1 (the positional head entries
    had no such argument: the stand-alone kernels read a plain d_action).  The only calls here that are not refused are
    the CEM steps on M == 0 problems, which answer RRL_OK without a launch.  rrl_rcpo_penalty's cases stand beside the
    packed entry's in tests/test_packed_baselines_cpu.py."""
    lib = _lib.load()
    OK, EINVAL, ERANGE = 0, -1, -3
    d = 0x1000
    ref = ctypes.byref

    # -- planner: every failure is RRL_EINVAL; either precision, host or device count
    plans = [
        ("packed missing", dict(packed=None)), ("cur_obs missing", dict(cur_obs=None)), ("ac_seqs missing", dict(ac_seqs=None)),
        ("scratch missing", dict(scratch=None)), ("costs missing", dict(costs=None)),
        ("M 0", dict(M=0)), ("M < 0", dict(M=-1)), ("pop 0", dict(pop=0)), ("plan_hor 0", dict(plan_hor=0)),
        ("plan_hor 17", dict(plan_hor=17)), ("hq 128", dict(hq=128)), ("he 256", dict(he=256)), ("n_nets 0", dict(n_nets=0)),
        ("npart != 4 n_nets", dict(npart=10)), ("rows >= 2^32", dict(M=1 << 22, pop=400)),
        ("noise missing and pop 0", dict(noise=None, pop=0)),
    ]
    for what, f in plans:
        for f16x3 in (0, 1):
            for m_dev in (None, d):
                assert lib.rrl_plan_cost(ref(_plan_cost(f16x3=f16x3, m_dev=m_dev, **f)), None) == EINVAL, (what, f16x3, m_dev)
    assert lib.rrl_plan_cost(None, None) == EINVAL
    w = _lib.rrl_plan_weights_t(256, 200, 5, *([d] * 18))
    for f16x3 in (0, 1):
        assert lib.rrl_plan_pack(None, f16x3, d, None) == EINVAL
        assert lib.rrl_plan_pack(ref(w), f16x3, None, None) == EINVAL
        for f in (dict(hq=128), dict(he=256), dict(n_nets=0)):
            assert lib.rrl_plan_pack(ref(_with(_lib.rrl_plan_weights_t(256, 200, 5, *([d] * 18)), **f)), f16x3, d, None) == EINVAL

    # -- CEM: pointers (RRL_EINVAL), then sizes (RRL_ERANGE), then num_elites (RRL_EINVAL), then M == 0 (RRL_OK)
    sizes = [("M < 0", dict(M=-1)), ("pop 0", dict(pop=0)), ("pop 1025", dict(pop=1025)), ("dim 0", dict(dim=0)),
             ("dim 65", dict(dim=65))]
    sample = [(n + " missing", {n: None}, EINVAL) for n in ("mean", "var", "lb", "ub", "active", "samples")]
    sample += [(what, f, ERANGE) for what, f in sizes]
    sample += [
        ("M pop > 0xffffffff", dict(M=1 << 23, pop=1024), ERANGE),
        ("M pop == 2^32 with pop 1024", dict(M=1 << 22, pop=1024), ERANGE),
        ("mean missing and pop 0", dict(mean=None, pop=0), EINVAL),
        ("samples missing and M pop > 0xffffffff", dict(samples=None, M=1 << 23, pop=1024), EINVAL),
        ("costs missing (not read) and dim 65", dict(costs=None, dim=65), ERANGE),
        ("num_elites 0 (not read) and M 0", dict(num_elites=0, M=0), OK),
        ("M 0", dict(M=0), OK),
    ]
    update = [(n + " missing", {n: None}, EINVAL) for n in ("samples", "costs", "mean", "var")]
    update += [(what, f, ERANGE) for what, f in sizes]
    update += [
        ("num_elites 0", dict(num_elites=0), EINVAL),
        ("num_elites pop + 1", dict(num_elites=41), EINVAL),
        ("costs missing and pop 1025", dict(costs=None, pop=1025), EINVAL),
        ("pop 0 and num_elites 0", dict(pop=0, num_elites=0), ERANGE),
        ("dim 65 and num_elites pop + 1", dict(dim=65, num_elites=41), ERANGE),
        ("num_elites 0 and M 0", dict(num_elites=0, M=0), EINVAL),
        ("active missing (nullable) and dim 0", dict(active=None, dim=0), ERANGE),
        ("active, lb, ub missing (nullable / not read) and M 0", dict(active=None, lb=None, ub=None, M=0), OK),
        ("M 0", dict(M=0), OK),
    ]
    for entry, cases in ((lib.rrl_cem_sample, sample), (lib.rrl_cem_update, update)):
        for what, f, want in cases:
            for m_dev in (None, d):
                assert entry(ref(_cem(m_dev=m_dev, **f)), None) == want, (entry.__name__, what, m_dev)
        assert entry(None, None) == EINVAL

    set_sizes = [("n 0", dict(n=0)), ("n < 0", dict(n=-1)), ("n 2^31", dict(n=1 << 31)), ("dim 0", dict(dim=0)),
                 ("dim 65", dict(dim=65))]
    begin = [(n + " missing", {n: None}, EINVAL) for n in ("mask", "prev_sol", "init_var", "obs", "idx", "count", "mean", "var",
                                                           "cur_obs", "active")]
    begin += [(what, f, ERANGE) for what, f in set_sizes]
    begin += [("obs missing and n 0", dict(obs=None, n=0), EINVAL),
              ("action missing, du 0 (not read) and n 0", dict(action=None, du=0, n=0), ERANGE)]
    finish = [(n + " missing", {n: None}, EINVAL) for n in ("mask", "idx", "count", "mean", "prev_sol", "action")]
    finish += [(what, f, ERANGE) for what, f in set_sizes]
    finish += [("du 0", dict(du=0), ERANGE), ("du dim + 1", dict(du=11), ERANGE),
               ("action missing and du 0", dict(action=None, du=0), EINVAL),
               ("begin's inputs missing (not read) and n 0", dict(init_var=None, obs=None, var=None, cur_obs=None, active=None,
                                                                  n=0), ERANGE)]
    for entry, cases in ((lib.rrl_cem_begin, begin), (lib.rrl_cem_finish, finish)):
        for what, f, want in cases:
            assert entry(ref(_cem_set(**f)), None) == want, (entry.__name__, what)
        assert entry(None, None) == EINVAL

    # -- stand-alone loss gradients: everything the kind's positional entry refused is RRL_EINVAL
    L = _lib
    required = {L.LOSS_SAC_CRITIC: ("out", "out_t", "v0", "v1", "v2", "alpha"),
                L.LOSS_SAC_POLICY: ("out", "v0", "alpha"),
                L.LOSS_QRISK_CRITIC: ("out", "out_t", "v0", "v1"),
                L.LOSS_QRISK_POLICY: ("out",),
                L.LOSS_DGD_QRISK: ("out",),
                L.LOSS_GAUSS_HEAD: ("out", "v0", "v1", "d_action"),
                L.LOSS_STOCH_HEAD: ("out", "v0", "v1", "v2", "d_action", "loss")}
    dout = lambda loss, B=64, out=d: lib.rrl_loss_dout(ref(loss), B, out, None)
    for kind, names in required.items():
        for n in names:
            assert dout(_loss(kind, **{n: None})) == EINVAL, (kind, n + " missing")
        assert dout(_loss(kind), out=None) == EINVAL, (kind, "dout missing")
        for B in (0, -64):
            assert dout(_loss(kind), B=B) == EINVAL, (kind, "B", B)
        for n_part in (0, 5, -1):
            assert dout(_loss(kind, n_part=n_part)) == EINVAL, (kind, "n_part", n_part)
        if kind in (L.LOSS_GAUSS_HEAD, L.LOSS_STOCH_HEAD):
            for n_heads in (0, -1):
                assert dout(_loss(kind, n_heads=n_heads)) == EINVAL, (kind, "n_heads", n_heads)
            assert dout(_loss(kind, da_parts=2, da_part_stride=256)) == EINVAL, (kind, "d_action as partials")
            assert dout(_loss(kind, da_parts=16, da_part_stride=256, da_group=4)) == EINVAL, (kind, "d_action as tile partials")
    assert dout(_loss(-1)) == EINVAL                       # `out` already is dOut
    for kind in (7, -2, 1 << 20):
        assert dout(_loss(kind)) == ERANGE, ("kind", kind)
    assert lib.rrl_loss_dout(None, 64, d, None) == EINVAL


def test_product_has_no_cpu_fallback():
    import pytest
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from recovery_rl_amd.env import make_vec_env
    with pytest.raises(_lib.RRLError):
        make_vec_env("navigation1", 4, device="cuda")
    with pytest.raises(_lib.RRLError):
        make_vec_env("navigation1", 4, device="cpu")


def test_product_never_imports_oracle():
    pkg = os.path.join(ROOT, "recovery_rl_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".hpp", ".h")):
                txt = open(os.path.join(dirpath, f)).read()
                assert "oracle" not in txt.lower() or f in (), (dirpath, f)


def test_header_is_plain_c(tmp_path):
    """include/rrl_hip.h is the C ABI a binding includes: it must compile as C99 on its own."""
    import subprocess
    src = tmp_path / "t.c"
    src.write_text('#include "rrl_hip.h"\nint main(void) { return rrl_abi_version() < 0; }\n')
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(root, "include"),
                           str(src)])


def test_pos_cnt_length_macro_matches_the_python_allocation(tmp_path):
    """RRL_POS_CNT_LEN(cap) of the header (what a binding allocates for rrl_replay_t.pos_cnt: chunk counts, super-chunk
    counts, chunk masks) equals the length replay_memory.py allocates, for aligned and ragged capacities."""
    import subprocess
    caps = [1, 63, 64, 65, 1000, 1023, 1024, 1025, 4096, 5000, 70000, 1000000, 1 << 21]
    src = tmp_path / "len.c"
    src.write_text('#include <stdio.h>\n#include "rrl_hip.h"\nint main(void) {\n' +
                   "".join('  printf("%%lld\\n", (long long)RRL_POS_CNT_LEN(%dLL));\n' % c for c in caps) +
                   "  return 0;\n}\n")
    exe = tmp_path / "len"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o",
                           str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    want = []
    for cap in caps:
        n_chunks = (cap + 63) // 64
        want.append((((n_chunks + 3) // 4) * 4 + (cap + 1023) // 1024 + 1) // 2 * 2 + 2 * n_chunks)
    assert got == want
    src_py = open(os.path.join(ROOT, "recovery_rl_amd", "replay_memory.py")).read()
    assert "(((n_chunks + 3) // 4) * 4 + (cap + 1023) // 1024 + 1) // 2 * 2 + 2 * n_chunks" in src_py
