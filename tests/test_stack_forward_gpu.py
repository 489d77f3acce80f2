"""The three-layer stack forward (csrc/mlp_fwd_kernels.hip) through every entry point and on every kernel its host dispatch
can choose -- the case table of stack_cases.py, which test_stack_forward_cpu.py proves complete -- against torch float64 with
no tolerance: every operand is a small integer, so every product and every partial sum is an integer below 2^24 and exact in
f32 in whatever order a kernel adds.  Every case also checks what a kernel must not do: the floats behind every output buffer
keep their sentinel (G = 1 cases included, where nothing else would hide a store past row M), and the rows behind the M rows
of every input are NaN, so that a read past row M that reaches a live row shows.  A policy head inside the stack kernel yields
no integers: it is pinned bit for bit to the stand-alone head launch (itself pinned to float64 in test_update_pieces_gpu.py)
and to the same stack without the head on the action it wrote."""
import ctypes as C
import os

import pytest
import torch

import stack_cases as SC
from recovery_rl_amd import _lib, fused

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _sync():
    torch.cuda.synchronize()


# ---- rrl_mlp3_forward --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SC.names("positional"))
def test_positional_forward_is_exact_against_float64(name):
    case = SC.BY_NAME[name]
    (m,) = case.members
    p, ref = SC.problem(m)
    split = SC.is_split(m)
    assert SC.case_path(case).label in (("0/256", "0/gen", "3") if split else ("1", "2"))
    _, t = SC.device_stack(m, p, DEV, save=case.opts.get("save", True), strided=case.opts.get("strided", False))
    finalize = case.opts.get("finalize", 1)
    fused.mlp3_forward(t["x"], t["W1"], t["b1"], t["W2"], t["b2"], t["W3"], t["b3"], out=t["out"], h1=t.get("h1"), h2=t.get("h2"),
                       scratch=t.get("scratch"), finalize=bool(finalize))
    _sync()
    SC.check_exact(t, ref, split, out_written=(not split) or bool(finalize), what=name)


# ---- groups of descriptors: rrl_mlp3_forward_multi and rrl_mlp3_forward_multi_packed ---------------------------------------------
def _groups(case):
    """The case's members as a list of groups (one for rrl_mlp3_forward_multi, one per seed for the packed entry), every
    member with a seed of its own: different weights and inputs everywhere."""
    groups = case.members if case.entry == "packed" else (case.members,)
    heads = case.opts.get("heads")
    if heads is not None and case.entry != "packed":
        heads = (heads,)
    out = []
    for s, g in enumerate(groups):
        out.append([(m, 10 * s + k, heads[s][k] if heads else None) for k, m in enumerate(g)])
    return out


def _launch(case, desc_groups):
    if case.entry == "packed":
        SC.forward_packed(desc_groups)
    else:
        SC.forward_multi(desc_groups[0])
    _sync()


def _pack_env_unset():
    # read once per process by the library: a stray setting would quietly turn the loop case into another kernel's
    assert os.environ.get("RRL_PACK_FWD_LOOP") is None, "RRL_PACK_FWD_LOOP is set: the packed cases would not run the kernels they claim"
    assert os.environ.get("RRL_PACK_PINNED") is None, "RRL_PACK_PINNED is set: the packed cases would not run the kernels they claim"


@pytest.fixture
def clean_plans():
    """Packed plans are keyed by the descriptors' bytes, pointers included: none may outlive its buffers."""
    lib = _lib.load()
    lib.rrl_pack_clear()
    yield
    _sync()
    lib.rrl_pack_clear()


def _run_exact(case):
    w2p = case.opts.get("w2p")
    stacks = []
    for group in _groups(case):
        row = []
        for m, seed, _ in group:
            p, ref = SC.problem(m, seed)
            desc, t = SC.device_stack(m, p, DEV, save=case.opts.get("save", True), strided=case.opts.get("strided", False), w2p=w2p)
            assert (desc.h1 is None and desc.h2 is None) == (not case.opts.get("save", True))
            row.append((m, seed, desc, t, ref))
        stacks.append(row)
    _launch(case, [[s[2] for s in row] for row in stacks])
    for row in stacks:
        for k, (m, seed, desc, t, ref) in enumerate(row):
            split = SC.is_split(m)
            what = (case.name, "seed %d member %d" % (seed // 10, k))
            if w2p == "other":          # the copy is what is read: the result is the other W2's
                other = SC.reference_other(m, seed)
                assert not torch.equal(other["partials"], ref["partials"])
                ref = other
            SC.check_exact(t, ref, split, out_written=not split, what=what)


@pytest.mark.parametrize("name", SC.names("multi", heads=False))
def test_forward_multi_is_exact_against_float64(name):
    _run_exact(SC.BY_NAME[name])


@pytest.mark.parametrize("name", SC.names("packed", heads=False))
def test_forward_multi_packed_is_exact_for_every_seed(name, clean_plans):
    _pack_env_unset()
    case = SC.BY_NAME[name]
    assert SC.case_path(case).label.startswith("packed")
    _run_exact(case)


# ---- a policy head inside the stack kernel -----------------------------------------------------------------------------------
def _run_heads(case):
    w2p = case.opts.get("w2p")
    first, second, info = [], [], []
    for group in _groups(case):
        d1, d2 = [], []
        for m, seed, head in group:
            p, ref = SC.problem(m, seed)
            if head is None:
                desc, t = SC.device_stack(m, p, DEV, w2p=w2p)
                desc_b, t_b = SC.device_stack(m, p, DEV, w2p=w2p)
                info.append((m, seed, None, t, t_b, ref, None, None))
            else:
                kind, n_part, obs = head
                assert m.din == 4
                x = p["x"].clone()
                x[:, 2:] = float("nan")              # columns 2..3 are computed, not read
                desc, t = SC.device_stack(m, p, DEV, w2p=w2p, x_live=x)
                ops = SC.head_operands(m.M, kind, n_part, obs, DEV, seed=1000 + seed)
                outs = SC.head_outputs(ops, DEV)
                desc.in_head = SC.head_desc(ops, outs)
                desc.use_in_head = 1
                # the same stack without the head: its x is filled in once the action exists
                desc_b, t_b = SC.device_stack(m, p, DEV, w2p=w2p, x_live=x)
                info.append((m, seed, ops, t, t_b, ref, outs, desc_b))
            d1.append(desc), d2.append(desc_b)
        first.append(d1), second.append(d2)
    _launch(case, first)
    lib = _lib.load()
    for m, seed, ops, t, t_b, ref, outs, _ in info:
        if ops is None:
            continue
        M = m.M
        # (a) + (c): action, logp and obs_out are the stand-alone head launch's, bit for bit, the sentinel rows behind row M
        # and the columns nobody was asked to write included
        alone = SC.head_outputs(ops, DEV)
        hd = (_lib.rrl_policy_head_t * 1)(SC.head_desc(ops, alone))
        _lib.check(lib.rrl_policy_heads_fwd_multi(1, hd, _lib.current_stream()), "rrl_policy_heads_fwd_multi")
        _sync()
        what = (case.name, "seed %d" % (seed // 10), m)
        assert torch.equal(outs["xa"], alone["xa"]), (what, "action / obs_out")
        assert torch.equal(outs["logp"], alone["logp"]), (what, "logp")
        assert bool((outs["xa"][M:] == SC.SENT).all()) and bool((outs["logp"][M:] == SC.SENT).all()), (what, "rows behind M")
        act = outs["xa"][:M, 2:]
        assert bool(torch.isfinite(act).all()) and not bool((act == SC.SENT).any()), what
        if ops["kind"] == SC.GAUSS:
            assert bool(torch.isfinite(outs["logp"][:M]).all()) and not bool((outs["logp"][:M] == SC.SENT).any()), what
        if ops["obs_in"] is not None:
            t_b["x"][:, :2] = ops["obs_in"][:M]
        if ops["obs_in"] is not None and ops["kind"] == SC.GAUSS:
            assert torch.equal(outs["xa"][:M, :2], ops["obs_in"][:M]), (what, "obs_out")
        else:       # the stochastic head as a launch of its own ignores obs_out (rrl_hip.h): so does the stack kernel
            assert bool((outs["xa"][:, :2] == SC.SENT).all()), (what, "obs_out written by a head that has none")
        t_b["x"][:, 2:] = act
    # (b) partials, h1 and h2 are those of the same launch without the heads on x = [obs | that action]
    _launch(case, second)
    for m, seed, ops, t, t_b, ref, outs, _ in info:
        what = (case.name, "seed %d" % (seed // 10), m)
        assert not SC.guards_intact(t) and not SC.guards_intact(t_b), what
        if ops is None:
            SC.check_exact(t, ref, True, out_written=False, what=what)
            SC.check_exact(t_b, ref, True, out_written=False, what=what)
            continue
        for k in ("scratch", "h1", "h2"):
            assert torch.equal(t[k], t_b[k]), (what, k)
            assert bool(torch.isfinite(t[k]).all()) and not bool((t[k] == SC.SENT).any()), (what, k)
        assert bool((t["out"] == SC.SENT).all()), what
        # the first layer on the observation columns alone is still an integer problem where the action's weights are zero:
        # the rows really are the case's x (not, say, row 0 everywhere)
        assert not torch.equal(t["h1"][:, 0], t["h1"][:, m.M - 1]) or m.M == 1, what


@pytest.mark.parametrize("name", SC.names("multi", heads=True))
def test_a_policy_head_inside_the_stack_kernel_is_the_stand_alone_head_and_stack(name):
    case = SC.BY_NAME[name]
    assert SC.case_path(case).label in ("0/256", "0/gen", "3", "5")
    _run_heads(case)


@pytest.mark.parametrize("name", SC.names("packed", heads=True))
def test_a_policy_head_inside_the_packed_loop_kernel(name, clean_plans):
    _pack_env_unset()
    case = SC.BY_NAME[name]
    assert SC.case_path(case).label == "packed4"
    _run_heads(case)


# ---- rrl_mlp3_forward_riders ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SC.names("riders"))
def test_a_noise_rider_in_front_of_the_stack_leaves_both_exact(name):
    case = SC.BY_NAME[name]
    (m,) = case.members
    p, ref = SC.problem(m)
    desc, t = SC.device_stack(m, p, DEV, save=case.opts.get("save", True), strided=case.opts.get("strided", False),
                              w2p=case.opts.get("w2p"))
    assert desc.ldx == (SC.LDX_STRIDED if case.opts.get("strided") else m.din)
    lib = _lib.load()
    pairs = 3000
    flat, noise = SC.guarded(DEV, pairs, 2)
    alone = torch.zeros(pairs, 2, device=DEV)
    ticks = [torch.tensor([5, 0], dtype=torch.int64, device=DEV) for _ in range(2)]       # {tick, ticket (kept 0: rrl_hip.h)}
    riders = _lib.rrl_fwd_riders_t(None, None, None, pairs, 77, 0, _lib.ptr(ticks[0]), 1, _lib.ptr(noise))
    _lib.check(lib.rrl_mlp3_forward_riders(C.byref(desc), C.byref(riders), _lib.current_stream()), "rrl_mlp3_forward_riders")
    _lib.check(lib.rrl_normal_fill(pairs, 77, 0, _lib.ptr(ticks[1]), 1, _lib.ptr(alone), _lib.current_stream()), "rrl_normal_fill")
    _sync()
    SC.check_exact(t, ref, True, out_written=False, what=name)
    assert torch.equal(noise, alone) and torch.equal(ticks[0], ticks[1]) and bool((SC.guard_of(flat, noise) == SC.SENT).all())
    assert ticks[0].tolist() == [6, 0] and float(noise.std()) > 0.5


def _int_rows(n, gen):
    f = lambda *s: torch.randint(-2, 3, s, generator=gen).float().to(DEV)
    return f(n, 2), f(n, 2), f(n), f(n, 2), f(n)


@pytest.mark.parametrize("name", SC.names("riders_keyed"))
def test_the_keyed_forward_is_exact_on_the_rows_the_stand_alone_draw_returns(name):
    """The batch's keys are selected 50 rows ahead, the rows pushed, and the forward reads its 2 B = 200 rows (s' over s)
    through the keys from a ring of integer-valued rows while its gather rider writes them to x: x is the stand-alone draw's
    batch and the partials are float64's on it."""
    from test_draw_ahead_gpu import _select
    from recovery_rl_amd.replay_memory import ReplayMemory
    case = SC.BY_NAME[name]
    (m,) = case.members
    B = m.M // 2
    assert m.M == 2 * B and m.M % 16 != 0 and m.din == 2
    gen = torch.Generator().manual_seed(17)
    mems = [ReplayMemory(512, 5, device=DEV) for _ in range(2)]
    before, pushed = _int_rows(300, gen), _int_rows(50, gen)
    for mem in mems:
        mem.push(*before)
        mem.sample(B)
    ahead, alone = mems
    _select(ahead, 50, batch=B)
    for mem in mems:
        mem.push(*pushed)
    p, _ = SC.problem(m)
    nan_rows = torch.full((m.M, 2), float("nan"), dtype=torch.float64)
    desc, t = SC.device_stack(m, p, DEV, save=case.opts.get("save", True), w2p=case.opts.get("w2p"), x_live=nan_rows, ldx=4)
    assert desc.ldx == 4
    rows = [tuple(torch.zeros(B, 4, device=DEV) for _ in range(3)) for _ in range(2)]
    xfull = t["xbuf"][:m.M]
    d, _ = ahead.draw_desc(B, rows=(rows[0][0], xfull[:B], xfull[B:]))
    gat = _lib.rrl_draw_ahead_t(C.pointer(d), 0, _lib.ptr(ahead.ahead_keys(B)))
    riders = _lib.rrl_fwd_riders_t(None, C.pointer(gat), None, 0, 0, 0, None, 0, None)
    _lib.check(_lib.load().rrl_mlp3_forward_riders(C.byref(desc), C.byref(riders), _lib.current_stream()), "rrl_mlp3_forward_riders")
    alone.sample(B, rows=rows[1])
    _sync()
    ahead.check_error()
    assert torch.equal(ahead.tick, alone.tick) and torch.equal(ahead.state, alone.state)
    for got, want in zip(ahead._batch(B), alone._batch(B)):
        assert torch.equal(got, want)
    x = torch.cat([alone._batch(B)[3], alone._batch(B)[0]])
    assert torch.equal(t["x"], x) and bool(x.abs().max() <= 2) and torch.equal(x, x.round())
    assert bool(torch.isnan(t["xbuf"][m.M:]).all())
    assert len({tuple(r) for r in x.tolist()}) > 10                     # a batch of different rows
    ref = SC.reference(x.double().cpu(), p["W1"], p["b1"], p["W2"], p["b2"], p["W3"], p["b3"])
    assert max(float(v.abs().max()) for v in ref.values()) <= SC.bound(m)[2] < 2 ** 24
    SC.check_exact(t, ref, True, out_written=False, what=name)
