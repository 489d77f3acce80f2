"""Stack.backward on a plain dOut tensor through the descriptor entry points alone (rrl_head_bwd_t / rrl_hidden_bwd_t /
rrl_input_bwd_t, one stack per launch) against torch float64, with no tolerance: every operand is a small integer, so
every product and every partial sum is an integer below 2^24 and exact in f32 in whatever order a kernel adds."""
import functools

import pytest
import torch

from recovery_rl_amd.fast_update import FlatNet, Stack

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# (G, H, B, din, dout, first layer inside the hidden-layer launch)
SHAPES = {
    "ragged_tiles": (2, 48, 40, 4, 1, False),            # no full tile row, FAST = false
    "full_tiles_short_K": (1, 128, 64, 2, 4, False),     # full tiles, K = B = 64 is not a panel multiple
    "first_layer_own_launch": (2, 128, 128, 4, 1, False),    # what set_fuse_first(False) runs
    "first_layer_fused": (2, 128, 128, 4, 1, True),          # (dW1, db1) and dx as tile partials
    # the production shapes the method still admits (the bound below: 2 * 256 * 2 * 256 * 4 * 4 = 2^22) ...
    "critic_256": (2, 256, 256, 4, 1, True),
    "policy_256": (1, 256, 256, 2, 4, True),
    "ragged_batch_256": (2, 256, 200, 4, 1, False),          # ... and --batch_size 200 at that width
}
FLAGS = ((True, False), (True, True), (False, True))     # (weight_grads, input_grad)
SENTINEL = 7.0


def ints(gen, *shape):
    return torch.randint(-2, 3, shape, generator=gen, device="cpu").double()


@functools.lru_cache(maxsize=None)
def problem(G, H, B, din, dout):
    """Operands (float64, on the host) and the float64 gradients of one shape: computed once, shared by its cases."""
    gen = torch.Generator().manual_seed(1000 * H + B)
    p = dict(x=ints(gen, B, din), h1=ints(gen, G, B, H), h2=ints(gen, G, B, H), dOut=ints(gen, G, B, dout),
             W1=ints(gen, G, H, din), b1=ints(gen, G, H), W2=ints(gen, G, H, H), b2=ints(gen, G, H),
             W3=ints(gen, G, dout, H), b3=ints(gen, G, dout))
    dh2 = (p["dOut"] @ p["W3"]) * (p["h2"] > 0)
    dh1 = (dh2 @ p["W2"]) * (p["h1"] > 0)
    ref = dict(W3=p["dOut"].transpose(1, 2) @ p["h2"], b3=p["dOut"].sum(1),
               W2=dh2.transpose(1, 2) @ p["h1"], b2=dh2.sum(1),
               W1=dh1.transpose(1, 2) @ p["x"], b1=dh1.sum(1), dx=dh1 @ p["W1"])
    # every partial sum of every output is bounded by the sum of the magnitudes: |dh2| <= 4 dout, |dh1| <= 2 H |dh2|, and
    # the widest sums run over max(B, H) terms of magnitude <= 2 |dh1| (by hand 2^20 at G 1, H 128, B 64, dout 4)
    assert 2 * max(B, H) * 2 * H * 4 * dout < 2 ** 24
    assert max(float(v.abs().max()) for v in ref.values()) < 2 ** 24
    return p, ref


@pytest.mark.parametrize("weight_grads,input_grad", FLAGS)
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_stack_backward_on_a_dout_tensor_is_exact_against_float64(shape, weight_grads, input_grad):
    G, H, B, din, dout, fused = SHAPES[shape]
    p, ref = problem(G, H, B, din, dout)
    f32 = lambda t: t.to(device=DEV, dtype=torch.float32)
    net = FlatNet([("W1", (G, H, din)), ("b1", (G, H)), ("W2", (G, H, H)), ("b2", (G, H)), ("W3", (G, dout, H)),
                   ("b3", (G, dout))], DEV)
    net.G, net.H, net.din, net.dout = G, H, din, dout
    for name in net.p:
        net.p[name].copy_(f32(p[name]))
    st = Stack(net, B)
    assert st.fuse_first == (B % 128 == 0 and H % 128 == 0)
    st.fuse_first = fused
    st.x = f32(p["x"])
    st.h1.copy_(f32(p["h1"]))
    st.h2.copy_(f32(p["h2"]))
    net.grad.fill_(SENTINEL)
    st.dx.fill_(SENTINEL)
    if st.first_part is not None:
        st.first_part.fill_(SENTINEL)
        st.dx_part.fill_(SENTINEL)
    got = st.backward(f32(p["dOut"]).contiguous(), weight_grads=weight_grads, input_grad=input_grad)
    torch.cuda.synchronize()
    if fused and weight_grads:          # (dW1, db1) as row-tile partials laid out like the head of the flat gradient buffer
        net.grad[:st.n_first] = st.first_part.double().sum(0).float()
    want = lambda name: ref[name].float().to(DEV)
    for name in ("W3", "b3", "W2", "b2", "W1", "b1"):
        if weight_grads:
            assert torch.equal(net.g[name], want(name)), name
        else:
            assert bool((net.g[name] == SENTINEL).all()), name
    if st.first_part is not None:       # the partials are written where asked for, and only there
        assert bool((st.first_part == SENTINEL).all()) != (fused and weight_grads)
        assert bool((st.dx_part == SENTINEL).all()) != (fused and input_grad)
    if not input_grad:
        assert got is None and bool((st.dx == SENTINEL).all())
    elif fused:
        assert got is st.dx_part and st.dx_parts()[1:] == (H // 16, st.dx_part.stride(0), 4)
        assert torch.equal(got.double().sum(0).float(), want("dx"))
    else:
        assert got is st.dx and torch.equal(got, want("dx"))
