"""Hand-written forward + backward of the SAC / Q_risk updates on the fused HIP kernels
(csrc/mlp_kernels.hip, csrc/update_kernels.hip) -- the `fast path` of `SAC.update_parameters`
(recovery_rl/sac.py:170-277) and `QRiskWrapper.update_parameters` (recovery_rl/qrisk.py:86-163).

Same mathematics as the autograd path in sac.py / qrisk.py (which stays as the general path for
automatic entropy tuning / Deterministic policy, and for the comparison algorithms LR / RSPO / SQRL / RCPO unless
RRL_FAST_BASELINES=1 routes them here);
`tests/test_fast_update_gpu.py` checks the two paths against each other and against the
reference KATs.  ~37 launches per update instead of ~150, no vendor GEMM.

Parameters of every network live in ONE flat f32 buffer (the nn.Module parameters are views into
it), twin heads stacked on a leading dimension so both heads run in one batched launch; Adam and
the Polyak target update are one kernel over the flat buffer.
"""
import math

import ctypes as C

import torch

from . import _lib, paths
from .fused import NN, NT, TN, gemm, mlp3_forward, mlp3_supported
# the switches and path decisions live in paths.py; the names below stay importable from here
from .paths import (BASELINE_FLAGS, eval_qsample_f16x3_enabled, eval_qsample_line, eval_rollout_path,  # noqa: F401
                    eval_scoring, eval_sqrl_f16x3_enabled, eval_sqrl_line, fast_baselines_enabled, fast_eval_enabled,
                    fast_eval_maze_enabled, fast_eval_qsample_enabled, fast_eval_sqrl_enabled, fast_path_supported,
                    fast_qsample_enabled, fast_sqrl_enabled, pack_qsample_enabled, pack_sqrl_enabled, qsample_acting_path,
                    qsample_f16x3_enabled, qsample_scoring, sqrl_acting_path, sqrl_f16x3_enabled, sqrl_scoring,
                    uses_baseline_terms)


# -- launch tape (seed packing, recovery_rl_amd/packed.py) -----------------------------------------------------------
# While a tape is set, every launch of the grouped path is ALSO appended to it: (kind, ctypes payload...).  The argument
# blocks of the steady-state iteration never change, so one recorded iteration of every seed is the launch list of the
# packed iteration: launch k of all seeds goes out as one rrl_*_packed call.
_TAPE = None


def set_tape(tape):
    global _TAPE
    _TAPE = tape


def record(kind, *payload):
    if _TAPE is not None:
        _TAPE.append((kind,) + payload)


# the FlatNets of a FastUpdater (attribute names): what checkpoints save and what seed packing switches
FLAT_NETS = ("critic", "critic_target", "policy", "qrisk", "qrisk_target", "recpolicy")


class FlatNet:
    """Flat parameter / gradient / Adam-state storage for one network, plus the layer views."""

    def __init__(self, named_shapes, device):
        self.device = device
        self.shapes = dict(named_shapes)
        total = sum(int(torch.Size(s).numel()) for _, s in named_shapes)
        self.flat = torch.zeros(total, dtype=torch.float32, device=device)
        self.grad = torch.zeros_like(self.flat)
        self.m = torch.zeros_like(self.flat)
        self.v = torch.zeros_like(self.flat)
        self.step = torch.zeros(2, dtype=torch.int64, device=device)   # {t, ticket}
        self.p, self.g, self.offset = {}, {}, {}
        off = 0
        for name, shape in named_shapes:
            n = int(torch.Size(shape).numel())
            self.p[name] = self.flat[off:off + n].view(shape)
            self.g[name] = self.grad[off:off + n].view(shape)
            self.offset[name] = off
            off += n
        # W2 a second time in the forward kernels' MFMA fragment order (rrl_w2_pack / rrl_stack_t.W2p; hidden width 256):
        # written by the fused optimiser launch together with the parameters (adam_multi), re-made from the row-major
        # values by every EAGER forward (w2_packed()) -- torch code may have written the parameters through the modules'
        # views since, and a permutation of 64 K floats costs less than finding out
        shape = self.shapes.get("W2")
        self.w2p = None
        if shape is not None and len(shape) == 3 and shape[1] == shape[2] == 256 and self.offset["W2"] % 4 == 0 \
                and torch.device(device).type == "cuda" and paths.switch("RRL_W2_FRAG"):
            self.w2p = torch.empty(int(torch.Size(shape).numel()), dtype=torch.float32, device=device)

    def w2_packed(self):
        """The fragment-order copy of W2, current: re-made here unless a hipGraph is being captured (a captured iteration is
        replayed with nothing but the library's kernels between its launches, and those keep the copy in step)."""
        if self.w2p is None:
            return None
        if not torch.cuda.is_current_stream_capturing():
            W2 = self.p["W2"]
            _lib.check(_lib.load().rrl_w2_pack(W2.shape[0], W2.shape[1], W2.data_ptr(), self.w2p.data_ptr(),
                                               _lib.current_stream()), "rrl_w2_pack")
        return self.w2p

    def rebind_grad(self, storage):
        """Move the gradient buffer into `storage` (a slice of a bucket shared with other networks, so that one
        collective reduces them together)."""
        assert storage.numel() == self.flat.numel() and storage.is_contiguous()
        self.grad = storage
        off = 0
        for name, shape in self.shapes.items():
            n = int(torch.Size(shape).numel())
            self.g[name] = storage[off:off + n].view(shape)
            off += n

    def adopt(self, name, params):
        """Copy the current values of `params` (list of nn.Parameter, stacked along dim 0 when more
        than one) into the flat buffer and re-point them at it."""
        dst = self.p[name]
        with torch.no_grad():
            if len(params) == 1:
                dst.copy_(params[0].data.reshape(dst.shape))
                params[0].data = dst.view(params[0].shape)
            else:
                for i, prm in enumerate(params):
                    dst[i].copy_(prm.data.reshape(dst[i].shape))
                    prm.data = dst[i].view(prm.shape)

    def adam(self, lr, target=None, tau=0.0, betas=(0.9, 0.999), eps=1e-8, part=None):
        """One optimiser step of this network alone (adam_multi with one member).  `part` = (first_part tensor
        [T, stride], n_first): the gradients of the leading n_first parameters (W1, b1) arrive as T row-tile partials
        (Stack.backward with fuse_first)."""
        adam_multi(lr, [(self, target, tau, part)], betas, eps)


def adam_multi(lr, nets, betas=(0.9, 0.999), eps=1e-8, duals=None):
    """One rrl_adam_step_multi launch over several FlatNets: nets = [(net, target or None, tau[, part]), ...];
    part = (first_part [T, stride], n_first) or None, see FlatNet.adam.  duals = [rrl_dual_t, ...]: the dual variables
    of the comparison algorithms step in the same launch (rrl_adam_step_multi_duals)."""
    lib = _lib.load()
    segs = (_lib.rrl_adam_seg_t * len(nets))()
    for k, item in enumerate(nets):
        net, target, tau = item[:3]
        part = item[3] if len(item) > 3 else None
        gp, n_part, stride, n_first = (None, 0, 0, 0) if part is None else \
            (part[0].data_ptr(), part[0].shape[0], part[0].stride(0), part[1])
        pack = net.w2p is not None and (target is None or target.w2p is not None)
        if not pack and (net.w2p is not None or (target is not None and target.w2p is not None)):
            raise _lib.RRLError("a network and its Polyak target must both keep the fragment-order W2 copy, or neither")
        segs[k] = _lib.rrl_adam_seg_t(net.flat.numel(), net.flat.data_ptr(), net.grad.data_ptr(), net.m.data_ptr(),
                                      net.v.data_ptr(), net.step.data_ptr(),
                                      None if target is None else target.flat.data_ptr(), tau, 0.0, None,
                                      gp, n_part, stride, n_first,
                                      net.w2p.data_ptr() if pack else None,
                                      target.w2p.data_ptr() if pack and target is not None else None,
                                      net.offset["W2"] if pack else 0, net.p["W2"].shape[0] if pack else 0)
    if duals:
        arr = (_lib.rrl_dual_t * len(duals))(*duals)
        record("adam_duals", segs, len(nets), arr, len(duals), float(lr), float(betas[0]), float(betas[1]), float(eps))
        _lib.check(lib.rrl_adam_step_multi_duals(len(nets), segs, len(duals), arr, lr, betas[0], betas[1], eps,
                                                 _lib.current_stream()), "rrl_adam_step_multi_duals")
        return
    record("adam", segs, len(nets), float(lr), float(betas[0]), float(betas[1]), float(eps))
    _lib.check(lib.rrl_adam_step_multi(len(nets), segs, lr, betas[0], betas[1], eps, _lib.current_stream()),
               "rrl_adam_step_multi")


def flatten_twin_q(net, device):
    """QNetwork / QNetworkConstraint -> FlatNet with heads stacked: W1 [2,H,din] ... b3 [2,1]."""
    H, din = net.linear1.weight.shape
    shapes = [("W1", (2, H, din)), ("b1", (2, H)), ("W2", (2, H, H)), ("b2", (2, H)),
              ("W3", (2, 1, H)), ("b3", (2, 1))]
    has_bn = hasattr(net, "bn1")
    if has_bn:
        shapes += [("bn_w", (din,)), ("bn_b", (din,))]
    f = FlatNet(shapes, device)
    f.adopt("W1", [net.linear1.weight, net.linear4.weight])
    f.adopt("b1", [net.linear1.bias, net.linear4.bias])
    f.adopt("W2", [net.linear2.weight, net.linear5.weight])
    f.adopt("b2", [net.linear2.bias, net.linear5.bias])
    f.adopt("W3", [net.linear3.weight, net.linear6.weight])
    f.adopt("b3", [net.linear3.bias, net.linear6.bias])
    if has_bn:
        f.adopt("bn_w", [net.bn1.weight])
        f.adopt("bn_b", [net.bn1.bias])
    f.G, f.H, f.din, f.dout = 2, H, din, 1
    return f


def flatten_policy(net, device):
    """GaussianPolicy (head = [mean; log_std], 4 rows) or StochasticPolicy (head = mean, 2 rows +
    log_std[2]) -> FlatNet with a leading head dimension of 1."""
    H, din = net.linear1.weight.shape
    gaussian = hasattr(net, "mean_linear")
    dout = 4 if gaussian else 2
    shapes = [("W1", (1, H, din)), ("b1", (1, H)), ("W2", (1, H, H)), ("b2", (1, H)),
              ("W3", (1, dout, H)), ("b3", (1, dout))]
    if not gaussian:
        shapes.append(("log_std", (2,)))
    f = FlatNet(shapes, device)
    f.adopt("W1", [net.linear1.weight])
    f.adopt("b1", [net.linear1.bias])
    f.adopt("W2", [net.linear2.weight])
    f.adopt("b2", [net.linear2.bias])
    with torch.no_grad():
        if gaussian:
            W3, b3 = f.p["W3"][0], f.p["b3"][0]
            W3[0:2].copy_(net.mean_linear.weight.data)
            W3[2:4].copy_(net.log_std_linear.weight.data)
            b3[0:2].copy_(net.mean_linear.bias.data)
            b3[2:4].copy_(net.log_std_linear.bias.data)
            net.mean_linear.weight.data, net.log_std_linear.weight.data = W3[0:2], W3[2:4]
            net.mean_linear.bias.data, net.log_std_linear.bias.data = b3[0:2], b3[2:4]
        else:
            f.adopt("W3", [net.mean.weight])
            f.adopt("b3", [net.mean.bias])
            f.adopt("log_std", [net.log_std])
    f.G, f.H, f.din, f.dout = 1, H, din, dout
    return f


class Stack:
    """Workspace + forward / backward of one 2-hidden-layer MLP stack at batch size B."""

    def __init__(self, net, B):
        self.net, self.B = net, B
        dev, G, H = net.device, net.G, net.H
        z = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)
        self.h1, self.h2, self.out = z(G, B, H), z(G, B, H), z(G, B, net.dout)
        self.dh1, self.dh2, self.dx = z(G, B, H), z(G, B, H), z(G, B, net.din)
        self.dOut = z(G, B, net.dout)               # a loss gradient that comes from a launch of its own (loss_dout)
        # partial last-layer sums of the small-batch forward: rrl_mlp3_is_split = number of parts (0: not split)
        self.nsplit = int(_lib.load().rrl_mlp3_is_split(B, H)) if mlp3_supported(H, net.din, net.dout) else 0
        self.split = self.nsplit > 0
        self.scratch = z(max(self.nsplit, 1), G, B, net.dout)
        self.finalize = False                       # True: always hand back the summed output tensor
        # False is a TEST REFERENCE (tests/test_fast_update_gpu.py): the two hidden-layer products of backward() as
        # rrl_gemm_f32 launches instead of the hidden-layer descriptor's tiles, for the bit-identity of the two
        self.pair_hidden = True
        self._folded = False
        self._init_first(dev, G, B, H, net.din)

    def _init_first(self, dev, G, B, H, din):
        """First layer of the backward inside the hidden-layer launch (rrl_first_layer_t): the 16 x 16 tiles of dh1 emit
        row-tile partials of (dW1, db1) -- laid out like the head [W1 | b1] of the flat gradient buffer, summed by
        Adam -- and column-tile partials of dx, summed by the policy-head backward.  One launch per stack backward less;
        dh1 never goes to memory."""
        self.fuse_first = B % 128 == 0 and H % 128 == 0 and B // 16 <= 64 and H // 16 <= 16
        # dx partials folded by the producer (rrl_first_layer_t.dx_fold): sums over four consecutive column tiles, H / 64
        # instead of H / 16 partials for the policy-head backward to add up -- in the paired launches (B x 4 outputs of a
        # policy head fit their dOut tile) and the block form of the packed ones; fold_dx = False keeps the tile partials
        # (the one-tile-per-workgroup launches; the consumer then sums them in the same grouped order: the same bits)
        self.fold_dx = self.fuse_first and B <= 256
        self.n_first = G * H * (din + 1)
        self.first_part = self.dx_part = None
        if self.fuse_first:
            self.first_part = torch.zeros(B // 16, self.n_first, dtype=torch.float32, device=dev)
            self.dx_part = torch.zeros(H // 16, G, B, din, dtype=torch.float32, device=dev)

    @property
    def grad_part(self):
        """What FlatNet.adam / adam_multi need to read this stack's (dW1, db1): (partials, count) or None."""
        return (self.first_part, self.n_first) if self.fuse_first else None

    def dx_parts(self):
        """(tensor [G, B, din] view of partial 0, number of partials, partial stride, group) of dL/dx after
        backward(input_grad): group = 4 -> tile partials, summed in groups of four first (rrl_loss_t.da_group)."""
        if self.fuse_first:
            n = self.dx_part.shape[0]
            return (self.dx_part[0], n // 4, self.dx_part.stride(0), 1) if self._folded else \
                (self.dx_part[0], n, self.dx_part.stride(0), 4 if n % 4 == 0 else 1)
        return self.dx, 1, 0, 1

    def forward(self, x, params=None, save=True):
        """x [B, din] shared by all heads.  `params` lets a target network reuse this workspace;
        `save` keeps the hidden activations for backward()."""
        P = (params or self.net).p
        G = self.net.G
        self.x = x
        self.parts = (self.out, 1, 0)       # (tensor, n_part, part_stride): how consumers read the output
        if mlp3_supported(self.net.H, self.net.din, self.net.dout):     # one launch for the whole stack
            record("unsupported", "rrl_mlp3_forward")
            mlp3_forward(x, P["W1"], P["b1"], P["W2"], P["b2"], P["W3"], P["b3"], out=self.out,
                         h1=self.h1 if save else None, h2=self.h2 if save else None, scratch=self.scratch,
                         finalize=self.finalize)
            if self.split and not self.finalize:   # partial last-layer sums: the consumer kernels add them up
                self.parts = (self.scratch, self.nsplit, self.scratch.stride(0))
            return self.parts
        xg = x.unsqueeze(0).expand(G, -1, -1)
        gemm(NT, xg, P["W1"], out=self.h1, bias=P["b1"], relu=True)
        gemm(NT, self.h1, P["W2"], out=self.h2, bias=P["b2"], relu=True)
        gemm(NT, self.h2, P["W3"], out=self.out, bias=P["b3"])
        return self.parts

    # -- descriptors of the same launches for the grouped entry points (rrl_*_multi) ----------------------------
    def forward_desc(self, x, params=None, save=True, in_head=None):
        """rrl_stack_t of forward(x, params, save); the caller launches it with forward_multi().  `in_head`
        (rrl_policy_head_t): columns 2..3 of x are computed by the stack kernel itself from that policy head."""
        assert mlp3_supported(self.net.H, self.net.din, self.net.dout) and not self.finalize
        P = (params or self.net).p
        net = self.net
        self.x = x
        assert x.stride(1) == 1
        self.parts = (self.scratch, self.nsplit, self.scratch.stride(0)) if self.split else (self.out, 1, 0)
        p = _lib.ptr
        if in_head is not None:
            assert self.split and net.din == 4, "the input head lives in the column-split kernels"
        w2p = (params or self.net).w2_packed() if self.split else None
        return _lib.rrl_stack_t(net.G, x.shape[0], net.H, net.din, net.dout, x.stride(0), p(x), p(P["W1"]), p(P["b1"]),
                                p(P["W2"]), p(P["b2"]), p(P["W3"]), p(P["b3"]), p(self.h1) if save else None,
                                p(self.h2) if save else None, p(self.out), p(self.scratch) if self.split else None,
                                in_head if in_head is not None else _lib.rrl_policy_head_t(), int(in_head is not None),
                                p(w2p) if w2p is not None else None)

    def backward_descs(self, dout, weight_grads=True, input_grad=False):
        """(rrl_head_bwd_t, rrl_hidden_bwd_t, rrl_input_bwd_t) of backward(dout, weight_grads, input_grad)."""
        P, Gr, net = self.net.p, self.net.g, self.net
        G, B, H = net.G, self.B, net.H
        p = _lib.ptr
        wg = weight_grads
        if isinstance(dout, _lib.rrl_loss_t):
            loss = dout
        else:
            assert dout.is_contiguous()
            loss = _lib.rrl_loss_t(-1, 1, 0, p(dout), None, None, None, None, None, None, 0.0, 0, 0, 0, None, None, 0, 0, 0)
        head = _lib.rrl_head_bwd_t(loss, G, B, H, net.dout, p(self.h2), p(P["W3"]), p(Gr["W3"]) if wg else None,
                                   p(Gr["b3"]) if wg else None, p(self.dh2))
        if self.fuse_first:
            # folded dx partials only where a folding launch is taken: a loss description (the paired launches), not a dOut tensor
            self._folded = bool(self.fold_dx and input_grad and loss.kind >= 0)
            first = _lib.rrl_first_layer_t(p(self.x), p(P["W1"]), self.x.stride(0), net.din,
                                           p(self.first_part) if wg else None, self.first_part.stride(0),
                                           p(self.dx_part) if input_grad else None, int(self._folded))
            hidden = _lib.rrl_hidden_bwd_t(G, B, H, p(self.dh2), p(self.h1), p(P["W2"]), p(Gr["W2"]) if wg else None,
                                           p(Gr["b2"]) if wg else None, None, first)
            return head, hidden, None
        hidden = _lib.rrl_hidden_bwd_t(G, B, H, p(self.dh2), p(self.h1), p(P["W2"]), p(Gr["W2"]) if wg else None,
                                       p(Gr["b2"]) if wg else None, p(self.dh1), _lib.rrl_first_layer_t())
        inp = _lib.rrl_input_bwd_t(G, B, H, net.din, self.x.stride(0), p(self.dh1), p(self.x), p(P["W1"]),
                                   p(Gr["W1"]) if wg else None, p(Gr["b1"]) if wg else None,
                                   p(self.dx) if input_grad else None)
        return head, hidden, inp

    def backward(self, dout, weight_grads=True, input_grad=False, fuse_loss=True):
        """dout: [G, B, dout] tensor, or an rrl_loss_t describing how the kernel computes it itself (fuse_loss = False:
        how the stand-alone launch of its kind computes it first, loss_dout).  Writes parameter gradients into net.g --
        (dW1, db1) as partials with fuse_first, grad_part -- (weight_grads) and/or returns dL/dx per head (input_grad):
        [G, B, din], or with fuse_first its column-tile partials (dx_parts)."""
        if not fuse_loss and isinstance(dout, _lib.rrl_loss_t):
            dout = loss_dout(dout, self.B, self.dOut)
        descs = self.backward_descs(dout, weight_grads, input_grad)
        if self.pair_hidden:
            backward_multi([descs])
        else:
            self._backward_gemm_reference(descs, weight_grads)
        if not input_grad:
            return None
        return self.dx_part if self.fuse_first else self.dx

    def _backward_gemm_reference(self, descs, weight_grads):
        """pair_hidden = False: head and input stages through their descriptors, dW2 (+ db2) and dh1 as two launches of
        the general GEMM kernel."""
        head, _, inp = descs
        assert inp is not None, "the GEMM reference writes dh1: set_fuse_first(False)"
        lib, st, P, Gr = _lib.load(), _lib.current_stream(), self.net.p, self.net.g
        _lib.check(lib.rrl_mlp_head_backward_multi(1, C.byref(head), st), "rrl_mlp_head_backward_multi")
        if weight_grads:
            gemm(TN, self.dh2, self.h1, out=Gr["W2"], colsum=Gr["b2"])
        gemm(NN, self.dh2, P["W2"], out=self.dh1, mask=self.h1)
        _lib.check(lib.rrl_mlp_input_backward_multi(1, C.byref(inp), st), "rrl_mlp_input_backward_multi")


def forward_multi(descs):
    """Independent stack forwards in ONE launch (rrl_mlp3_forward_multi)."""
    arr = (_lib.rrl_stack_t * len(descs))(*descs)
    record("forward", arr, len(descs))
    _lib.check(_lib.load().rrl_mlp3_forward_multi(len(descs), arr, _lib.current_stream()), "rrl_mlp3_forward_multi")


def backward_multi(triples):
    """Independent stack backwards, stage by stage: three launches for all of them (head, hidden, input)."""
    lib, st, n = _lib.load(), _lib.current_stream(), len(triples)
    head_list = [t[0] for t in triples]
    heads = (_lib.rrl_head_bwd_t * len(head_list))(*head_list)
    hidden = (_lib.rrl_hidden_bwd_t * n)(*[t[1] for t in triples])
    rest = [t[2] for t in triples if t[2] is not None]          # stacks whose first layer is not fused into `hidden`
    inputs = (_lib.rrl_input_bwd_t * len(rest))(*rest) if rest else None
    record("pair_bwd", heads, hidden, n)
    if inputs is not None:
        record("unsupported", "rrl_mlp_input_backward_multi")
    # head + hidden backward: one launch for the critic-loss kinds (rrl_mlp_backward_pair_multi), else the two launches
    _lib.check(lib.rrl_mlp_backward_pair_multi(n, heads, hidden, st), "rrl_mlp_backward_pair_multi")
    if inputs is not None:
        _lib.check(lib.rrl_mlp_input_backward_multi(len(inputs), inputs, st), "rrl_mlp_input_backward_multi")


def heads_multi(heads):
    """Independent policy heads (rrl_policy_head_t) in one launch; a lone head is a list of one."""
    arr = (_lib.rrl_policy_head_t * len(heads))(*heads)
    record("heads", arr, len(heads))
    _lib.check(_lib.load().rrl_policy_heads_fwd_multi(len(heads), arr, _lib.current_stream()),
               "rrl_policy_heads_fwd_multi")


def loss_dout(loss, B, dout):
    """The gradient an rrl_loss_t describes, written into the tensor `dout` [G, B, dout] by the stand-alone launch of its
    kind (rrl_loss_dout) instead of inside the head-backward kernel: what FastUpdater.fuse_loss = False runs.
    -> dout, for Stack.backward to read."""
    # the head kernels read d_action as a plain tensor: the producing backward must have written dx, not partials
    assert loss.da_parts <= 1, "fuse_loss = False needs set_fuse_first(False)"
    _lib.check(_lib.load().rrl_loss_dout(C.byref(loss), B, dout.data_ptr(), _lib.current_stream()), "rrl_loss_dout")
    return dout


class StackRows(Stack):
    """Rows [lo, hi) of a single-head Stack whose forward ran on a taller batch (several inputs of the SAME
    network stacked along the batch: one launch instead of one per input).  Shares the parent's activations and
    outputs, owns the backward workspace of its rows."""

    def __init__(self, parent, lo, hi):
        assert parent.net.G == 1, "row slices of a multi-head stack are not contiguous"
        self.parent, self.lo, self.hi = parent, lo, hi
        self.net, self.B = parent.net, hi - lo
        dev, H = parent.net.device, parent.net.H
        z = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)
        self.h1, self.h2 = parent.h1[:, lo:hi], parent.h2[:, lo:hi]
        self.dh1, self.dh2, self.dx = z(1, self.B, H), z(1, self.B, H), z(1, self.B, parent.net.din)
        self.dOut = z(1, self.B, parent.net.dout)
        self.pair_hidden = True
        self._folded = False
        self._init_first(dev, 1, self.B, H, parent.net.din)

    def forward(self, *a, **k):
        raise RuntimeError("run the parent's forward, then use .after_forward()")

    def after_forward(self):
        """(tensor, n_part, part_stride) of this slice's outputs after the parent's forward."""
        t, n_part, ps = self.parent.parts
        self.x = self.parent.x[self.lo:self.hi]
        self.parts = (t[0, 0, self.lo:self.hi] if n_part > 1 else t[0, self.lo:self.hi], n_part, ps)
        return self.parts


class FastUpdater:
    """Fused-kernel implementation of one SAC step and one Q_risk (+ model-free recovery) step for the
    default Recovery-RL configuration.  Owns the flat parameter storage of the agent's networks."""

    def __init__(self, agent, batch_size):
        self.agent = agent
        self.qr = agent.safety_critic
        self.B = B = batch_size
        dev = self.dev = agent.device
        self.lib = _lib.load()
        self.critic = flatten_twin_q(agent.critic, dev)
        self.critic_target = flatten_twin_q(agent.critic_target, dev)
        self.policy = flatten_policy(agent.policy, dev)
        self.qrisk = flatten_twin_q(self.qr.safety_critic, dev)
        self.qrisk_target = flatten_twin_q(self.qr.safety_critic_target, dev)
        self.recpolicy = flatten_policy(self.qr.policy, dev)
        z = lambda *s: torch.zeros(*s, dtype=torch.float32, device=dev)
        # stacks (workspaces) -- a network evaluated twice with saved activations needs two
        # SAC evaluates the policy on s' and on s with the same weights: one forward over 2B stacked rows
        self.pol_a = Stack(self.policy, B)
        self.pol_ab = Stack(self.policy, 2 * B)
        self.pol_next, self.pol_b = StackRows(self.pol_ab, 0, B), StackRows(self.pol_ab, B, 2 * B)
        self.cri_a, self.cri_b = Stack(self.critic, B), Stack(self.critic, B)
        self.qr_a, self.qr_b = Stack(self.qrisk, B), Stack(self.qrisk, B)
        self.rec_a = Stack(self.recpolicy, B)
        # the target networks are evaluated in the same set of forwards as the online ones: own workspaces
        self.cri_t, self.qr_t = Stack(self.critic, B), Stack(self.qrisk, B)
        # kernels that do not depend on each other share launches (rrl_*_multi): the grouped entry points exist for the
        # one-launch stack forward only (H % 16 == 0, H <= 256, <= 4 inputs / outputs); other widths (--hidden_size 512)
        # take the separate calls, whose Stack.forward falls back to the per-layer GEMM kernel
        self.grouped = all(mlp3_supported(net.H, net.din, net.dout)
                           for net in (self.critic, self.policy, self.qrisk, self.recpolicy))
        self.fuse_heads = True     # policy heads evaluated by the consuming critic stack (rrl_stack_t.in_head)
        self.xu_q, self.x2u_q, self.xpu_q = z(B, 4), z(B, 4), z(B, 4)   # the Q_risk batch's rows (drawn up front)
        self.xu = z(B, 4)                                           # [s | a]
        self.x_pol = z(2 * B, 4)                                    # [s' | a'] stacked on [s | pi]
        self.x2u, self.xpu = self.x_pol[:B], self.x_pol[B:]
        self.logp2, self.logp = z(B), z(B)
        self.losses = z(8)   # q1, q2, policy, (pad) | qr1, qr2, recpolicy, (pad)
        self.sync_world, self._avg, self.sac_bucket = 1, None, None
        self.fuse_loss = True      # loss gradients computed inside the head-backward kernels (no grad launches)
        self._noise = None
        self.keyed = False         # the last update pair took its task batch through keys drawn ahead (update_pair)
        self._noise_buf, self._actor_noise, self._actor_noise_fresh = None, None, False
        self.actor_rows = 0
        self.noise_seed = (int(getattr(agent, "seed", 0)) ^ 0x6E6F697365) & 0xFFFFFFFFFFFFFFFF
        self.noise_tick = torch.zeros(2, dtype=torch.int64, device=dev)
        self.alpha = torch.full((1,), float(agent.alpha), dtype=torch.float32, device=dev)
        self.scale = agent.policy.action_scale.to(dev).float().contiguous()
        self.bias = agent.policy.action_bias.to(dev).float().contiguous()
        self.rscale = self.qr.policy.action_scale.to(dev).float().contiguous()
        self.rbias = self.qr.policy.action_bias.to(dev).float().contiguous()
        self._init_baselines(agent, B, z)

    def _init_baselines(self, agent, B, z):
        """The comparison algorithms' terms of the SAC update (sac.py:170-277): --DGD_constraints (the Lagrangian term
        nu (max sigmoid(Q_risk(s, pi)) - eps_safe) of the policy loss), --update_nu (the nu step), --RCPO (the penalty
        lambda max sigmoid(Q_risk(s, a)) of the critic target and the lambda step).  Q_risk runs in the SAC update at its
        weights before this iteration's Q_risk step, on workspaces of its own: (s, pi) saved with an input gradient, (s, a)
        forward only."""
        dev = self.dev
        self.dgd, self.update_nu, self.rcpo = bool(agent.DGD_constraints), bool(agent.update_nu), bool(agent.RCPO)
        self.qr_p, self.qr_sa = Stack(self.qrisk, B), Stack(self.qrisk, B)
        self.penalty = z(B)
        self.dual_stats = z(4)          # mean max sigmoid(z) at (s, pi) | at (s, a) | Lagrangian policy loss | (pad)
        # the multipliers the kernels read and the dual step writes: persistent float32 device scalars (SAC._set_dual keeps
        # writing them in place)
        if self.update_nu and not torch.is_tensor(agent.nu):
            agent.nu = torch.tensor(float(agent.nu), dtype=torch.float32, device=dev)
        if self.rcpo and not torch.is_tensor(agent.lambda_RCPO):
            agent.lambda_RCPO = torch.tensor(float(agent.lambda_RCPO), dtype=torch.float32, device=dev)
        if self.dgd:
            self._join_dx(self.cri_b, self.qr_p)
        for opt, prm, on in ((agent.nu_optim, agent.log_nu, self.update_nu),
                             (agent.lambda_RCPO_optim, agent.log_lambda_RCPO, self.rcpo)):
            if on:
                dual_state(opt, prm)

    def _join_dx(self, a, b):
        """The policy loss of --DGD_constraints has two action-gradient sources, critic(s, pi) and Q_risk(s, pi): their dx
        buffers become the two halves of ONE tensor, so that one d_action description of the policy-head backward covers
        both (joint_d_action)."""
        assert a.net.H == b.net.H and a.net.din == b.net.din and a.net.G == b.net.G == 2 and a.B == b.B
        if a.first_part is not None and not a.fold_dx:
            # unfolded tile partials of two stacks are more than the head backward adds up per source: plain dx
            for st in (a, b):
                st.fuse_first, st.first_part, st.dx_part = False, None, None
        j = torch.zeros(4, a.B, a.net.din, dtype=torch.float32, device=self.dev)
        a.dx, b.dx = j[0:2], j[2:4]
        if a.dx_part is not None:
            jp = torch.zeros(2, *a.dx_part.shape, dtype=torch.float32, device=self.dev)
            a.dx_part, b.dx_part = jp[0], jp[1]

    def joint_d_action(self):
        """(d_action, (n_heads, head_stride)) of critic(s, pi) + Q_risk(s, pi) after both backwards (input_grad).  Each
        source's partials (tile t, head g) lie (2 t + g) B din floats apart, so one source is 2 t partials added one after
        the other, and the second source's block follows the first's: a fixed order, the same bits from run to run."""
        a, b = self.cri_b, self.qr_p
        B, din = a.B, a.net.din
        if a.fuse_first:
            assert b.fuse_first and a._folded == b._folded
            n = a.dx_part.shape[0] // 4 if a._folded else a.dx_part.shape[0]
            assert 2 * n <= 16
            return (a.dx_part[0], 2 * n, B * din, 1), (2, a.dx_part.numel())
        return a.dx, (4, B * din)

    def _duals(self, nu):
        """rrl_dual_t members of this SAC update's optimiser launch."""
        ag, p = self.agent, _lib.ptr
        out = []
        if self.dgd or self.update_nu:
            d = _lib.rrl_dual_t(stat=p(self.dual_stats[0:1]), eps_safe=float(ag.eps_safe), lr=float(0.1 * ag.lr))
            if self.update_nu:
                st = dual_state(ag.nu_optim, ag.log_nu)
                d.log_p, d.exp_avg, d.exp_avg_sq, d.step = p(ag.log_nu), p(st["exp_avg"]), p(st["exp_avg_sq"]), p(st["step"])
                d.value = p(ag.nu)
            if self.dgd:
                d.loss_in, d.loss_out, d.f_loss = p(self.losses[2:3]), p(self.dual_stats[2:3]), float(nu)
            out.append(d)
        if self.rcpo:
            st = dual_state(ag.lambda_RCPO_optim, ag.log_lambda_RCPO)
            out.append(_lib.rrl_dual_t(p(ag.log_lambda_RCPO), p(st["exp_avg"]), p(st["exp_avg_sq"]), p(st["step"]),
                                       p(ag.lambda_RCPO), p(self.dual_stats[1:2]), float(ag.eps_safe), float(0.1 * ag.lr),
                                       None, None, 0.0))
        return out

    def _penalty(self, z, want_penalty=True, mean=None):
        """rrl_rcpo_penalty: penalty = lambda max sigmoid(z) (want_penalty) and the batch mean of max sigmoid(z)."""
        t, n_part, ps = z
        p = _lib.ptr
        a = _lib.rrl_penalty_args_t(self.B, p(t), n_part, ps, p(self.agent.lambda_RCPO) if want_penalty else None,
                                    p(self.penalty) if want_penalty else None, p(mean))
        record("penalty", a)
        _lib.check(self.lib.rrl_rcpo_penalty(C.byref(a), _lib.current_stream()), "rrl_rcpo_penalty")

    def policy_loss(self):
        """The SAC policy loss statistic of the last update (with the Lagrangian term under --DGD_constraints, put together
        by the optimiser launch)."""
        return self.dual_stats[2] if self.dgd else self.losses[2]

    # -- helpers ---------------------------------------------------------------------------------
    def stacks(self):
        return [self.pol_a, self.pol_ab, self.pol_next, self.pol_b, self.cri_a, self.cri_b, self.cri_t, self.qr_a,
                self.qr_b, self.qr_t, self.rec_a, self.qr_p, self.qr_sa]

    def set_fuse_first(self, on):
        """First layer of every stack backward inside the hidden-layer launch (partial sums read by Adam and by the
        policy-head backward) or as its own launch writing the flat gradient buffer (needed when the gradient buffers
        are all-reduced, and by the stand-alone loss-gradient kernels of fuse_loss = False)."""
        for st in self.stacks():
            st.fuse_first = bool(on) and st.first_part is not None

    def gather_first_grads(self):
        """Write the summed (dW1, db1) partials of the last backward into the flat gradient buffers (inspection and
        tests; the optimiser reads the partials directly)."""
        for net, st in ((self.critic, self.cri_a), (self.policy, self.pol_b), (self.qrisk, self.qr_a),
                        (self.recpolicy, self.rec_a)):
            if st.fuse_first:
                net.grad[:st.n_first] = st.first_part.sum(0)

    # -- env-shard data parallelism (one learner, envs and replay split over ranks) ---------------------------
    def enable_grad_sync(self, world):
        """Every rank holds the same weights and averages gradients before each optimiser step: three
        all-reduces per iteration ([critic | policy] in one bucket, Q_risk, recovery policy -- the last two
        cannot share one because the recovery policy's gradient is taken at the UPDATED Q_risk, qrisk.py:150).
        Parameters, targets and Adam state start from rank 0's."""
        import torch.distributed as dist
        n1, n2 = self.critic.flat.numel(), self.policy.flat.numel()
        self.sac_bucket = torch.zeros(n1 + n2, dtype=torch.float32, device=self.dev)
        self.critic.rebind_grad(self.sac_bucket[:n1])
        self.policy.rebind_grad(self.sac_bucket[n1:])
        for net in (self.critic, self.critic_target, self.policy, self.qrisk, self.qrisk_target, self.recpolicy):
            dist.broadcast(net.flat, 0)
        self.sync_world = world
        self.set_fuse_first(False)              # the all-reduce works on the flat gradient buffers
        self._avg = dist.ReduceOp.AVG if dist.get_backend() == "nccl" else None

    def _sync(self, grad):
        if self.sync_world <= 1:
            return
        import torch.distributed as dist
        if self._avg is not None:
            dist.all_reduce(grad, op=self._avg)               # RCCL ring over xGMI; <= 0.8 MB: latency-bound
        else:                                                 # gloo (CPU-side reduction, tests): no AVG op
            dist.all_reduce(grad, op=dist.ReduceOp.SUM)
            grad.mul_(1.0 / self.sync_world)

    def _loss(self, kind, out, n_part, part_stride, out_t=None, v0=None, v1=None, v2=None, v3=None, alpha=None,
              f0=0.0, d_action=None, loss=None, d_heads=None):
        """rrl_loss_t for Stack.backward: the head-backward kernel evaluates the loss gradient itself.
        d_action = the critic's input gradient dx [2, B, 4] whose action columns feed a policy head; d_heads =
        (n_heads, head_stride) when it is not that tensor's two heads (joint_d_action)."""
        p = _lib.ptr
        ld = n_heads = hs = parts = ps = group = 0
        da = None
        if d_action is not None:
            if isinstance(d_action, tuple):           # Stack.dx_parts(): column-tile partials of the critic's dx
                d_action, parts, ps, group = d_action
            da, ld, n_heads, hs = d_action[0, :, 2:4].data_ptr(), d_action.stride(1), 2, d_action.stride(0)
            if d_heads is not None:
                n_heads, hs = d_heads
        return _lib.rrl_loss_t(kind, n_part, part_stride, p(out), p(out_t), p(v0), p(v1), p(v2), p(v3), p(alpha),
                               float(f0), ld, n_heads, hs, da, p(loss), parts, ps, group)

    def _load_batch(self, batch, rows_loaded=False, rows=None):
        s, a, r, s2, m = batch
        if not rows_loaded:       # the sample-gather kernel normally writes these rows itself
            xu, x2u, xpu = rows or self.rows
            xu[:, 0:2] = s
            xu[:, 2:4] = a
            x2u[:, 0:2] = s2
            xpu[:, 0:2] = s
        return s, a, r.reshape(-1), s2, m.reshape(-1)

    @property
    def rows(self):
        return (self.xu, self.x2u, self.xpu)

    @property
    def rows_q(self):
        return (self.xu_q, self.x2u_q, self.xpu_q)

    def _noise_pairs(self):
        """The noise buffer of one lock-step iteration: the 4 [B,2] draws of the two updates followed by the 2 [N,2]
        draws of the acting pass.  Hands out its views for the fill the caller is about to launch; -> the number of
        normal pairs that fill writes."""
        n_act, n_upd = self.actor_rows, 4 * self.B * 2
        need = n_upd + 2 * n_act * 2
        if self._noise_buf is None or self._noise_buf.numel() != need:
            self._noise_buf = torch.zeros(need, dtype=torch.float32, device=self.dev)
        self._noise = self._noise_buf[:n_upd].view(4, self.B, 2)
        self._actor_noise = self._noise_buf[n_upd:].view(2, n_act, 2) if n_act else None
        self._actor_noise_fresh = n_act > 0
        return need // 2

    def _fill_noise(self):
        """ONE rrl_normal_fill launch per lock-step iteration (Philox stream RRL_STREAM_NOISE, device-side tick)."""
        pairs = self._noise_pairs()
        record("unsupported", "rrl_normal_fill")
        _lib.check(self.lib.rrl_normal_fill(pairs, self.noise_seed, 0, _lib.ptr(self.noise_tick), 1,
                                            _lib.ptr(self._noise_buf), _lib.current_stream()), "rrl_normal_fill")

    def noise(self, which):
        """Policy noise for the two updates of one iteration (which = 0: the SAC update draws fresh noise for
        the whole iteration, 1: the Q_risk update uses the second half)."""
        if which == 0 or self._noise is None:
            self._fill_noise()
        n = self._noise
        return (n[0], n[1]) if which == 0 else (n[2], n[3])

    def actor_noise(self, n):
        """[2, n, 2] draws for FastActor: the tail of this iteration's fill, or its own fill when the updates did
        not run (or ran for a different n) since the last acting pass."""
        if self.actor_rows != n:
            self.actor_rows = n
            self._actor_noise_fresh = False
        if not self._actor_noise_fresh:
            self._fill_noise()
        self._actor_noise_fresh = False
        return self._actor_noise

    def _gauss_desc(self, head, eps, action_view, logp, n=None, obs_in=None, obs_out=None):
        t, n_part, ps = head
        p = _lib.ptr
        return _lib.rrl_policy_head_t(_lib.HEAD_GAUSS, n or self.B, p(t), n_part, ps, p(eps), p(self.scale),
                                      p(self.bias), p(action_view), action_view.stride(0), p(logp), None, p(obs_in),
                                      p(obs_out), None, 0.0)

    def _stoch_desc(self, head, eps, action_view, n=None):
        t, n_part, ps = head
        p = _lib.ptr
        return _lib.rrl_policy_head_t(_lib.HEAD_STOCH, n or self.B, p(t), n_part, ps, p(eps), p(self.rscale),
                                      p(self.rbias), p(action_view), action_view.stride(0), None, None, None, None,
                                      p(self.recpolicy.p["log_std"]), float(self.qr.policy.min_log_std))

    def can_draw_ahead(self):
        """The task batch's keys can be selected one env step ahead and the draw launch dissolved into the first policy
        forward's (rrl_mlp3_forward_riders): solo launches (no tape: the seed packer records the stand-alone launches), the
        column-split kernels at hidden width 256, batches that fit the forward's 256-thread workgroups."""
        return bool(_TAPE is None and self.grouped and self.sync_world == 1 and self.B <= 256 and self.pol_ab.split
                    and self.policy.H == 256 and self.recpolicy.H == 256)

    def select_ahead(self, desc, memory, rows):
        """The forward `desc` (the acting pass's recovery-policy forward, which precedes the env step) with the select half
        of the NEXT iteration's task-batch draw as a rider workgroup: the keys for the ring as it will be once the step has
        pushed its `rows` rows.  Nothing observable moves (the tick advances with the gather half)."""
        d, _ = memory.draw_desc(self.B, rows=self.rows, ahead=rows)
        sel = _lib.rrl_draw_ahead_t(C.pointer(d), rows, _lib.ptr(memory.ahead_keys(self.B)))
        riders = _lib.rrl_fwd_riders_t(C.pointer(sel), None, None, 0, 0, 0, None, 0, None)
        _lib.check(self.lib.rrl_mlp3_forward_riders(C.byref(desc), C.byref(riders), _lib.current_stream()),
                   "rrl_mlp3_forward_riders")
        memory.ahead.selected(self.B, rows)

    def update_pair(self, memory, recovery_memory, rider=None, nu=None, draw_ahead=False):
        """One SAC update and (recovery_memory not None) one Q_risk + recovery-policy update of a lock-step iteration
        (experiment.py:397-416): both replay draws and the iteration's policy noise in ONE launch, then the two
        updates on the grouped kernels.  Same draws, same arithmetic, same parameters as the separate calls.
        `rider` = (FastActor, obs): the acting pass that follows this update takes two of its three forwards along in the
        Q_risk update's launches (FastActor.ride_*; the LAST update pair of an iteration only).
        `nu`: the multiplier of the Lagrangian term (--DGD_constraints), the value SAC.update_parameters is passed.
        `draw_ahead` (one update pair per iteration, VectorLoop.draw_ahead): with the task batch's keys selected ahead
        and still valid (replay_memory.DrawAhead) there is no draw launch -- the first policy forward reads its rows
        through the keys and takes the gather, the safety buffer's draw and the noise fill along as rider workgroups
        -- and the acting pass of `rider` selects the next iteration's keys.  Same keys, same rows, same ticks."""
        B, qr = self.B, self.qr
        ahead_ok = bool(draw_ahead and rider is not None and self.can_draw_ahead())
        keyed = memory.ahead.take(B) and ahead_ok
        # a captured iteration is replayed as it is: it selects ahead only if it also consumed keys
        rider_selects = ahead_ok and (keyed or not torch.cuda.is_current_stream_capturing())
        if rider is not None:
            rider[0].select_for = (memory, rider[0].n) if rider_selects and len(memory) + rider[0].n >= B else None
        self.keyed = keyed
        d1, batch = memory.draw_desc(B, rows=self.rows)
        d2 = batch_q = None
        if recovery_memory is not None:
            d2, batch_q = recovery_memory.draw_desc(B, pos_fraction=qr.pos_fraction, rows=self.rows_q,
                                                    demo_share=qr.demo_share)
        pairs = self._noise_pairs()
        if keyed:
            gat = _lib.rrl_draw_ahead_t(C.pointer(d1), 0, _lib.ptr(memory.ahead_keys(B)))
            riders = _lib.rrl_fwd_riders_t(None, C.pointer(gat), C.pointer(d2) if d2 is not None else None, pairs,
                                           self.noise_seed, 0, _lib.ptr(self.noise_tick), 1, _lib.ptr(self._noise_buf))
            desc = self.pol_ab.forward_desc(self.x_pol[:, 0:2])
            _lib.check(self.lib.rrl_mlp3_forward_riders(C.byref(desc), C.byref(riders), _lib.current_stream()),
                       "rrl_mlp3_forward_riders")
        else:
            record("sample", _lib.rrl_sample_args_t(C.pointer(d1), C.pointer(d2) if d2 is not None else None, pairs,
                                                    self.noise_seed, 0, _lib.ptr(self.noise_tick), 1,
                                                    _lib.ptr(self._noise_buf)), d1, d2)
            _lib.check(self.lib.rrl_sample_multi(C.byref(d1), C.byref(d2) if d2 is not None else None, pairs,
                                                 self.noise_seed, 0, _lib.ptr(self.noise_tick), 1,
                                                 _lib.ptr(self._noise_buf), _lib.current_stream()), "rrl_sample_multi")
        n = self._noise
        self.sac_update(batch, n[0], n[1], rows_loaded=True, nu=nu, grouped=True, policy_forwarded=keyed)
        if recovery_memory is not None:
            self.qrisk_update(batch_q, n[2], n[3], rows_loaded=True, rows=self.rows_q, grouped=True, rider=rider)
        return self.losses

    # -- the sets of independent launches an update is made of: ONE rrl_*_multi launch each (grouped), or member by member
    #    (forwards through their stand-alone entry point, policy heads and backwards as launches of one descriptor) -- the
    #    same kernel bodies on the same inputs, the same bits either way ---------------------------------------------------
    def _forwards(self, members, grouped, riders=()):
        """Independent stack forwards: members = [(stack, x, options of Stack.forward_desc)]; `riders`: rrl_stack_t of
        another pass's forwards, in front of them in the same launch (FastActor.ride_*).  Grouped: one launch per four
        -- a lone member too where it runs the column-split kernels (the stand-alone launch's kernel body, and a launch
        the tape can pack); otherwise every member through Stack.forward."""
        if grouped and (len(members) + len(riders) > 1 or members[0][0].split):
            descs = list(riders) + [st.forward_desc(x, **opt) for st, x, opt in members]
            for k in range(0, len(descs), 4):
                forward_multi(descs[k:k + 4])
            return
        assert not riders
        for st, x, opt in members:
            assert opt.get("in_head") is None, "a policy head rides in the grouped column-split launches only"
            st.forward(x, params=opt.get("params"), save=opt.get("save", True))

    def _heads(self, heads, consumer, grouped):
        """Policy heads (rrl_policy_head_t, or None for one that is not needed) whose actions stacks like `consumer` read
        next.  Grouped on the column-split kernels nothing goes out: the heads are handed back, for the consuming stacks
        to evaluate them (in_head of _forwards).  Otherwise they are launched here -- together, or one by one -- and None
        is handed back for each."""
        if grouped and self.fuse_heads and consumer.split:
            return heads
        live = [hd for hd in heads if hd is not None]
        if grouped:
            heads_multi(live)
        else:
            for hd in live:
                heads_multi([hd])
        return [None] * len(heads)

    def _backwards(self, members, grouped):
        """Independent stack backwards with their loss descriptions: members = [(stack, rrl_loss_t, weight_grads,
        input_grad)].  Grouped: one launch per stage for all of them; a lone member, or member by member: Stack.backward
        (which is where fuse_loss = False takes the loss gradient from a launch of its own)."""
        if grouped and len(members) > 1:
            backward_multi([st.backward_descs(loss, wg, ig) for st, loss, wg, ig in members])
            return
        for st, loss, wg, ig in members:
            st.backward(loss, weight_grads=wg, input_grad=ig, fuse_loss=self.fuse_loss or grouped)

    def _nu(self, nu):
        """The multiplier of the Lagrangian term as a host float: the value passed in (the reference's nu_schedule), else
        the agent's."""
        if not self.dgd:
            return 0.0
        nu = self.agent.nu if nu is None else nu
        return float(nu)

    # -- SAC -------------------------------------------------------------------------------------
    def sac_update(self, batch, eps_next, eps_pi, rows_loaded=False, nu=None, grouped=False, policy_forwarded=False):
        """One SAC step (sac.py:170-277): at hidden 256 / batch 256 ten launches member by member, five grouped
        (update_pair; tests/test_launch_plan_cpu.py).  The comparison algorithms' Q_risk forwards join the critic forwards'
        set (a second launch when both (s, pi) and (s, a) are needed: four members at most), their backward the critic
        backwards' set, the duals the optimiser launch; the RCPO penalty is one launch more.
        `policy_forwarded`: the policy forward on (s', s) ran in the caller's launch."""
        ag, B = self.agent, self.B
        nu = self._nu(nu)
        s, a, r, s2, m = self._load_batch(batch, rows_loaded)
        # pi(s') and pi(s) share the weights (both gradients are taken before either step): ONE policy forward
        if not policy_forwarded:
            self._forwards([(self.pol_ab, self.x_pol[:, 0:2], {})], grouped)
        head2, head = self.pol_next.after_forward(), self.pol_b.after_forward()
        # a' ~ pi(s') for the target min Q_target(s', a') - alpha log pi (sac.py:192-201) and pi(s) for the policy loss
        hd2, hd1 = self._heads([self._gauss_desc(head2, eps_next, self.x2u[:, 2:4], self.logp2),
                                self._gauss_desc(head, eps_pi, self.xpu[:, 2:4], self.logp)], self.cri_t, grouped)
        # critic_target(s', a'), critic(s, a), critic(s, pi): three independent forwards (sac.py:192-218); the policy loss is
        # taken at the PRE-update critic (both gradients before either step)
        fwd = [(self.cri_t, self.x2u, dict(params=self.critic_target, save=False, in_head=hd2)),
               (self.cri_a, self.xu, {}), (self.cri_b, self.xpu, dict(in_head=hd1))]
        if self.dgd or self.update_nu:      # Q_risk(s, pi) at its pre-update weights: pi evaluated by this stack too, written
            hq = None                       # by the critic's only
            if hd1 is not None:
                hq = _lib.rrl_policy_head_t.from_buffer_copy(hd1)
                hq.action, hq.logp = None, None
            fwd.append((self.qr_p, self.xpu, dict(save=self.dgd, in_head=hq)))
        if self.rcpo:
            fwd.append((self.qr_sa, self.xu, dict(save=False)))
        self._forwards(fwd, grouped)
        qt, n_part, ps = self.cri_t.parts
        q, qp = self.cri_a.parts[0], self.cri_b.parts[0]
        if self.rcpo:                                                  # lambda max sigmoid(Q_risk(s, a)) (sac.py:202-205)
            self._penalty(self.qr_sa.parts, mean=self.dual_stats[1:2])
        if self.update_nu and not self.dgd:
            self._penalty(self.qr_p.parts, want_penalty=False, mean=self.dual_stats[0:1])
        # the critic's backward for its own loss (weight gradients, sac.py:233-235) and for the policy loss (input gradient)
        members = [
            (self.cri_a, self._loss(_lib.LOSS_SAC_CRITIC, q, n_part, ps, out_t=qt, v0=self.logp2, v1=r, v2=m,
                                    v3=self.penalty if self.rcpo else None, alpha=self.alpha, f0=ag.gamma,
                                    loss=self.losses), True, False),
            (self.cri_b, self._loss(_lib.LOSS_SAC_POLICY, qp, n_part, ps, v0=self.logp, alpha=self.alpha,
                                    loss=self.losses[2:]), False, True)]
        if self.dgd:
            members.append((self.qr_p, self._loss(_lib.LOSS_DGD_QRISK, *self.qr_p.parts, f0=nu, loss=self.dual_stats[0:1]),
                            False, True))
        self._backwards(members, grouped)
        # d pi = action columns of dx [2,B,4], summed over the two critic heads inside the policy's head backward
        # (and over Q_risk's two after them: joint_d_action)
        ht, hn, hs = head
        da, dh = self.joint_d_action() if self.dgd else (self.cri_b.dx_parts(), None)
        self._backwards([(self.pol_b, self._loss(_lib.LOSS_GAUSS_HEAD, ht, hn, hs, v0=eps_pi, v1=self.scale,
                                                 f0=float(ag.alpha) / B, d_action=da, d_heads=dh), True, False)], grouped)
        if self.sync_world > 1:
            self._sync(self.sac_bucket)
        # both optimiser steps + the soft target update (:273-274) in one launch (+ the duals)
        adam_multi(ag.lr, [(self.critic, self.critic_target, ag.tau, self.cri_a.grad_part),
                           (self.policy, None, 0.0, self.pol_b.grad_part)], duals=self._duals(nu))
        return self.losses

    def can_carry_actor(self):
        """The acting pass's task-policy and Q_risk forwards can ride in the grouped Q_risk update's forward launches
        (qrisk_update): model-free recovery, policy heads evaluated by the consuming stacks, every stack on the column-split
        kernels."""
        return bool(self.grouped and self.qr.MF_recovery and self.fuse_heads and self.qr_t.split and self.qr_b.split
                    and self.pol_a.split and self.rec_a.split and self.sync_world == 1)

    # -- Q_risk ------------------------------------------------------------------------------------
    def qrisk_update(self, batch, eps_next, eps_pi, rows_loaded=False, rows=None, grouped=False, rider=None):
        """One Q_risk step and (MF_recovery) one recovery-policy step (qrisk.py:86-163) on the row buffers `rows` (default:
        the ones the SAC update works on): at hidden 256 / batch 256 twelve launches member by member, eight grouped -- the
        task policy on s' and the recovery policy on s in one forward launch (the recovery policy does not depend on the
        critic step in between), the target and online critics in one, the heads inside the stacks that read their actions.
        rider = (FastActor, obs) (grouped, can_carry_actor()): the acting pass that follows needs the task policy on the N
        observations -- final since the SAC step -- and Q_risk(obs, a_task) -- final since this update's critic step: the
        first rides in this update's first forward launch, the second in its forward at the updated critic.  The acting pass
        is left with the recovery policy's forward (final only after this update's last step): 17 -> 16 launches per
        iteration, and the two 256-row launches that waited alone on the chip run under the 4096-row ones.  Same kernels,
        same inputs: same bits."""
        qr = self.qr
        xu, x2u, xpu = rows = rows or self.rows
        s, a, c, s2, m = self._load_batch(batch, rows_loaded, rows)
        mf = bool(qr.MF_recovery)
        assert rider is None or self.can_carry_actor()
        fwd = [(self.pol_a, x2u[:, 0:2], dict(save=False))]                # a' from the TASK policy (qrisk.py:119-120)
        if mf:
            fwd.append((self.rec_a, xpu[:, 0:2], {}))
        # the rider: the large member first (mlp_fwd_kernels.hip: measured forms)
        self._forwards(fwd, grouped, riders=[rider[0].ride_policy(rider[1])] if rider else ())
        hd_next, hd_rec = self._heads([self._gauss_desc(self.pol_a.parts, eps_next, x2u[:, 2:4], self.logp2),
                                       self._stoch_desc(self.rec_a.parts, eps_pi, xpu[:, 2:4]) if mf else None],
                                      self.qr_t, grouped)
        self._forwards([(self.qr_t, x2u, dict(params=self.qrisk_target, save=False, in_head=hd_next)),
                        (self.qr_a, xu, {})], grouped)
        zt, n_part, ps = self.qr_t.parts
        z = self.qr_a.parts[0]
        self._backwards([(self.qr_a, self._loss(_lib.LOSS_QRISK_CRITIC, z, n_part, ps, out_t=zt, v0=c, v1=m,
                                                f0=qr.gamma_safe, loss=self.losses[4:]), True, False)], grouped)
        self._sync(self.qrisk.grad)
        self.qrisk.adam(qr.lr, target=self.qrisk_target, tau=qr.tau, part=self.qr_a.grad_part)
        if mf:                                                             # qrisk.py:150-158, at the UPDATED critic
            raw, rn, rs = self.rec_a.parts
            ls = self.recpolicy.p["log_std"]
            self._forwards([(self.qr_b, xpu, dict(in_head=hd_rec))], grouped,
                           riders=[rider[0].ride_qrisk()] if rider else ())
            zp, n_part, ps = self.qr_b.parts
            self._backwards([(self.qr_b, self._loss(_lib.LOSS_QRISK_POLICY, zp, n_part, ps, loss=self.losses[6:]),
                              False, True)], grouped)
            self._backwards([(self.rec_a, self._loss(_lib.LOSS_STOCH_HEAD, raw, rn, rs, v0=eps_pi, v1=ls, v2=self.rscale,
                                                     f0=qr.policy.min_log_std, d_action=self.qr_b.dx_parts(),
                                                     loss=self.recpolicy.g["log_std"]), True, False)], grouped)
            self._sync(self.recpolicy.grad)
            self.recpolicy.adam(qr.lr, part=self.rec_a.grad_part)
        return self.losses


# The acting launches of the SQRL and Q-sampling lines: (line, gate inside the call, f16x3 scores) -> (tape kind, entry point).
# The packed entry of a kind (packed.PackedLoop) is the stand-alone name plus "_packed"; the gated entries' drops "_gated" (the
# packed Q-sampling stage exists with the gate inside it only).
ACT_ENTRIES = {("sqrl", False, False): ("sqrl", "rrl_sqrl_act"),
               ("sqrl", False, True): ("sqrl_f16x3", "rrl_sqrl_act_f16x3"),
               ("qsample", False, False): ("qsample", "rrl_qsample_act"),
               ("qsample", True, False): ("qsample", "rrl_qsample_act_gated"),
               ("qsample", False, True): ("qsample_f16x3", "rrl_qsample_act_f16x3"),
               ("qsample", True, True): ("qsample_f16x3", "rrl_qsample_act_gated_f16x3")}
ACT_PACKED = {kind: entry.replace("_gated", "") + "_packed" for kind, entry in ACT_ENTRIES.values()}


class FastActor:
    """Batched get_action (experiment.py:546-577) for N envs on the fused kernels: task policy sample,
    Q_risk of (s, a_task), model-free recovery action and the recovery gate -- 8 launches instead of
    ~60 PyTorch ones."""

    def __init__(self, fast, n):
        self.f, self.n = fast, n
        dev = fast.dev
        z = lambda *s: torch.zeros(*s, dtype=torch.float32, device=dev)
        self.pol, self.qr, self.rec = Stack(fast.policy, n), Stack(fast.qrisk, n), Stack(fast.recpolicy, n)
        self.xa = z(n, 4)                       # [s | a_task]
        self.task_action, self.rec_action, self.real_action = z(n, 2), z(n, 2), z(n, 2)
        self.recovery = torch.zeros(n, dtype=torch.uint8, device=dev)
        self._ride = None
        self.select_for = None          # (task buffer, rows): the next draw's keys are selected in this pass's last forward
        # SQRL constraint sampling (act_sqrl): Philox seed (the loop sets its own) and the device tick {tick, ticket}
        self.sqrl_seed = int(getattr(fast.agent, "seed", 0)) & 0xFFFFFFFFFFFFFFFF
        self.sqrl_tick = torch.zeros(2, dtype=torch.int64, device=dev)
        # RRL_SQRL_F16X3=1 (the loop sets it when it is built): act_sqrl scores on rrl_sqrl_act_f16x3, from a hi / lo stream of
        # Q_risk's W2 this actor owns (sqrl_w2h, made at the first pass)
        self.sqrl_f16x3 = False
        self.sqrl_w2h = None
        # Q-sampling recovery (act_qsample): seed and device tick likewise, the action box on the device, the launch's scratch
        self.qsample_seed = self.sqrl_seed
        self.qsample_tick = torch.zeros(2, dtype=torch.int64, device=dev)
        ac = getattr(fast.qr, "ac_space", None)
        self.qsample_box = None if ac is None else tuple(
            torch.as_tensor(b, dtype=torch.float32, device=dev).contiguous() for b in (ac.low, ac.high))
        self._qsample_scratch = None
        # RRL_QSAMPLE_F16X3=1 (the loop sets it when it is built): act_qsample scores on rrl_qsample_act_f16x3, from a hi / lo
        # stream of Q_risk's W2 this actor owns (qsample_w2h, made at the first pass)
        self.qsample_f16x3 = False
        self.qsample_w2h = None

    # -- two of the three forwards of act(defer_select=True) as riders of the Q_risk update's launches -----------------------
    def ride_policy(self, obs):
        """rrl_stack_t of the task policy's forward on the acting observations, for a launch the caller issues (any time after
        the SAC step of this iteration).  Starts a ride: ride_qrisk() and act() complete it."""
        assert obs.shape[0] == self.n and self.f.can_carry_actor() and self.qr.split
        self._ride = {"obs": obs, "noise": self.f.actor_noise(self.n), "qrisk": False}
        return self.pol.forward_desc(obs, save=False)

    def ride_qrisk(self):
        """rrl_stack_t of Q_risk(obs, a_task) with the task head evaluated by the stack (it stores the action in xa for the
        step kernel), for a launch the caller issues after the policy rider's launch and the safety critic's step."""
        r = self._ride
        self.qr.finalize = False
        r["qrisk"] = True
        return self.qr.forward_desc(self.xa, save=False, in_head=self._task_head(r["noise"][0], r["obs"]))

    def _finish_ride(self, obs, eps_safe):
        """What is left of act(defer_select=True) after both riders: the recovery policy's forward (its step is the last of
        the iteration's updates); its head and the gate run in the env-step kernel."""
        f, r = self.f, self._ride
        self._ride = None
        assert r["qrisk"] and obs is r["obs"], "the acting pass of a ride must follow its two riders, on the same observations"
        sel, self.select_for = self.select_for, None
        if sel is not None:
            f.select_ahead(self.rec.forward_desc(obs, save=False), *sel)
        else:
            forward_multi([self.rec.forward_desc(obs, save=False)])
        return self._deferred(eps_safe, rec_head=f._stoch_desc(self.rec.parts, r["noise"][1], self.rec_action, n=self.n))

    def _deferred(self, eps_safe, rec_action=None, rec_head=None):
        """The gate left to the env-step kernel: its inputs -- Q_risk(s, a_task) as the last forward left it, the recovery
        action or the head that yields it -- in `pending_select`, the buffers that kernel fills as the result."""
        self.pending_select = (*self.qr.parts, float(eps_safe), rec_action, rec_head)
        return self.xa[:, 2:4], self.real_action, self.recovery

    def _task_head(self, eps, obs):
        """The task policy's head on this pass's forward.  It also copies obs into columns 0..1 of xa: [s | a_task] is
        assembled without a copy launch."""
        return self.f._gauss_desc(self.pol.parts, eps, self.xa[:, 2:4], None, n=self.n, obs_in=obs, obs_out=self.xa)

    def _gate(self, eps_safe):
        """Q_risk(s, a_task) on xa, then recovery[i] = max(sigmoid(z1), sigmoid(z2)) > eps_safe and the action select
        (experiment.py:566-571) -> (task action, executed action, recovery)."""
        self.qr.finalize = True                  # recovery_select reads a plain [2,n] tensor
        zq, _, _ = self.qr.forward(self.xa, save=False)
        _lib.check(self.f.lib.rrl_recovery_select(self.n, zq.data_ptr(), eps_safe, self.xa[:, 2:4].data_ptr(), 4,
                                                  self.rec_action.data_ptr(), self.real_action.data_ptr(),
                                                  self.recovery.data_ptr(), self.task_action.data_ptr(),
                                                  _lib.current_stream()), "rrl_recovery_select")
        return self.task_action, self.real_action, self.recovery

    def act(self, obs, eps_safe, use_recovery, mf_recovery, noise=None, defer_select=False):
        """-> (task action [n,2], executed action [n,2], recovery u8[n] or None); persistent buffers.
        defer_select: the recovery gate is left to the env-step kernel (rrl_step_push_t.sel_*); `pending_select` then
        holds its inputs, the task action is the strided view xa[:, 2:4] and the other two are filled by that kernel."""
        f, n = self.f, self.n
        self.pending_select = None
        if self._ride is not None:
            assert noise is None and defer_select and use_recovery and mf_recovery
            return self._finish_ride(obs, eps_safe)
        if noise is None:
            noise = f.actor_noise(n)
        if not use_recovery:
            # (grouped, on the column-split kernels: the stand-alone launch's kernel body through the group entry point, a launch
            # the tape can pack)
            f._forwards([(self.pol, obs, dict(save=False))], f.grouped)
            heads_multi([f._gauss_desc(self.pol.parts, noise[0], self.task_action, None, n=n)])
            return self.task_action, self.task_action, None
        assert mf_recovery, "FastActor covers the model-free recovery policy"
        grouped = f.grouped
        # task policy and recovery policy on the same observations: one forward launch, one head launch (grouped)
        f._forwards([(self.pol, obs, dict(save=False)), (self.rec, obs, dict(save=False))], grouped)
        task_head = self._task_head(noise[0], obs)
        rec_head = f._stoch_desc(self.rec.parts, noise[1], self.rec_action, n=n)
        defer_select = defer_select and grouped
        if defer_select and f.fuse_heads and self.qr.split:
            # no head launch: the task action is evaluated by the Q_risk stack that consumes it (and stored in xa
            # for the step kernel), the recovery action by the step kernel itself
            self.qr.finalize = False
            forward_multi([self.qr.forward_desc(self.xa, save=False, in_head=task_head)])
            return self._deferred(eps_safe, rec_head=rec_head)
        if grouped:
            heads_multi([task_head, rec_head])
        else:
            heads_multi([task_head]), heads_multi([rec_head])
        if defer_select:
            self.qr.finalize = False            # the step kernel adds the partial last-layer sums itself
            self.qr.forward(self.xa, save=False)
            return self._deferred(eps_safe, rec_action=self.rec_action)
        return self._gate(eps_safe)

    def act_sqrl(self, obs, eps_safe, k=100, eps=None, u=None, diag=None):
        """SQRL constraint sampling (SAC._sqrl_action) for the n envs on the fused kernels: the task policy's forward at n rows
        (its head is the same for an env's k candidates), then ONE rrl_sqrl_act launch -- candidates, twin Q_risk on the
        n k rows, pick -- that draws on its own Philox streams at this actor's device tick.  -> the persistent task_action
        buffer.  `eps` [n, k, 2] f32 / `u` [n] f64 inject the draws, `diag` = {name: tensor} asks for the kernel's
        diagnostic outputs (q, logp, cand, z, pick, cstar, n_safe) -- tests."""
        f, n = self.f, self.n
        assert obs.shape == (n, 2) and obs.is_contiguous()
        self.pending_select = None
        w2p = f.qrisk.w2_packed()
        if w2p is None or f.qrisk.H != 256:
            raise _lib.RRLError("rrl_sqrl_act needs Q_risk at hidden width 256 with its fragment-order W2 copy")
        f._forwards([(self.pol, obs, dict(save=False))], f.grouped)
        head, n_part, ps = self.pol.parts
        p, P, d = _lib.ptr, f.qrisk.p, diag or {}
        a = _lib.rrl_sqrl_act_t(n=n, k=k, H=f.qrisk.H, d_obs=2, d_act=2, obs=p(obs), head=p(head), n_part=n_part,
                                part_stride=ps, scale=p(f.scale), bias=p(f.bias), W1=p(P["W1"]), b1=p(P["b1"]), W2p=p(w2p),
                                b2=p(P["b2"]), W3=p(P["W3"]), b3=p(P["b3"]), eps_safe=float(eps_safe), seed=self.sqrl_seed,
                                counter=0, counter_dev=p(self.sqrl_tick), counter_inc=1, eps_in=p(eps), u_in=p(u),
                                action=p(self.task_action), **{name: p(t) for name, t in d.items()})
        self._sqrl_args = a              # keeps the argument block alive until the launch has been issued (and for profiles/)
        if self.sqrl_f16x3:
            self._f16x3_stream(a, "sqrl_w2h")
        self._launch("sqrl", False, self.sqrl_f16x3, a)
        return self.task_action

    def _f16x3_stream(self, a, attr):
        """Layer 2 of the scores of descriptor `a` in f16x3: the hi / lo fragment stream of Q_risk's live W2 (this actor's `attr`,
        made at the first pass) takes the place of a.W2p and is re-made in front of every launch (inside the captured graph; no
        optimiser launch keeps it current) by a call the tape records."""
        f, W2 = self.f, self.f.qrisk.p["W2"]
        if getattr(self, attr) is None:
            setattr(self, attr, torch.empty(W2.numel(), dtype=torch.float32, device=f.dev))
        w2h = getattr(self, attr)
        a.W2p = _lib.ptr(w2h)
        pack = (W2.shape[0], W2.shape[1], _lib.ptr(W2), _lib.ptr(w2h))
        record("call", f.lib.rrl_w2_pack_f16x3, pack, (W2, w2h))
        _lib.check(f.lib.rrl_w2_pack_f16x3(*pack, _lib.current_stream()), "rrl_w2_pack_f16x3")

    def _launch(self, line, gated, f16x3, *blocks):
        """The acting launch of `line` on its argument blocks: recorded under its tape kind, issued and checked (ACT_ENTRIES)."""
        kind, entry = ACT_ENTRIES[line, bool(gated), bool(f16x3)]
        record(kind, *blocks)
        _lib.check(getattr(self.f.lib, entry)(*map(C.byref, blocks), _lib.current_stream()), entry)

    def act_qsample(self, obs, eps_safe, k=1000, cand=None, diag=None, gated=False):
        """Q-sampling recovery (QRiskWrapper.select_action, qrisk.py:214-225) for the n envs on the fused kernels: the sequence of
        act_gate -- the task policy's forward and head, the Q_risk gate -- which leaves task_action, real_action = task_action
        and recovery, then ONE rrl_qsample_act call on the gated envs: k uniform candidates from the action box on the
        actor's own Philox stream and device tick, the twin Q_risk on each, the argmin into real_action.
        -> (task action, executed action, recovery u8[n]); persistent buffers.  `cand` [n, k, 2] f32 injects the candidates,
        `diag` = {name: tensor} asks for the launch's diagnostic outputs (q, z, cand, pick) -- tests.
        gated (RRL_PACK_QSAMPLE=1, pack_qsample_enabled): the same pass as three calls the launch tape records -- the task
        policy's forward, Q_risk on [s | a_task] left as partial last-layer sums with the task head evaluated by the stack,
        and rrl_qsample_act_gated, which evaluates the gate from those sums itself.  Same noise, same Philox stream, same
        tick, same bits in the three buffers."""
        f, n = self.f, self.n
        assert obs.shape == (n, 2) and obs.is_contiguous()
        w2p = f.qrisk.w2_packed()
        if w2p is None or f.qrisk.H != 256:
            raise _lib.RRLError("rrl_qsample_act needs Q_risk at hidden width 256 with its fragment-order W2 copy")
        if gated:
            gate = self._qsample_gate(obs, eps_safe)
        else:
            self.act_gate(obs, eps_safe)
        floats = int(f.lib.rrl_qsample_scratch_floats(n, k))
        if floats < 0:
            _lib.check(floats, "rrl_qsample_scratch_floats")
        if self._qsample_scratch is None or self._qsample_scratch.numel() < floats:
            self._qsample_scratch = torch.empty(max(floats, 1), dtype=torch.float32, device=f.dev)
        lo, hi = self.qsample_box
        p, P, d = _lib.ptr, f.qrisk.p, diag or {}
        a = _lib.rrl_qsample_act_t(n=n, k=k, H=f.qrisk.H, d_obs=2, d_act=2, obs=p(obs), mask=None if gated else p(self.recovery),
                                   lo=p(lo), hi=p(hi),
                                   W1=p(P["W1"]), b1=p(P["b1"]), W2p=p(w2p), b2=p(P["b2"]), W3=p(P["W3"]), b3=p(P["b3"]),
                                   seed=self.qsample_seed, counter=0, counter_dev=p(self.qsample_tick), counter_inc=1,
                                   cand_in=p(cand), scratch=p(self._qsample_scratch), action=p(self.real_action),
                                   **{name: p(t) for name, t in d.items()})
        self._qsample_args = a           # keeps the argument block alive until the launch has been issued (and for profiles/)
        if self.qsample_f16x3:
            self._f16x3_stream(a, "qsample_w2h")
        if gated:
            self._qsample_gate_args = gate
        self._launch("qsample", gated, self.qsample_f16x3, *((a, gate) if gated else (a,)))
        return self.task_action, self.real_action, self.recovery

    def _qsample_gate(self, obs, eps_safe):
        """The forwards of act_gate through the entry points the launch tape records, the gate itself left to the qsample
        call: -> its rrl_qsample_gate_t, reading Q_risk(s, a_task) as this pass's forward leaves it (qr.parts)."""
        f, n = self.f, self.n
        noise = f.actor_noise(n)
        self.pending_select = None
        f._forwards([(self.pol, obs, dict(save=False))], f.grouped)
        task_head = self._task_head(noise[0], obs)
        self.qr.finalize = False                 # the qsample kernels add the partial last-layer sums themselves
        if f.fuse_heads and self.qr.split:
            # no head launch: the task action is evaluated by the Q_risk stack that consumes it (and stored in xa)
            forward_multi([self.qr.forward_desc(self.xa, save=False, in_head=task_head)])
        else:
            heads_multi([task_head])
            forward_multi([self.qr.forward_desc(self.xa, save=False)])
        z, n_part, ps = self.qr.parts
        p = _lib.ptr
        return _lib.rrl_qsample_gate_t(z=p(z), n_part=n_part, part_stride=ps, eps_safe=float(eps_safe),
                                       task_action=p(self.xa[:, 2:4]), ld_task=4, task_out=p(self.task_action),
                                       recovery_out=p(self.recovery))

    def act_gate(self, obs, eps_safe, noise=None):
        """Task action + recovery gate for a controller that acts elsewhere (model-based recovery: MPC.act on the gated rows):
        -> (task action [n,2], recovery u8[n]); persistent buffers."""
        if noise is None:
            noise = self.f.actor_noise(self.n)
        self.pending_select = None
        self.pol.forward(obs, save=False)
        heads_multi([self._task_head(noise[0], obs)])
        # the kernel's action selection runs on a dummy recovery action: the planner's action is merged in by the caller
        task, _, recovery = self._gate(eps_safe)
        return task, recovery


def dual_state(opt, param):
    """torch.optim.Adam's state of a dual variable (capturable: `step` a float32 device scalar), created up front in
    torch's own format: the fused dual step (rrl_adam_step_multi_duals) reads and writes these tensors, so state_dict(),
    checkpoints and a later autograd step see them as torch would have left them."""
    st = opt.state[param]
    if len(st) == 0:
        st["step"] = torch.zeros((), dtype=torch.float32, device=param.device)
        st["exp_avg"] = torch.zeros_like(param, memory_format=torch.preserve_format)
        st["exp_avg_sq"] = torch.zeros_like(param, memory_format=torch.preserve_format)
    return st


class EvalRollout:
    """One evaluation (Experiment.get_test_rollout_vectorized) of `env`'s envs as one rrl_eval_rollout launch on the live flat
    weights of `fast`.  Owns the per-env result buffers and its OWN fragment-order copies of the three W2 matrices, re-made
    right before each launch: it depends neither on RRL_W2_FRAG nor on how many seeds a packed run keeps those copies for.
    qsample=True: the Q-sampling form (rrl_eval_rollout_qs) -- no recovery policy; a gated row executes the best of QSAMPLE_K
    uniform candidates from the action box FastActor.qsample_box takes, drawn inside the launch.
    sqrl=True: the SQRL form (rrl_eval_rollout_sqrl) -- no gate and no recovery policy; every live row executes the pick
    among SQRL_K candidates of the task policy's head (its four stacked last-layer rows), scored by Q_risk inside the launch.
    f16x3=True (with qsample or sqrl): the candidates are scored in f16x3 (rrl_eval_rollout_qs_f16x3 / _sqrl_f16x3) on a
    rrl_w2_pack_f16x3 stream of Q_risk's W2 that is owned here and re-made right before each launch, as the W2 copies are."""

    QSAMPLE_K = 1000                   # QRiskWrapper.select_action's candidate count
    SQRL_K = 100                       # SAC._sqrl_action's

    def __init__(self, fast, env, eps_safe, use_recovery, qsample=False, sqrl=False, f16x3=False):
        self.f, self.env, self.n = fast, env, env.num_envs
        self.eps_safe, self.use_recovery, self.qsample = float(eps_safe), bool(use_recovery), bool(qsample)
        self.sqrl, self.f16x3 = bool(sqrl), bool(f16x3)
        if self.sqrl and (self.use_recovery or self.qsample):
            raise _lib.RRLError("rrl_eval_rollout_sqrl: SQRL without a recovery policy only")
        if self.f16x3 and not (self.sqrl or self.qsample):
            raise _lib.RRLError("f16x3 evaluation scoring: the Q-sampling and SQRL forms only (they score candidates)")
        dev = fast.dev
        self.ret = torch.zeros(self.n, dtype=torch.float32, device=dev)
        self.success = torch.zeros(self.n, dtype=torch.uint8, device=dev)
        self.violation = torch.zeros(self.n, dtype=torch.uint8, device=dev)
        self.steps = torch.zeros(self.n, dtype=torch.int32, device=dev)
        self.nets = [fast.policy] + ([fast.qrisk] + ([] if self.qsample else [fast.recpolicy]) if self.use_recovery else [])
        if self.sqrl:
            self.nets = [fast.policy, fast.qrisk]
        if self.qsample:
            ac = fast.qr.ac_space
            self.box = tuple(torch.as_tensor(b, dtype=torch.float32, device=dev).contiguous() for b in (ac.low, ac.high))
        self.w2p = [torch.empty(net.p["W2"].numel(), dtype=torch.float32, device=dev) for net in self.nets]
        self.qw2h = torch.empty(fast.qrisk.p["W2"].numel(), dtype=torch.float32, device=dev) if self.f16x3 else None
        self.args = None

    def desc(self, T, reset=True, pos=None, trace=None):
        """The launch's rrl_eval_rollout_t (the Q-sampling form: rrl_eval_rollout_qs_t around it) on the live flat buffers and
        the env's seed and device tick, the W2 copies made current.  `pos` [n, 2] f64 with reset=False: the start states;
        `trace` = {name: tensor} asks for trace buffers."""
        trace = dict(trace or {})
        own = {name: trace.pop(name) for name in ("tr_pick", "tr_q", "tr_head", "tr_cstar", "tr_nsafe") if name in trace}
        f, p = self.f, _lib.ptr
        for net, w2p in zip(self.nets, self.w2p):
            W2 = net.p["W2"]
            _lib.check(f.lib.rrl_w2_pack(W2.shape[0], W2.shape[1], W2.data_ptr(), w2p.data_ptr(), _lib.current_stream()),
                       "rrl_w2_pack")
        if self.f16x3:
            W2 = f.qrisk.p["W2"]
            _lib.check(f.lib.rrl_w2_pack_f16x3(W2.shape[0], W2.shape[1], W2.data_ptr(), self.qw2h.data_ptr(),
                                               _lib.current_stream()), "rrl_w2_pack_f16x3")
        P = f.policy.p
        a = _lib.rrl_eval_rollout_t(n=self.n, T=int(T), H=f.policy.H, d_obs=2, d_act=2, env_kind=self.env.kind,
                                    reset=int(bool(reset)), pos=p(pos), pW1=p(P["W1"]), pb1=p(P["b1"]), pW2p=p(self.w2p[0]),
                                    pb2=p(P["b2"]), pW3=p(P["W3"]), pb3=p(P["b3"]), scale=p(f.scale), bias=p(f.bias),
                                    seed=self.env.seed_value, counter=0, counter_dev=p(self.env.tick), ret=p(self.ret),
                                    success=p(self.success), violation=p(self.violation), steps=p(self.steps),
                                    **{name: p(t) for name, t in (trace or {}).items()})
        if self.use_recovery or self.sqrl:
            Q = f.qrisk.p
            a.qW1, a.qb1, a.qW2p, a.qb2, a.qW3, a.qb3 = (p(Q["W1"]), p(Q["b1"]), p(self.w2p[1]), p(Q["b2"]), p(Q["W3"]),
                                                         p(Q["b3"]))
            a.eps_safe = self.eps_safe
        if self.sqrl:
            a = _lib.rrl_eval_rollout_sqrl_t(base=a, k=self.SQRL_K, horizon=int(self.env.horizon) if self.maze else 0,
                                             **{name: p(t) for name, t in own.items()})
        elif self.qsample:
            a = _lib.rrl_eval_rollout_qs_t(base=a, k=self.QSAMPLE_K, horizon=int(self.env.horizon) if self.maze else 0,
                                           lo=p(self.box[0]), hi=p(self.box[1]), **{name: p(t) for name, t in own.items()})
        elif self.use_recovery:
            R = f.recpolicy.p
            a.rW1, a.rb1, a.rW2p, a.rb2, a.rW3, a.rb3 = (p(R["W1"]), p(R["b1"]), p(self.w2p[2]), p(R["b2"]), p(R["W3"]),
                                                         p(R["b3"]))
            a.rscale, a.rbias, a.rlog_std = p(f.rscale), p(f.rbias), p(R["log_std"])
            a.min_log_std = f.qr.policy.min_log_std
        self.args = a              # keeps the argument block alive until the launch has been issued
        return a

    @property
    def maze(self):
        return self.env.kind == _lib.ENV_MAZE

    @property
    def entry(self):
        """(entry, descriptor type, side) of this rollout's form: the stand-alone entry's name -- the packed one is that name +
        "_packed" --, the descriptor it takes, and what rides beside the descriptor (per seed, in a packed launch): None, the
        env's own horizon for the base form on Maze (it ends a row; T stays horizon + 1) or the f16x3 stream.  The Q-sampling
        and SQRL forms have one entry for both env families: the Maze horizon rides in their descriptor."""
        if self.sqrl or self.qsample:
            name, desc_t = (("rrl_eval_rollout_sqrl", _lib.rrl_eval_rollout_sqrl_t) if self.sqrl else
                            ("rrl_eval_rollout_qs", _lib.rrl_eval_rollout_qs_t))
            return (name + "_f16x3", desc_t, C.c_void_p(self.qw2h.data_ptr())) if self.f16x3 else (name, desc_t, None)
        if self.maze:
            return "rrl_eval_rollout_maze", _lib.rrl_eval_rollout_t, C.c_int(int(self.env.horizon))
        return "rrl_eval_rollout", _lib.rrl_eval_rollout_t, None

    def launch(self, T, **kw):
        a = self.desc(T, **kw)
        name, _, side = self.entry
        _lib.check(getattr(self.f.lib, name)(C.byref(a), *([] if side is None else [side]), _lib.current_stream()), name)

    def stats(self, label):
        """The three means of the per-env arrays, as the module path takes them."""
        return {"label": label, "avg_reward": float(self.ret.mean().item()),
                "success_rate": float(self.success.bool().float().mean().item()),
                "violation_rate": float(self.violation.bool().float().mean().item())}


def eval_rollouts_packed(rollouts, T):
    """The evaluations of several seeds (EvalRollout each) as ONE rrl_eval_rollout_packed launch (one env per packed run:
    rrl_eval_rollout_maze_packed with every seed's env horizon when that env is Maze; rrl_eval_rollout_qs_packed for the
    Q-sampling form, rrl_eval_rollout_sqrl_packed for the SQRL form; their _f16x3_packed entries, with every seed's stream,
    when the rollouts score in f16x3 -- all of them or none)."""
    if len({r.f16x3 for r in rollouts}) > 1:
        raise _lib.RRLError("eval_rollouts_packed: f16x3 and f32 rollouts in one call")
    name, desc_t, side = rollouts[0].entry
    S = len(rollouts)
    args = (desc_t * S)(*[r.desc(T) for r in rollouts])
    sides = [] if side is None else [(type(side) * S)(*[r.entry[2] for r in rollouts])]
    _lib.check(getattr(_lib.load(), name + "_packed")(S, args, *sides, _lib.current_stream()), name + "_packed")
