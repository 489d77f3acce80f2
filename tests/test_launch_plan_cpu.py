"""Which entry points one SAC update and one Q_risk (+ recovery-policy) update launch, pinned on the CPU: FastUpdater is built
on CPU tensors and the library replaced by a recorder that notes the entry point and returns 0 (the host-only queries go
through to the real library, which loads without a device).  The two updates are stated once (FastUpdater.sac_update /
qrisk_update) and issued either member by member through the stand-alone entry points -- what SAC.update_parameters and
QRiskWrapper.update_parameters run, and the reference of the GPU tests -- or with independent kernels sharing launches
(grouped = True: update_pair, the captured iteration, the bench).  The expected values were recorded the same way before
the two statements of each update were merged into one, and the stack backward and the optimiser step then moved from
their positional entry points to the descriptor ones (ABI 6): the entry-point names below changed, no count did.  The same
holds for the policy heads (ABI 7): a lone head is rrl_policy_heads_fwd_multi with one member, where the positional Gaussian
and stochastic head entry points stood (2 and 1 + 1 launches became 2 and 2)."""
from collections import Counter

import numpy as np
import pytest
import torch

import arg_utils
from recovery_rl_amd import _lib
from recovery_rl_amd.sac import SAC
from recovery_rl_amd.spaces import Box

ACT = Box(-np.ones(2), np.ones(2))
OBS = Box(-np.ones(2) * np.inf, np.ones(2) * np.inf)
HOST_ONLY = ("rrl_mlp3_is_split", "rrl_abi_version", "rrl_last_hip_error")


@pytest.fixture
def calls(monkeypatch):
    real, names = _lib.load(), []

    class Recorder:
        def __getattr__(self, name):
            if name in HOST_ONLY:
                return getattr(real, name)
            return lambda *args: names.append(name[4:]) or 0           # without the rrl_ prefix

    monkeypatch.setattr(_lib, "_lib", Recorder())
    monkeypatch.setattr(_lib, "current_stream", lambda: 0)
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: False)
    return names


def updater(hidden, B):
    argv = ["--env-name", "navigation1", "--hidden_size", str(hidden), "--use_recovery", "--MF_recovery",
            "--gamma_safe", "0.8", "--eps_safe", "0.3"]
    torch.manual_seed(0)
    fast = SAC(OBS, ACT, arg_utils.get_args(argv), "/tmp").enable_fast_path(B)
    r = lambda *s: torch.randn(*s)
    return fast, (r(B, 2), r(B, 2), r(B), r(B, 2), r(B)), r(B, 2), r(B, 2)


def launches(calls, fn, *args, **kw):
    del calls[:]
    fn(*args, **kw)
    return list(calls)


FWD, PAIR, ADAM = "mlp3_forward_multi", "mlp_backward_pair_multi", "adam_step_multi"


def test_launches_of_the_two_updates_at_hidden_256_batch_256(calls):
    fast, batch, e1, e2 = updater(256, 256)
    assert fast.grouped and fast.cri_a.split and fast.cri_a.fuse_first
    # grouped: the sequence of the captured iteration
    assert launches(calls, fast.sac_update, batch, e1, e2, grouped=True) == [FWD, FWD, PAIR, PAIR, ADAM]
    assert launches(calls, fast.qrisk_update, batch, e1, e2, rows=fast.rows_q, grouped=True) == \
        [FWD, FWD, PAIR, ADAM, FWD, PAIR, PAIR, ADAM]
    # member by member: the same work through the stand-alone entry points
    assert Counter(launches(calls, fast.sac_update, batch, e1, e2)) == \
        {"mlp3_forward": 4, "policy_heads_fwd_multi": 2, PAIR: 3, ADAM: 1}
    assert Counter(launches(calls, fast.qrisk_update, batch, e1, e2)) == \
        {"mlp3_forward": 5, "policy_heads_fwd_multi": 2, PAIR: 3, ADAM: 2}


# a lone stack backward, first layer as its own launch: with weight gradients / for the input gradient only (the same
# two launches: the hidden-layer descriptor then has no dW2)
BWD_W = {PAIR: 1, "mlp_input_backward_multi": 1}
BWD_X = {PAIR: 1, "mlp_input_backward_multi": 1}


def total(*counts):
    return sum((Counter(c) for c in counts), Counter())


def test_launches_of_the_two_updates_at_hidden_32_batch_64(calls):
    """No column-split forward at this width, no first layer inside the hidden-layer launch at this batch: policy heads are
    launches of their own, lone members take the stand-alone entry points in the grouped mode too."""
    fast, batch, e1, e2 = updater(32, 64)
    assert fast.grouped and not fast.cri_a.split and not fast.cri_a.fuse_first
    assert Counter(launches(calls, fast.sac_update, batch, e1, e2, grouped=True)) == total(
        {"mlp3_forward": 1, "policy_heads_fwd_multi": 1, FWD: 1, PAIR: 1, "mlp_input_backward_multi": 1, ADAM: 1}, BWD_W)
    assert Counter(launches(calls, fast.qrisk_update, batch, e1, e2, rows=fast.rows_q, grouped=True)) == total(
        {FWD: 2, "policy_heads_fwd_multi": 1, "mlp3_forward": 1, ADAM: 2}, BWD_W, BWD_X, BWD_W)
    assert Counter(launches(calls, fast.sac_update, batch, e1, e2)) == total(
        {"mlp3_forward": 4, "policy_heads_fwd_multi": 2, ADAM: 1}, BWD_W, BWD_X, BWD_W)
    assert Counter(launches(calls, fast.qrisk_update, batch, e1, e2)) == total(
        {"mlp3_forward": 5, "policy_heads_fwd_multi": 2, ADAM: 2}, BWD_W, BWD_X, BWD_W)


def test_launches_of_the_two_updates_at_hidden_512_batch_256(calls):
    """A width the one-launch forward does not cover: every layer of a forward on the GEMM kernel, no grouped mode."""
    fast, batch, e1, e2 = updater(512, 256)
    assert not fast.grouped and not fast.cri_a.fuse_first
    assert Counter(launches(calls, fast.sac_update, batch, e1, e2)) == total(
        {"gemm_f32": 3 * 4, "policy_heads_fwd_multi": 2, ADAM: 1}, BWD_W, BWD_X, BWD_W)
    assert Counter(launches(calls, fast.qrisk_update, batch, e1, e2)) == total(
        {"gemm_f32": 3 * 5, "policy_heads_fwd_multi": 2, ADAM: 2}, BWD_W, BWD_X, BWD_W)
