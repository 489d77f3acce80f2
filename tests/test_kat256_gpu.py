"""The kernels the bench times against numbers the REFERENCE produced at the production shape (hidden 256, batch 256, 4096
acting rows; tests/golden/model_golden_256.npz from gen_model_golden_256.py): one SAC update + one Q_risk / recovery-policy
update through the grouped fused path (mlp3_fwd_split_group_kernel<1>, backward_pair_kernel, gemm16_group_kernel,
head_bwd_loss_kernel, adam_multi_kernel) and through the stand-alone entry points, and one acting pass through
mlp3_fwd_split_group_kernel<2> with the policy head evaluated by the consuming Q_risk stack.  recovery_rl/sac.py:170-277,
qrisk.py:86-182, experiment.py:546-577 at arg_utils.py:77,89 defaults."""
import numpy as np
import pytest
import torch

import kat256 as KAT

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.mark.parametrize("path", ("grouped", "stand_alone"))
def test_fused_updates_match_the_reference_at_hidden_256_batch_256(path):
    G = KAT.golden()
    agent = KAT.build_agent(DEV)
    fast = agent.enable_fast_path(KAT.K.B)
    qr = agent.safety_critic
    assert fast.grouped and fast.cri_a.split and fast.cri_a.fuse_first      # the launch structure of the timed iteration
    batch, c, e1, e2 = KAT.inputs(DEV)
    s, a, r, s2, m = batch
    if path == "grouped":
        fast._load_batch(batch)                       # the rows the replay draw writes (rrl_sample_multi)
        losses = fast.sac_update(batch, e1, e2, rows_loaded=True, grouped=True).clone()
    else:
        res = agent.update_parameters(None, KAT.K.B, 0, safety_critic=qr, batch=batch, eps_next=e1, eps_pi=e2, as_floats=True)
        assert np.allclose(res, G["sac.returns"], rtol=KAT.REL, atol=2e-6), (res, G["sac.returns"])
        losses = fast.losses.clone()
    assert np.allclose(losses[:3].cpu().numpy(), G["sac.returns"][:3], rtol=KAT.REL, atol=2e-6)
    fast.gather_first_grads()
    KAT.check_grads(G, "sac.grad.critic", KAT.flat_grads_twin(fast.critic))
    KAT.check_grads(G, "sac.grad.policy", KAT.flat_grads_policy(fast.policy, True))
    KAT.check_post(G, "sac.post.critic", agent.critic, "sac.grad.critic")
    KAT.check_post(G, "sac.post.critic_target", agent.critic_target)
    KAT.check_post(G, "sac.post.policy", agent.policy, "sac.grad.policy")
    assert int(fast.critic.step[0].item()) == 1 and int(fast.policy.step[0].item()) == 1
    q_batch = (s, a, c, s2, m)
    if path == "grouped":
        xu, x2u, xpu = fast.rows_q
        xu[:, 0:2], xu[:, 2:4], x2u[:, 0:2], xpu[:, 0:2] = s, a, s2, s
        fast.qrisk_update(q_batch, e1, e2, rows_loaded=True, rows=fast.rows_q, grouped=True)
    else:
        qr.update_parameters(policy=agent.policy, batch=q_batch, eps_next=e1, eps_pi=e2)
    fast.gather_first_grads()
    KAT.check_grads(G, "mf.grad.qrisk", KAT.flat_grads_twin(fast.qrisk))
    KAT.check_grads(G, "mf.grad.recpolicy", KAT.flat_grads_policy(fast.recpolicy, False))
    KAT.check_post(G, "mf.post.qrisk", qr.safety_critic, "mf.grad.qrisk")
    KAT.check_post(G, "mf.post.qrisk_target", qr.safety_critic_target)
    KAT.check_post(G, "mf.post.recpolicy", qr.policy, "mf.grad.recpolicy")
    assert np.allclose(qr.get_value(s, a).cpu().numpy().ravel(), G["mf.get_value"], rtol=KAT.REL, atol=2e-6)
    assert int(fast.qrisk.step[0].item()) == 1 and int(fast.recpolicy.step[0].item()) == 1


def _updated_agent():
    agent = KAT.build_agent(DEV)
    fast = agent.enable_fast_path(KAT.K.B)
    batch, c, e1, e2 = KAT.inputs(DEV)
    agent.update_parameters(None, KAT.K.B, 0, safety_critic=agent.safety_critic, batch=batch, eps_next=e1, eps_pi=e2)
    agent.safety_critic.update_parameters(policy=agent.policy, batch=(batch[0], batch[1], c, batch[3], batch[4]),
                                          eps_next=e1, eps_pi=e2)
    return agent, fast


@pytest.mark.parametrize("defer", (False, True))
def test_acting_pass_at_4096_rows_matches_the_reference(defer):
    """get_action (experiment.py:546-577) for 4096 observations on the updated networks: task action, Q_risk(s, a_task), the
    gate at eps_safe and the recovery action.  defer = True is the timed iteration's form: the task policy's head is evaluated
    by the Q_risk stack that consumes its action, the gate is left to the step kernel."""
    from recovery_rl_amd.fast_update import FastActor
    G = KAT.golden()
    agent, fast = _updated_agent()
    n = KAT.K.N_ACT
    actor = FastActor(fast, n)
    obs, noise = KAT.K.acting()
    obs, noise = torch.as_tensor(obs, device=DEV), torch.as_tensor(noise, device=DEV)
    eps_safe = 0.3
    task, real, rec = actor.act(obs, eps_safe, True, True, noise=noise, defer_select=defer)
    if defer:
        zq, zn, zs, thr, rec_action, rec_head = actor.pending_select
        assert zn == 4 and rec_action is None and rec_head is not None and thr == pytest.approx(eps_safe)
        z = actor.qr.scratch.sum(0)                                   # the partial last-layer sums the step kernel adds up
        risk = torch.sigmoid(z).max(0).values.reshape(-1)
        KAT.check_acting(G, actor.xa[:, 2:4], risk, None)
        assert torch.equal(actor.xa[:, 0:2], obs)
        return
    risk = torch.sigmoid(actor.qr.out).max(0).values.reshape(-1)
    KAT.check_acting(G, task, risk, actor.rec_action)
    ref_risk = torch.as_tensor(G["act.risk"], device=DEV)
    gate = ref_risk > eps_safe
    border = (ref_risk - eps_safe).abs() < 1e-5
    assert torch.equal(rec.bool()[~border], gate[~border]) and 0 < int(gate.sum()) <= n
    want = torch.where(gate.unsqueeze(1), torch.as_tensor(G["act.rec_action"], device=DEV),
                       torch.as_tensor(G["act.task_action"], device=DEV))
    assert torch.allclose(real[~border], want[~border], rtol=KAT.REL, atol=1e-5)
