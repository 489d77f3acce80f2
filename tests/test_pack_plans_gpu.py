"""A packed plan (csrc/pack.hpp) is stored once and complete: from an empty cache the same call twice succeeds twice, the
second call (a hit: it launches from the stored plan alone) writes bit for bit what the first (the miss that built it) wrote,
and rrl_pack_clear() then frees exactly the plans the first call stored."""
import pytest
import torch

import backward_cases as BC
from recovery_rl_amd import _lib
from test_eval_rollout_gpu import GUARD, Launch, launch_packed, same_bits

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def twice(call, outputs, restore):
    """call() twice from an empty plan cache, `restore()` in between -> plans stored; asserts the outputs' bits agree."""
    lib = _lib.load()
    torch.cuda.synchronize()
    lib.rrl_pack_clear()
    runs = []
    for _ in range(2):
        restore()
        assert call() == 0
        torch.cuda.synchronize()
        runs.append([t.clone() for t in outputs])
    assert all(torch.equal(a, b) for a, b in zip(*runs))
    return lib.rrl_pack_clear()


def test_penalty_plan():
    p, S, B = _lib.ptr, 2, 8
    g = torch.Generator(device=DEV)
    g.manual_seed(5)
    z = [torch.randn(1, 2, B, device=DEV, generator=g) * 2 for _ in range(S)]
    lam = [torch.rand(1, device=DEV, generator=g) * 10 + 0.5 for _ in range(S)]
    pen, mean = [torch.empty(B, device=DEV) for _ in range(S)], [torch.empty(1, device=DEV) for _ in range(S)]
    args = (_lib.rrl_penalty_args_t * S)(*[_lib.rrl_penalty_args_t(B, p(z[s]), 1, z[s].stride(0), p(lam[s]), p(pen[s]), p(mean[s]))
                                           for s in range(S)])
    stored = twice(lambda: _lib.load().rrl_rcpo_penalty_packed(S, args, _lib.current_stream()), pen + mean,
                   lambda: [t.fill_(-7.0) for t in pen + mean])
    assert stored == 1
    assert all(float(t[0]) != -7.0 for t in pen + mean)


def test_eval_rollout_plan():
    # 17 rows per seed: two tiles of 16, the second ragged
    launches = [Launch(kind, 17, 2, False, 1) for kind in ("navigation1", "navigation2")]
    first = {id(l): (l.tick.clone(), {k: t.clone() for k, t in l.buf.items()}) for l in launches}
    results = []

    def restore():                      # the device tick advances with every rollout: the same call needs the same tick
        for l in launches:
            tick, buf = first[id(l)]
            l.tick.copy_(tick)
            for k, t in buf.items():
                l.buf[k].copy_(t)

    def call():
        results.append(launch_packed(launches))          # (raises unless RRL_OK)
        return 0
    outputs = [t for l in launches for t in l.buf.values()] + [l.tick for l in launches]
    assert twice(call, outputs, restore) == 1
    assert all(same_bits(a, b) for a, b in zip(*results))
    assert all((out["ret"][:17] != GUARD[torch.float32]).all() for out in results[0])


def test_not_pairable_backward_pair_plans():
    case = BC.BY_NAME["pair-S3-fallback"]
    if BC.removed_by_env(case):
        pytest.skip("an RRL_PACK_PAIR_* setting takes this case off the label %s" % BC.removed_by_env(case))
    assert BC.case_path(case) == "pair-pack-fallback"
    groups = [[BC.Member(case.entry, m, 10 * s + k, DEV) for k, m in enumerate(g)] for s, g in enumerate(case.seeds)]
    outs = [[mb.outputs() for mb in g] for g in groups]
    flat = [o[k + "_flat"] for og in outs for o in og for k in BC.OUTPUTS]
    stored = twice(lambda: BC.launch(case.entry, groups, outs), flat, lambda: [t.fill_(BC.SENT) for t in flat])
    # counted on the parent commit: the "not pairable" marker, the packed head launch's plan and the packed hidden launch's
    assert stored == 3
    assert any(bool((t != BC.SENT).any()) for t in flat)
