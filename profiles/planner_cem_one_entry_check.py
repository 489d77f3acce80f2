"""ABI 8 against ABI 7 on the same box and the same inputs: the planner, CEM and stand-alone loss-gradient entry points of
the in-tree library (descriptors alone) against the parent commit's library driven through its positional signatures.
Every output buffer and every tick is compared with torch.equal (buffers start from a sentinel on both sides, so what a
launch leaves alone is compared too).

    python profiles/planner_cem_one_entry_check.py <parent librrl_hip.so> [result.json]
The parent library is the parent commit's tree built with its own recovery_rl_amd/_lib.py build()."""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402

from recovery_rl_amd import _lib  # noqa: E402

DEV = "cuda:0"
p = _lib.ptr


def parent_library(path):
    """The ABI 7 library with the positional signatures this change removed."""
    old = C.CDLL(os.path.abspath(path))
    vp, i32, i64, u64, ci, f64, f32, ll = (C.c_void_p, C.c_int32, C.c_int64, C.c_uint64, C.c_int, C.c_double, C.c_float,
                                          C.c_longlong)
    plan = [vp, ci, ci, ci, ci, ll, ci, ci, vp, vp, vp, u64, u64, vp, u64, vp, vp, vp]
    sig = {
        "rrl_plan_pack": [vp, vp, vp], "rrl_plan_pack_f16x3": [vp, vp, vp],
        "rrl_plan_cost": plan, "rrl_plan_cost_f16x3": plan,
        "rrl_plan_cost_n": [ci, vp, ci, ci, ci, ci, vp, ll, ci, ci, vp, vp, vp, u64, u64, vp, u64, vp, vp, vp],
        "rrl_cem_sample": [i64, i32, i32, vp, vp, vp, vp, f64, ci, vp, u64, u64, vp, u64, vp, vp],
        "rrl_cem_update": [i64, i32, i32, i32, f64, vp, vp, vp, vp, vp, vp],
        "rrl_cem_begin": [i64, vp, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp],
        "rrl_cem_sample_n": [vp, i64, i32, i32, vp, vp, vp, vp, f64, ci, vp, u64, u64, vp, u64, vp, vp],
        "rrl_cem_update_n": [vp, i64, i32, i32, i32, f64, vp, vp, vp, vp, vp, vp],
        "rrl_cem_finish": [i64, vp, i32, i32, vp, vp, vp, vp, vp, vp],
        "rrl_gauss_head_bwd": [ci, vp, ci, ll, vp, vp, vp, ci, ci, ll, f32, vp, vp],
        "rrl_sac_critic_grad": [ci, vp, vp, ci, ll, vp, vp, vp, f32, vp, vp, vp, vp, vp],
        "rrl_sac_policy_grad": [ci, vp, ci, ll, vp, vp, vp, vp, vp],
        "rrl_qrisk_critic_grad": [ci, vp, vp, ci, ll, vp, vp, f32, vp, vp, vp],
        "rrl_qrisk_policy_grad": [ci, vp, ci, ll, vp, vp, vp],
        "rrl_dgd_qrisk_grad": [ci, vp, ci, ll, f32, vp, vp, vp],
        "rrl_rcpo_penalty": [ci, vp, ci, ll, vp, vp, vp, vp],
        "rrl_stoch_head_bwd": [ci, vp, ci, ll, vp, vp, f32, vp, vp, ci, ci, ll, vp, vp, vp],
    }
    for name, args in sig.items():
        getattr(old, name).argtypes, getattr(old, name).restype = args, ci
    old.rrl_abi_version.restype = ci
    assert old.rrl_abi_version() == 7, "the parent library is the ABI 7 build"
    return old


def same(pairs):
    torch.cuda.synchronize()
    return all(bool(torch.equal(a, b)) for a, b in pairs)


def planner(old, new, out):
    from test_plan_gpu import build
    for f16x3 in (False, True):
        _, mpc, _ = build(f16x3=f16x3)
        fp, st = mpc.fused, _lib.current_stream()
        packed_old = torch.zeros_like(fp.packed)
        w = _lib.rrl_plan_weights_t(fp.hq, fp.he, fp.n_nets, *[t.data_ptr() for t in fp._keep])
        assert (old.rrl_plan_pack_f16x3 if f16x3 else old.rrl_plan_pack)(C.addressof(w), p(packed_old), st) == 0
        out.append({"what": "rrl_plan_pack", "f16x3": f16x3, "identical": same([(packed_old, fp.packed)])})
        for M, pop, hor in ((1, 400, 5), (2, 30, 5), (5, 7, 5), (3, 100, 9)):
            g = torch.Generator(device=DEV).manual_seed(M * 1000 + pop + hor)
            bound = M + 2
            acs = torch.rand(bound, pop, hor * 2, device=DEV, generator=g) * 2 - 1
            obs = torch.randn(bound, 2, device=DEV, generator=g) * torch.tensor([1.5, 1.0], device=DEV) + \
                torch.tensor([-0.5, 0.3], device=DEV)
            for device_count in (False, True):
                rows = bound if device_count else M
                noise = torch.randn(hor, rows * pop * mpc.npart, 2, device=DEV, generator=g)
                count = torch.tensor([M], dtype=torch.int32, device=DEV) if device_count else None
                n_scratch = int(new.rrl_plan_scratch_floats(fp.n_nets, rows, pop))
                for nz in (noise, None):
                    ticks = [torch.zeros(2, dtype=torch.int64, device=DEV) for _ in range(2)]
                    costs = [torch.full((rows, pop), -7.0, device=DEV) for _ in range(2)]
                    scratch = [torch.zeros(n_scratch, device=DEV) for _ in range(2)]
                    tail = (pop, hor, p(obs), p(acs), p(nz), fp.seed, 3, p(ticks[0]), 1, p(scratch[0]), p(costs[0]), st)
                    if device_count:
                        rc = old.rrl_plan_cost_n(int(f16x3), p(fp.packed), fp.hq, fp.he, fp.n_nets, mpc.npart, p(count), rows, *tail)
                    else:
                        entry = old.rrl_plan_cost_f16x3 if f16x3 else old.rrl_plan_cost
                        rc = entry(p(fp.packed), fp.hq, fp.he, fp.n_nets, mpc.npart, rows, *tail)
                    assert rc == 0
                    a = _lib.rrl_plan_cost_t(p(fp.packed), fp.hq, fp.he, fp.n_nets, mpc.npart, int(f16x3), rows, p(count), pop, hor,
                                             p(obs), p(acs), p(nz), fp.seed, 3, p(ticks[1]), 1, p(scratch[1]), p(costs[1]))
                    assert new.rrl_plan_cost(C.byref(a), st) == 0
                    out.append({"what": "rrl_plan_cost", "f16x3": f16x3, "M": M, "pop": pop, "plan_hor": hor,
                                "count": "device" if device_count else "host", "noise": "array" if nz is not None else "philox",
                                "identical": same([(costs[0], costs[1]), (ticks[0], ticks[1]), (scratch[0], scratch[1])]),
                                "costs_std": float(costs[1][:M].std())})


def cem(old, new, out):
    st = _lib.current_stream()
    for M, pop, dim in ((3, 40, 10), (2, 1000, 7)):
        g = torch.Generator(device=DEV).manual_seed(M * 1000 + pop + dim)
        for device_count in (False, True):
            rows = M + 2 if device_count else M
            count = torch.tensor([M], dtype=torch.int32, device=DEV) if device_count else None
            mean0 = (torch.rand(rows, dim, device=DEV, generator=g, dtype=torch.float64) * 1.8 - 0.9)
            var0 = torch.rand(rows, dim, device=DEV, generator=g, dtype=torch.float64) * 0.3
            var0[M // 2] = 1e-5                      # one problem has converged: inactive
            lb, ub = -torch.ones(dim, dtype=torch.float64, device=DEV), torch.ones(dim, dtype=torch.float64, device=DEV)
            costs = torch.randn(rows, pop, device=DEV, generator=g)
            costs[0, :3] = float("nan")
            side = []
            for k in range(2):
                side.append(dict(mean=mean0.clone(), var=var0.clone(), active=torch.full((rows,), 9, dtype=torch.uint8, device=DEV),
                                 samples=torch.full((rows, pop, dim), 7.0, device=DEV),
                                 tick=torch.zeros(2, dtype=torch.int64, device=DEV)))
            o, n = side
            ne = max(1, pop // 10)
            s_args = (pop, dim, p(o["mean"]), p(o["var"]), p(lb), p(ub), 1e-3, 1, p(o["active"]), 11, 2, p(o["tick"]), 1,
                      p(o["samples"]), st)
            u_args = (pop, dim, ne, 0.25, p(o["samples"]), p(costs), p(o["mean"]), p(o["var"]), p(o["active"]), st)
            c = _lib.rrl_cem_t(rows, p(count), pop, dim, p(n["mean"]), p(n["var"]), p(lb), p(ub), 1e-3, 1, p(n["active"]), 11, 2,
                               p(n["tick"]), 1, p(n["samples"]), ne, 0.25, p(costs))
            for step in range(2):                    # two iterations: the second samples from the updated mean / variance
                if device_count:
                    assert old.rrl_cem_sample_n(p(count), rows, *s_args) == 0 and old.rrl_cem_update_n(p(count), rows, *u_args) == 0
                else:
                    assert old.rrl_cem_sample(rows, *s_args) == 0 and old.rrl_cem_update(rows, *u_args) == 0
                assert new.rrl_cem_sample(c, st) == 0 and new.rrl_cem_update(c, st) == 0
            out.append({"what": "rrl_cem_sample + rrl_cem_update, two iterations", "M": M, "pop": pop, "dim": dim,
                        "count": "device" if device_count else "host",
                        "identical": same([(o[k], n[k]) for k in o]), "tick": int(n["tick"][0])})
    for n_env, frac in ((64, 0.3), (700, 0.05)):
        g = torch.Generator(device=DEV).manual_seed(n_env)
        dim, du = 10, 2
        mask = (torch.rand(n_env, device=DEV, generator=g) < frac).to(torch.uint8)
        obs = torch.randn(n_env, 2, device=DEV, generator=g)
        init_var = torch.rand(dim, device=DEV, generator=g, dtype=torch.float64)
        prev0 = torch.rand(n_env, dim, device=DEV, generator=g, dtype=torch.float64)
        side = []
        for k in range(2):
            side.append(dict(prev_sol=prev0.clone(), idx=torch.full((n_env,), -1, dtype=torch.int32, device=DEV),
                             count=torch.full((1,), -1, dtype=torch.int32, device=DEV),
                             mean=torch.full((n_env, dim), -5.0, dtype=torch.float64, device=DEV),
                             var=torch.full((n_env, dim), -5.0, dtype=torch.float64, device=DEV),
                             cur_obs=torch.full((n_env, 2), -5.0, device=DEV),
                             active=torch.full((n_env,), 9, dtype=torch.uint8, device=DEV),
                             action=torch.full((n_env, du), -5.0, device=DEV)))
        o, n = side
        assert old.rrl_cem_begin(n_env, p(mask), dim, p(o["prev_sol"]), p(init_var), p(obs), p(o["idx"]), p(o["count"]),
                                 p(o["mean"]), p(o["var"]), p(o["cur_obs"]), p(o["active"]), st) == 0
        s = _lib.rrl_cem_set_t(n_env, p(mask), dim, du, p(n["prev_sol"]), p(init_var), p(obs), p(n["idx"]), p(n["count"]),
                               p(n["mean"]), p(n["var"]), p(n["cur_obs"]), p(n["active"]), p(n["action"]))
        assert new.rrl_cem_begin(s, st) == 0
        begun = same([(o[k], n[k]) for k in o])
        assert old.rrl_cem_finish(n_env, p(mask), dim, du, p(o["idx"]), p(o["count"]), p(o["mean"]), p(o["prev_sol"]),
                                  p(o["action"]), st) == 0
        assert new.rrl_cem_finish(s, st) == 0
        out.append({"what": "rrl_cem_begin, rrl_cem_finish", "n": n_env, "masked": int(mask.sum()), "count": int(n["count"][0]),
                    "identical": begun and same([(o[k], n[k]) for k in o])})


def losses(old, new, out):
    st, L = _lib.current_stream(), _lib
    for B, n_part in ((64, 1), (256, 4)):
        g = torch.Generator(device=DEV).manual_seed(B)
        r = lambda *s: torch.randn(*s, device=DEV, generator=g)
        q, qt, head, raw = r(n_part, 2, B), r(n_part, 2, B), r(n_part, B, 4), r(n_part, B, 2)
        v = [r(B) for _ in range(3)]
        m = (torch.rand(B, device=DEV, generator=g) < 0.8).float()
        alpha, pen, eps, scale, log_std, dx = r(1).abs(), r(B).abs(), r(B, 2), r(2).abs() + 0.5, r(2), r(2, B, 4)
        da = dict(d_action=dx.data_ptr() + 8, ld=4, n_heads=2, head_stride=B * 4)     # the action columns of dx [2, B, 4]
        crit = dict(n_part=n_part, part_stride=2 * B)
        cases = {
            "sac_critic": (L.LOSS_SAC_CRITIC, (2, B), 2, dict(out=p(q), out_t=p(qt), v0=p(v[0]), v1=p(v[1]), v2=p(m), v3=p(pen),
                                                              alpha=p(alpha), f0=0.99, **crit)),
            "sac_policy": (L.LOSS_SAC_POLICY, (2, B), 1, dict(out=p(q), v0=p(v[0]), alpha=p(alpha), **crit)),
            "qrisk_critic": (L.LOSS_QRISK_CRITIC, (2, B), 2, dict(out=p(q), out_t=p(qt), v0=p(m), v1=p(m), f0=0.8, **crit)),
            "qrisk_policy": (L.LOSS_QRISK_POLICY, (2, B), 1, dict(out=p(q), **crit)),
            "dgd_qrisk": (L.LOSS_DGD_QRISK, (2, B), 1, dict(out=p(q), f0=50.0, **crit)),
            "gauss_head": (L.LOSS_GAUSS_HEAD, (B, 4), 0, dict(out=p(head), n_part=n_part, part_stride=4 * B, v0=p(eps), v1=p(scale),
                                                              f0=0.2 / B, **da)),
            "stoch_head": (L.LOSS_STOCH_HEAD, (B, 2), 2, dict(out=p(raw), n_part=n_part, part_stride=2 * B, v0=p(eps),
                                                              v1=p(log_std), v2=p(scale), f0=-1.0, **da)),
        }
        for name, (kind, shape, n_loss, f) in cases.items():
            d = [torch.full(shape, -7.0, device=DEV) for _ in range(2)]
            ls = [torch.full((max(n_loss, 1),), -7.0, device=DEV) for _ in range(2)]
            o = _lib.rrl_loss_t(kind=kind, loss=p(ls[0]) if n_loss else None, **f)
            out_ = (o.out, o.n_part, o.part_stride)
            tail = (o.d_action, o.ld, o.n_heads, o.head_stride)
            rc = {
                "sac_critic": lambda: old.rrl_sac_critic_grad(B, o.out, o.out_t, o.n_part, o.part_stride, o.v0, o.v1, o.v2, o.f0,
                                                              o.alpha, o.v3, p(d[0]), o.loss, st),
                "sac_policy": lambda: old.rrl_sac_policy_grad(B, *out_, o.v0, o.alpha, p(d[0]), o.loss, st),
                "qrisk_critic": lambda: old.rrl_qrisk_critic_grad(B, o.out, o.out_t, o.n_part, o.part_stride, o.v0, o.v1, o.f0,
                                                                  p(d[0]), o.loss, st),
                "qrisk_policy": lambda: old.rrl_qrisk_policy_grad(B, *out_, p(d[0]), o.loss, st),
                "dgd_qrisk": lambda: old.rrl_dgd_qrisk_grad(B, *out_, o.f0, p(d[0]), o.loss, st),
                "gauss_head": lambda: old.rrl_gauss_head_bwd(B, *out_, o.v0, o.v1, *tail, o.f0, p(d[0]), st),
                "stoch_head": lambda: old.rrl_stoch_head_bwd(B, *out_, o.v0, o.v1, o.f0, o.v2, *tail, p(d[0]), o.loss, st),
            }[name]()
            assert rc == 0
            nl = _lib.rrl_loss_t(kind=kind, loss=p(ls[1]) if n_loss else None, **f)
            assert new.rrl_loss_dout(C.byref(nl), B, p(d[1]), st) == 0
            out.append({"what": "rrl_loss_dout", "kind": name, "B": B, "n_part": n_part,
                        "identical": same([(d[0], d[1]), (ls[0], ls[1])]), "written": bool((d[1] != -7.0).all())})
        lam = r(1).abs() + 1
        for want in (True, False):
            pens, means = [torch.full((B,), -7.0, device=DEV) for _ in range(2)], [torch.full((1,), -7.0, device=DEV) for _ in range(2)]
            args = lambda k: (B, p(q), n_part, 2 * B, p(lam) if want else None, p(pens[k]) if want else None, p(means[k]))
            assert old.rrl_rcpo_penalty(*args(0), st) == 0
            assert new.rrl_rcpo_penalty(C.byref(_lib.rrl_penalty_args_t(*args(1))), st) == 0
            out.append({"what": "rrl_rcpo_penalty", "form": "penalty and mean" if want else "mean only", "B": B, "n_part": n_part,
                        "identical": same([(pens[0], pens[1]), (means[0], means[1])])})


def main():
    old, new = parent_library(sys.argv[1]), _lib.load()
    assert new.rrl_abi_version() == 8
    out = []
    planner(old, new, out)
    cem(old, new, out)
    losses(old, new, out)
    res = {"what": "in-tree library (ABI 8, descriptors) against the parent library (ABI 7, positional), same inputs",
           "cases": out, "n_cases": len(out), "all_identical": all(c["identical"] for c in out)}
    text = json.dumps(res, indent=1)
    if len(sys.argv) > 2:
        open(sys.argv[2], "w").write(text + "\n")
    print(json.dumps({"n_cases": len(out), "all_identical": res["all_identical"],
                      "different": [c for c in out if not c["identical"]]}))
    sys.exit(0 if res["all_identical"] else 1)


if __name__ == "__main__":
    main()
