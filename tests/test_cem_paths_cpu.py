"""The tables of cem_cases.py reach every launch edge of the CEM bookkeeping kernels -- proven on the host from the constants
parsed out of csrc/rrl_host.hpp and csrc/cem_kernels.hip, so that a retuned constant fails here instead of moving a case of
test_cem_paths_gpu.py off its edge unnoticed --; the float64 restatement of the elite update equals the C oracle bit for bit on
every update case; the oracle's draws obey the specification of the truncated-normal sampling on every sample case; and the
restatements of begin and finish are the host-count arithmetic of MPC.act."""
import os
import re

import numpy as np
import pytest
import torch

import cem_cases as CC
from oracle import c_oracle as co

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "recovery_rl_amd", "csrc")


def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _all_equal(pattern, text, what, at_least=1):
    found = re.findall(pattern, text)
    assert len(found) >= at_least and len(set(found)) == 1, "%s: found %r in the source" % (what, found)
    return int(found[0])


# ---- the literals are the sources' --------------------------------------------------------------------------------------------
def test_the_restated_constants_are_the_sources():
    host, hip = _src("rrl_host.hpp"), _src("cem_kernels.hip")
    got = dict(kBlock=_all_equal(r"constexpr\s+int\s+kBlock\s*=\s*(\d+)\s*;", host, "kBlock"),
               kMaxGrid=_all_equal(r"constexpr\s+int\s+kMaxGrid\s*=\s*(\d+)\s*;", host, "kMaxGrid"),
               kBeginBlock=_all_equal(r"constexpr\s+int\s+kBeginBlock\s*=\s*(\d+)\s*;", hip, "kBeginBlock"),
               max_pop=_all_equal(r"pop <= 0 \|\| pop > (\d+)", hip, "the pop limit", at_least=2),
               max_dim=_all_equal(r"dim <= 0 \|\| (?:s->)?dim > (\d+)", hip, "the dim limit", at_least=4))
    assert got == CC.CONSTANTS
    assert (CC.K_BLOCK, CC.K_MAX_GRID, CC.K_BEGIN_BLOCK, CC.MAX_POP, CC.MAX_DIM) == tuple(got[k] for k in (
        "kBlock", "kMaxGrid", "kBeginBlock", "max_pop", "max_dim"))
    assert CC.STRIDE_ELEMENTS == got["kMaxGrid"] * got["kBlock"] == 524288 and CC.K_BEGIN_BLOCK % CC.WAVE == 0
    # the launch arithmetic the tables rely on
    for line in ("return int(g < 1 ? 1 : (g > kMaxGrid ? kMaxGrid : g));",):
        assert line in host, line
    for line in ("dim3(grid_for(M * pop * dim)), dim3(kBlock)", "dim3(grid_for(s->n * s->dim)), dim3(kBlock)",
                 "cem_begin_kernel, dim3(1), dim3(kBeginBlock)", "while (padded < pop) padded <<= 1;",
                 "cem_update_kernel, dim3((unsigned)M), dim3(kBlock), size_t(padded) * 8",
                 "for (int64_t first = 0; first < n; first += kBeginBlock) {", "c = (c != c) ? 1e6f : c;",
                 "bool act = vmax > epsilon;", "if (sticky && !active[m]) act = false;",
                 "rrl::advance_counter(counter_dev, (m_dev && M == 0) ? 0 : counter_inc);",
                 "rrl::normal_at(seed, row, rrl::kStreamCem, (ctr << 20) | (uint64_t(d) << 8) | attempt, z0, z1);"):
        assert line in hip, line
    assert _all_equal(r"\bkStreamCem\s*=\s*(\d+)\b", _src("rrl_device.hpp"), "kStreamCem") == CC.STREAM_CEM == co.STREAM_CEM
    assert CC.grid_for(1) == 1 and CC.grid_for(257) == 2 and CC.grid_for(CC.STRIDE_ELEMENTS + 1) == CC.K_MAX_GRID
    assert [CC.padded_pop(p) for p in (1, 2, 3, 64, 65, 400, 1024)] == [1, 2, 4, 64, 128, 512, 1024]
    with open(os.path.join(os.path.dirname(HERE), "oracle", "Makefile")) as f:
        assert "-ffp-contract=off" in f.read()           # the oracle's sums are the restatement's: no fused multiply-add


# ---- the tables reach what they claim -----------------------------------------------------------------------------------------
def _pow2(p):
    return p & (p - 1) == 0


def test_the_sample_table_reaches_its_edges():
    cases = CC.SAMPLE_CASES
    el = {c.name: c.M * c.pop * c.dim for c in cases}
    assert any(c.M == 3 and c.pop == 400 and c.dim == 10 for c in cases)
    over = [n for n, e in el.items() if e > CC.K_MAX_GRID * CC.K_BLOCK]
    assert over and all(el[n] < 2 * CC.STRIDE_ELEMENTS for n in over)     # just over: the second trip is ragged
    assert max(el.values()) == 560000
    assert {1, CC.MAX_POP} <= {c.pop for c in cases} and {1, CC.MAX_DIM} <= {c.dim for c in cases}
    assert any(c.M >= 2000 and c.pop * c.dim <= 16 for c in cases)
    assert {c.bounds for c in cases} == set(CC.BOUNDS)
    # several problems inside one workgroup and one problem over several workgroups
    assert any(c.pop * c.dim < CC.K_BLOCK // 2 and c.M > 2 for c in cases) and any(c.pop * c.dim > 4 * CC.K_BLOCK for c in cases)
    setups = {c.setup for c in cases}
    for mean in ("interior", "on_ub", "on_lb", "outside"):
        assert any(s.startswith("mean:%s:" % mean) for s in setups), mean
    for var in ("below", "at", "above"):
        assert any(s.startswith("mean:") and s.endswith(":" + var) for s in setups), var
    assert {"act:eps", "act:next", "act:lastdim", "sticky"} <= setups
    assert {c.sticky for c in cases if c.setup == "sticky"} == {0, 1}
    # counters: host alone, tick alone, both; counter_inc of 1 and 3; every kind of device count
    assert any(c.tick is None and c.counter for c in cases) and any(c.tick and not c.counter for c in cases)
    both = [c for c in cases if c.tick and c.counter]
    assert {1, 3} <= {c.inc for c in both}
    assert any(c.live == 0 for c in cases) and any(c.live is not None and 0 < c.live < c.M for c in cases)
    assert any(c.live == c.M for c in cases)
    # the production flags together: sticky, device count, device tick, counter_inc = 1, host counter 0
    assert any(c.sticky == 1 and c.live == c.M and c.tick is not None and c.inc == 1 and c.counter == 0 for c in cases)
    # a ticket taken by one workgroup, by some and by the whole capped grid
    grids = {CC.grid_for(el[c.name]) for c in cases if c.tick is not None and c.inc}
    assert CC.K_MAX_GRID in grids and any(1 < g < CC.K_MAX_GRID for g in grids)
    for c in cases:
        assert c.what and 1 <= c.pop <= CC.MAX_POP and 1 <= c.dim <= CC.MAX_DIM and c.M * c.pop <= 0xffffffff
        assert CC.oracle_counter(c) < 2 ** 44                               # the counter is shifted left by 20 bits


def test_the_sample_inputs_are_what_their_cases_say():
    for c in CC.SAMPLE_CASES:
        x = CC.sample_inputs(c.name)
        mean, var, lb, ub = x["mean"], x["var"], x["lb"], x["ub"]
        assert mean.shape == var.shape == (c.M, c.dim) and lb.shape == ub.shape == (c.dim,) and (lb < ub).all()
        if c.bounds == "varied" and c.dim > 1:
            assert len(set(lb)) == c.dim and len(set(ub)) == c.dim and len(set(ub - lb)) == c.dim
        cl = CC.clamp_of(mean, lb, ub)
        kind = c.setup.split(":")
        if kind[0] == "mean":
            inside = ((mean > lb) & (mean < ub))
            if kind[1] == "interior":
                assert inside.all() and (cl > 0).all()
            elif kind[1] == "on_ub":
                assert (mean[0] == ub).all() and (mean[:, ::2] == ub[::2]).all() and inside[1:, 1::2].all()
                assert (cl[:, ::2] == 0).all() and (cl[1:, 1::2] > 0).all()
            elif kind[1] == "on_lb":
                assert (mean[0] == lb).all() and (mean[:, ::2] == lb[::2]).all() and inside[1:, 1::2].all()
                assert (cl[:, ::2] == 0).all()
            else:
                assert (mean[:, ::2] > ub[::2]).all() and (mean[:, 1::4] < lb[1::4]).all() and (cl > 0).all()
            pos = cl > 0
            assert dict(below=(var[pos] < cl[pos]).all(), at=(var == cl).all(), above=(var > cl).all())[kind[2]]
        if kind[0] == "generic" and c.M >= 3:
            assert (var.max(1) > CC.EPSILON).any() and (var.max(1) <= CC.EPSILON).any()
        if c.setup == "act:eps":
            assert (var[0] == CC.EPSILON).all()
        if c.setup == "act:next":
            assert var[0].max() > CC.EPSILON and var[0].max() == np.nextafter(CC.EPSILON, np.inf) and (np.sort(var[0])[:-1] == CC.EPSILON).all()
        if c.setup == "act:lastdim":
            assert (var[0, :-1] <= CC.EPSILON).all() and var[0, -1] > CC.EPSILON
        if c.setup == "sticky":
            assert x["active_in"].tolist() == [0, 1, 7, 0] and var[0].max() > CC.EPSILON > var[1].max()


def test_the_update_table_reaches_its_edges():
    cases = CC.UPDATE_CASES
    assert {c.pop for c in cases} == set(CC.UPDATE_POPS) and {c.dim for c in cases} == set(CC.UPDATE_DIMS)
    assert {c.alpha for c in cases} == set(CC.UPDATE_ALPHAS) and {c.ne for c in cases} == {"one", "tenth", "all"}
    assert {c.costs for c in cases} == set(CC.COST_PATTERNS)
    pops = set(CC.UPDATE_POPS)
    # every pop class: below, at and above a power of two (63 / 64 / 65, 255 / 256 / 257, 1023 / 1024), and kBlock
    for p in (64, CC.K_BLOCK, CC.MAX_POP):
        assert {p - 1, p} <= pops and _pow2(p)
    assert {65, CC.K_BLOCK + 1} <= pops and {1, 2, 3} <= pops
    assert any(p < CC.K_BLOCK for p in pops) and any(CC.K_BLOCK < p for p in pops)
    # padding keys exist exactly where pop is no power of two; each such pop runs with every key an elite
    for p in pops:
        assert (CC.padded_pop(p) > p) == (not _pow2(p))
        if not _pow2(p):
            assert any(c.pop == p and c.ne == "all" for c in cases), p
    # +inf costs, every key an elite, padding keys in the sort: at a pop below a wave, below kBlock and above it
    hard = [c.pop for c in cases if c.costs == "inf_plus" and c.ne == "all" and not _pow2(c.pop)]
    assert any(p < CC.WAVE for p in hard) and any(p > CC.K_BLOCK for p in hard)
    assert any(c.M == 1 for c in cases) and any(c.M >= 2000 and c.pop <= 128 for c in cases)
    assert any(c.pop == 400 and c.dim == 10 and c.ne == "tenth" and c.alpha == 0.1 for c in cases)     # production
    for c in cases:
        assert c.what and 1 <= CC.num_elites_of(c) <= c.pop


def test_the_cost_patterns_hold_what_they_name():
    rng = np.random.RandomState(0)
    f32 = np.float32
    tiny = np.finfo(f32).tiny
    for pop in (2, 3, 65, 400):
        c = {p: CC.costs_of(p, rng, pop) for p in CC.COST_PATTERNS}
        assert all(v.dtype == f32 and v.shape == (pop,) for v in c.values())
        assert (np.diff(c["ascending"]) > 0).all() and (np.diff(c["descending"]) < 0).all() and len(set(c["equal"])) == 1
        assert np.isnan(c["all_nan"]).all()
        assert np.isnan(c["nan_1e6"]).any() and (c["nan_1e6"] == f32(1e6)).any()
        assert (c["nan_1e6"][~np.isnan(c["nan_1e6"])] >= f32(1e6)).all()
        assert np.isposinf(c["inf_plus"][[0, -1]]).all() and np.isneginf(c["inf_minus"][-1])
        z = c["signed_zero"]
        assert (z == 0).sum() >= 2 and np.signbit(z[z == 0]).any() and not np.signbit(z[z == 0]).all() and (z[z != 0] >= 1).all()
        d = c["denormal"]
        assert (d != 0).all() and (np.abs(d) < tiny).all() and len(set(d.tolist())) <= pop
        m = c["dup_min"]
        assert (m == m.min()).sum() == 2 and m[pop - 1] == m.min() and m[CC.dup_low(pop)] == m.min()
    # the inputs of a case: problem M inactive, all problems with costs of the case's pattern
    for case in CC.UPDATE_CASES:
        x = CC.update_inputs(case.name)
        assert x["samples"].shape == (case.M + 2, case.pop, case.dim) and x["active"].tolist() == [1] * case.M + [0, 1]


def test_the_set_table_reaches_its_edges():
    cases = CC.SET_CASES
    ns = {c.n for c in cases}
    assert set(CC.SET_NS) <= ns and {(c.dim, c.du) for c in cases} == set(CC.SET_DIMS)
    assert {c.mask for c in cases} == set(CC.MASK_PATTERNS)
    for edge in (CC.WAVE, CC.K_BEGIN_BLOCK, 2 * CC.K_BEGIN_BLOCK):
        assert {edge - 1, edge, edge + 1} <= ns or {edge, edge + 1} <= ns and any(n < edge for n in ns), edge
    assert {63, 64, 65, 1023, 1024, 1025, 2048, 2049} <= ns
    # cem_finish_kernel's grid stride: one case just over, every other case under
    over = [c for c in cases if c.n * c.dim > CC.K_MAX_GRID * CC.K_BLOCK]
    assert len(over) == 1 and over[0].n * over[0].dim < CC.STRIDE_ELEMENTS + 1024
    assert any(c.du == c.dim and c.dim > 1 for c in cases) and any(c.dim % c.du for c in cases)
    passes = lambda c: -(-c.n // CC.K_BEGIN_BLOCK)
    for c in cases:
        x = CC.set_inputs(c.name)
        mask, on = x["mask"], np.flatnonzero(x["mask"])
        assert c.what and mask.shape == (c.n,) and 1 <= c.du <= c.dim <= CC.MAX_DIM
        if c.mask == "zeros":
            assert on.size == 0
        if c.mask == "ones":
            assert on.size == c.n
        if c.mask == "none_first_1024":
            assert on.size > 1 and on.min() >= CC.K_BEGIN_BLOCK and passes(c) >= 2
        if c.mask == "last":
            assert on.tolist() == [c.n - 1]
        if c.mask == "first_last":
            assert on.tolist() == [0, c.n - 1]
        if c.mask == "random30":
            assert 0.2 < on.size / c.n < 0.4
        if c.mask == "wave_gap":
            assert mask[:64].all() and not mask[64:128].any() and mask[128:].any() and passes(c) >= 2
        if c.mask == "bytes":
            assert {2, 0x80, 255} <= set(mask.tolist()) and 0 in mask
    # base_sh carried into a later pass: zero, a full pass's 1024, and something between
    carried = set()
    for c in cases:
        mask = CC.set_inputs(c.name)["mask"]
        for p in range(1, passes(c)):
            if mask[p * CC.K_BEGIN_BLOCK:].any():
                carried.add(int((mask[:p * CC.K_BEGIN_BLOCK] != 0).sum()))
    assert 0 in carried and CC.K_BEGIN_BLOCK in carried and any(0 < b < CC.K_BEGIN_BLOCK for b in carried)
    # the chain and the captured round: set rows on both sides of the first pass
    for n, kind in CC.CHAIN["cases"]:
        m = CC.chain_mask(n, kind)
        assert m.shape == (n,) and 3 < m.sum() < n
    m = CC.chain_mask(1100, "spread")
    assert m[:CC.K_BEGIN_BLOCK].sum() > 3 and m[CC.K_BEGIN_BLOCK:].sum() > 3 and m[CC.K_BEGIN_BLOCK - 1] and m[CC.K_BEGIN_BLOCK]
    assert CC.CAPTURE["n"] > CC.K_BEGIN_BLOCK


# ---- the elite update: the float64 restatement is the oracle -------------------------------------------------------------------
@pytest.mark.parametrize("name", [c.name for c in CC.UPDATE_CASES])
def test_the_oracle_update_equals_the_restatement_bit_for_bit(name):
    """Both are sequential IEEE float64 sums in (cost, index) order with contraction off: every case is bit-equal (observed
    deviation 0 on all of them, so the derived bound 4 num_elites 2^-53 max|x| is not needed)."""
    c, x = CC.UPDATE_BY_NAME[name], CC.update_inputs(name)
    ne = CC.num_elites_of(c)
    got_m, got_v = co.cem_update(x["samples"], x["costs"], x["mean"], x["var"], ne, c.alpha, active=x["active"])
    ref_m, ref_v = CC.update_reference(name)
    assert got_m.tobytes() == ref_m.tobytes() and got_v.tobytes() == ref_v.tobytes()
    # the inactive problem keeps its values; an active one moves unless alpha = 1
    assert np.array_equal(ref_m[c.M], x["mean"][c.M]) and np.array_equal(ref_v[c.M], x["var"][c.M])
    if c.alpha == 1.0:
        assert np.array_equal(ref_m, x["mean"]) and np.array_equal(ref_v, x["var"])
    else:
        assert (ref_m[:c.M] != x["mean"][:c.M]).all() and (ref_m[c.M + 1] != x["mean"][c.M + 1]).all()
    assert np.isfinite(ref_m).all() and np.isfinite(ref_v).all() and (ref_v >= 0).all()
    # the elites by hand for the patterns whose order is known
    s = x["samples"][0].astype(np.float64)
    if c.costs in ("equal", "all_nan", "ascending"):
        want = s[:ne]
    elif c.costs == "descending":
        want = s[::-1][:ne]
    elif c.costs == "dup_min" and ne == 1:
        want = s[CC.dup_low(c.pop)][None]
    else:
        return
    em = want.sum(0) / ne if ne <= 2 else None
    if em is not None:                                           # one or two addends: the sum does not depend on its order
        assert np.array_equal(ref_m[0], c.alpha * x["mean"][0] + (1.0 - c.alpha) * em)
    else:
        assert np.allclose(ref_m[0], c.alpha * x["mean"][0] + (1.0 - c.alpha) * want.mean(0), rtol=1e-12, atol=1e-14)


def test_the_restatement_reproduces_the_references_iterations(golden_dir):
    """The two iterations captured from the reference (mpc_golden.npz), which reduces the float32 elites in float32."""
    G = np.load(os.path.join(golden_dir, "mpc_golden.npz"))
    for case in ("mid", "edge"):
        pre = "cem." + case + "."
        m, v = CC.restate_update(G[pre + "samples"][None], G[pre + "costs"][None], G[pre + "init_mean"][None],
                                 G[pre + "init_var"][None], int(G["cem.num_elites"]), float(G["cem.alpha"]))
        assert np.allclose(m[0], G[pre + "new_mean"], rtol=1e-5, atol=1e-6)
        assert np.allclose(v[0], G[pre + "new_var"], rtol=1e-4, atol=1e-7)


# ---- the sampling: the oracle's draws obey the specification ----------------------------------------------------------------
def _truncnorm(row, counter, d):
    """The specification of one draw: the Philox normal of (seed, row, STREAM_CEM, counter << 20 | d << 8 | attempt), redrawn
    while |z| > 2."""
    for attempt in range(256):
        z = co.normal2(CC.SEED, row, CC.STREAM_CEM, (counter << 20) | (d << 8) | attempt)[0]
        if -2.0 <= z <= 2.0:
            return z
    return min(2.0, max(-2.0, z))


@pytest.mark.parametrize("name", [c.name for c in CC.SAMPLE_CASES])
def test_the_oracle_draws_obey_the_specification(name):
    c, x = CC.SAMPLE_BY_NAME[name], CC.sample_inputs(name)
    n = CC.live_of(c)
    samples, active = CC.sample_oracle(name)
    mean, var, lb, ub = x["mean"][:n], x["var"][:n], x["lb"], x["ub"]
    assert samples.shape == (n, c.pop, c.dim) and samples.dtype == np.float32
    # activity: max(var) > epsilon, strictly; sticky: and active on entry
    want = var.max(1) > CC.EPSILON if n else np.zeros(0, bool)
    if c.sticky:
        want = want & (x["active_in"][:n] != 0)
    assert np.array_equal(active, want.astype(np.uint8))
    if x["expect_active"] is not None:
        assert active.tolist() == x["expect_active"][:n]
    on = active.astype(bool)
    assert not samples[~on].any()                                           # inactive problems are untouched
    cv = np.minimum(CC.clamp_of(mean, lb, ub), var)                         # optimizers.py:95-99
    sd = np.sqrt(cv)
    s64 = samples.astype(np.float64)
    exact = (cv == 0)[:, None, :] & on[:, None, None]
    assert np.array_equal(np.broadcast_to(mean.astype(np.float32)[:, None, :], samples.shape)[np.broadcast_to(exact, samples.shape)],
                          samples[np.broadcast_to(exact, samples.shape)])
    if "on_ub" in c.setup or "on_lb" in c.setup:
        assert exact[0].all() and exact.sum() == c.dim + (c.M - 1) * c.dim // 2          # per candidate
    drawn = np.broadcast_to((cv > 0)[:, None, :] & on[:, None, None], samples.shape)
    with np.errstate(divide="ignore", invalid="ignore"):
        z = (s64 - mean[:, None, :]) / sd[:, None, :]
        slack = 2.0 ** -23 * np.abs(s64) / sd[:, None, :]                   # the rounding of the sample to float32
    assert drawn.sum() > 0 or not on.any()
    assert (np.abs(z[drawn]) <= 2.0 + slack[drawn]).all()
    if drawn.sum() > 1000:
        assert abs(z[drawn].mean()) < 0.1 and 0.8 < z[drawn].std() < 0.95    # N(0, 1) truncated at +-2: sd 0.8796
    # a handful of elements recomputed from the Philox stream: row = m pop + i, dimension d, the summed counter -- bit for bit
    rng = np.random.RandomState(1)
    where = np.argwhere(drawn)
    picks = where[rng.choice(len(where), min(24, len(where)), replace=False)] if len(where) else []
    last = np.argwhere(drawn)[-1:] if len(where) else []
    for m, i, d in list(picks) + list(last):
        zz = _truncnorm(int(m) * c.pop + int(i), CC.oracle_counter(c), int(d))
        assert np.float32(zz * np.sqrt(cv[m, d]) + mean[m, d]) == samples[m, i, d], (m, i, d)


def test_sticky_and_counter_cases_differ_as_they_should():
    one, zero = CC.sample_oracle("sticky-1"), CC.sample_oracle("sticky-0")
    assert one[1].tolist() == [0, 0, 1, 0] and zero[1].tolist() == [1, 0, 1, 0]
    assert np.array_equal(one[0][2], zero[0][2]) and zero[0][0].any() and not one[0][0].any()
    # the same inputs at the same summed counter draw the same samples, at another counter others
    s = {n: CC.sample_oracle(n)[0] for n in ("count-host", "count-tick", "count-both-inc1", "count-both-inc3", "mdev-5of5")}
    assert np.array_equal(s["count-host"], s["count-tick"]) and np.array_equal(s["count-both-inc1"], s["count-both-inc3"])
    assert np.array_equal(s["count-host"], s["count-both-inc1"]) and not np.array_equal(s["count-host"], s["mdev-5of5"])
    assert CC.tick_after(CC.SAMPLE_BY_NAME["mdev-0"]) == 7 and CC.tick_after(CC.SAMPLE_BY_NAME["mdev-2of5"]) == 10
    assert CC.tick_after(CC.SAMPLE_BY_NAME["count-host"]) is None and CC.tick_after(CC.SAMPLE_BY_NAME["count-inc0"]) == 7


# ---- begin and finish: the restatements are MPC.act's host-count arithmetic ---------------------------------------------------
@pytest.mark.parametrize("name", ["n65-dim10-du2-random30", "n4173-dim7-du3-bytes"])
def test_the_restatements_are_the_host_count_path_of_act(name):
    """MPC.act without a device count: idx = mask.nonzero(), obtain_solution(prev_sol[idx], init_var.expand(...)), then the shift
    and the scatter of MPC.py:281-285, here with torch on the CPU and the case's `mean` for the optimiser's solution."""
    c, x, ref = CC.SET_BY_NAME[name], CC.set_inputs(name), CC.set_reference(name)
    t = lambda a: torch.from_numpy(np.array(a))
    mask, prev_sol, obs = t(x["mask"]), t(x["prev_sol"]), t(x["obs"])
    idx = mask.bool().nonzero().squeeze(1)
    count = idx.numel()
    b = ref["begin"]
    assert int(b["count"][0]) == count > 0 and np.array_equal(b["idx"][:count], idx.numpy())
    assert np.array_equal(b["mean"][:count], prev_sol[idx].numpy())
    assert np.array_equal(b["var"][:count], t(x["init_var"]).expand(count, -1).numpy())
    assert np.array_equal(b["cur_obs"][:count], obs[idx].contiguous().numpy()) and (b["active"][:count] == 1).all()
    for k, fill in (("idx", CC.S_IDX), ("mean", CC.S_F64), ("var", CC.S_F64), ("cur_obs", CC.S_OBS), ("active", CC.S_ACTIVE)):
        assert (b[k][count:] == fill).all() and b[k].shape[0] == c.n, k
    soln = t(x["mean"])[:count]
    out = torch.zeros(c.n, c.du, dtype=torch.float32)
    shifted = torch.cat([soln[:, c.du:], torch.zeros(count, c.du, dtype=soln.dtype)], dim=1)
    prev_sol[idx] = shifted
    out[idx] = soln[:, :c.du].to(torch.float32)
    assert np.array_equal(ref["action"], out.numpy()) and np.array_equal(ref["prev_sol"], prev_sol.numpy())
    assert not (ref["action"] == CC.S_ACTION).any() and np.abs(ref["prev_sol"]).max() <= 1.0


def test_finish_after_an_empty_mask_restated():
    for c in CC.SET_CASES:
        if c.mask == "zeros":
            ref, x = CC.set_reference(c.name), CC.set_inputs(c.name)
            assert int(ref["begin"]["count"][0]) == 0 and not ref["action"].any() and ref["action"].shape == (c.n, c.du)
            assert np.array_equal(ref["prev_sol"], x["prev_sol"])
