"""rrl_plan_pack / rrl_plan_cost at kernel level, through their descriptors alone, on every case of plan_cases.py: costs and the
three quantities the kernels leave in `scratch` (q0, e0, partial) against the float64 restatement under rule 1 in both
precisions, with guard values in and behind every output; then what the sources promise bit for bit -- a group's results do
not depend on where in the launch it sits as long as bit 2 of its index is kept, the device count, the host and device ticks,
the in-kernel Philox stream, a NaN draw nothing reads, a re-packed buffer.  test_plan_paths_cpu.py proves that the table
reaches every launch edge and that rule 1 catches a kernel that is wrong."""
import numpy as np
import pytest
import torch

import plan_cases as PC
from oracle import c_oracle

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HOR = 5
_planners = {}


def planner(n_nets=5):
    if n_nets not in _planners:
        _planners[n_nets] = PC.Planner(PC.weights(n_nets), DEV)
    return _planners[n_nets]


def run_case(name, f16x3, **kw):
    case = PC.BY_NAME[name]
    obs, acs, noise = PC.inputs(name)
    return planner(case.n_nets).run(f16x3, obs, acs, noise, case.plan_hor, **kw)


def written(t):
    return bool((t != PC.GUARD).all())


# ---- values ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f16x3", PC.PRECISIONS)
@pytest.mark.parametrize("name", PC.names())
def test_costs_and_scratch_against_float64(name, f16x3):
    case = PC.BY_NAME[name]
    r = run_case(name, f16x3)
    out, report = r["out"], []
    bad = PC.compare(name, out, f16x3, report)
    for k, dev, bound, ratio in report:                      # (kept by the run that fills LAB_NOTES.md)
        print("RATIO %s %s %s dev=%.3e bound=%.3e ratio=%.2f" % (name, "f16x3" if f16x3 else "f32", k, dev, bound, ratio))
    assert r["tails"], "written behind the end of costs or scratch"
    assert written(out.costs) and written(out.partial) and written(out.q0)
    if case.plan_hor == 1:                                   # the first-step kernel skips the members: nothing writes e0
        assert bool((out.e0 == PC.GUARD).all())
    else:
        assert written(out.e0)
    assert not bad, (bad, report)


# ---- placement, bit for bit -------------------------------------------------------------------------------------------------
def _bases(pop):
    """The base envs of a placement launch, each with obs, actions and noise rows of its own: 8 envs of one candidate, or two
    envs of pop (a multiple of 8) candidates, which the launch alternates."""
    envs = PC.PLACEMENT["bases"] if pop == 1 else 2
    return PC.make_inputs(envs, pop, HOR, 20, seed=900 + pop)


def _tile_envs(obs, acs, noise, order):
    """The launch whose env i is base env order[i]."""
    per = acs.shape[1] * 20
    z = noise.reshape(HOR, obs.shape[0], per, 2)
    return obs[order], acs[order], z[:, order].reshape(HOR, -1, 2)


@pytest.mark.parametrize("f16x3", PC.PRECISIONS)
@pytest.mark.parametrize("M,pop", PC.PLACEMENT["launches"])
def test_a_group_computes_the_same_bits_wherever_it_sits_at_its_parity(M, pop, f16x3):
    """Copies of 8 base groups at every position that keeps bit 2 of the group index: through the first and last blocks of both
    kernels, the ragged tail and the tiles with the flipped phase order."""
    obs, acs, noise = _bases(pop)
    envs = obs.shape[0]
    p = planner()
    small = p.run(f16x3, obs, acs, noise, HOR)["out"]
    order = torch.arange(M) % envs
    big = p.run(f16x3, *_tile_envs(obs, acs, noise, order), HOR)
    assert big["tails"]
    out = big["out"]
    gsrc = (order[:, None] * pop + torch.arange(pop)[None, :]).reshape(-1).to(DEV)       # group g of the launch is base gsrc[g]
    assert bool((((torch.arange(M * pop, device=DEV) >> 2) & 1) == ((gsrc >> 2) & 1)).all())
    want = PC.Out(small.costs.reshape(-1)[gsrc].view(M, pop), small.partial[gsrc], small.q0[gsrc], small.e0[gsrc])
    assert not PC.same_bits(out, want), PC.same_bits(out, want)


@pytest.mark.parametrize("f16x3", PC.PRECISIONS)
def test_a_group_at_the_other_parity_agrees_under_rule_one(f16x3):
    """Base b placed at b ^ 4: the member's last layer adds its 13th column tile into another strip, so the bits may differ;
    the values obey rule 1 against the float64 restatement of the bases."""
    obs, acs, noise = _bases(1)
    order = torch.arange(8) ^ 4
    got = planner().run(f16x3, *_tile_envs(obs, acs, noise, order), HOR)["out"]
    back = order.to(DEV)                                       # b ^ 4 is its own inverse
    got = PC.Out(got.costs[back], got.partial[back], got.q0[back], got.e0[back])
    w = PC.weights(5)
    r64, r32 = (PC.restate(w, obs, acs, noise, 20, 5, HOR, dtype=d) for d in (torch.float64, torch.float32))
    res = PC.rule1(got, r64, r32, f16x3)
    assert not PC.broken(res), res


# ---- the device count -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f16x3", PC.PRECISIONS)
@pytest.mark.parametrize("live", PC.DEVICE_COUNT["live"])
def test_the_device_count_computes_the_live_problems_and_touches_nothing_else(live, f16x3):
    M, pop, inc = PC.DEVICE_COUNT["M"], PC.DEVICE_COUNT["pop"], 3
    p = planner()
    obs, acs, _ = PC.make_inputs(M, pop, HOR, 20, seed=700)
    noise = torch.randn(HOR, max(live, 1) * pop * 20, 2, generator=torch.Generator().manual_seed(live))
    count = torch.tensor([live], dtype=torch.int32, device=DEV)
    tick = torch.zeros(2, dtype=torch.int64, device=DEV)
    dev = p.run(f16x3, obs, acs, noise, HOR, m_dev=count, counter_dev=tick, counter_inc=inc)
    assert dev["tails"]
    out, n = dev["out"], live * pop
    assert tick.tolist() == [inc if live else 0, 0]
    for t in (out.costs.reshape(-1), out.partial, out.q0, out.e0):
        assert bool((t[n:] == PC.GUARD).all()), "written past the live groups"
    if live:
        tick0 = torch.zeros(2, dtype=torch.int64, device=DEV)
        host = p.run(f16x3, obs[:live], acs[:live], noise, HOR, counter_dev=tick0, counter_inc=inc)["out"]
        assert tick0.tolist() == [inc, 0]
        assert torch.equal(out.costs[:live], host.costs)
        assert torch.equal(out.partial[:n], host.partial) and torch.equal(out.q0[:n], host.q0) and torch.equal(out.e0[:n], host.e0)


# ---- counters and the in-kernel Philox noise --------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def philox():
    """The documented stream for the PHILOX case at its ticks: normals(seed, rows, RRL_STREAM_PLAN, tick * 16 + t) cast to f32."""
    case = PC.BY_NAME[PC.PHILOX["case"]]
    rows = PC.groups_of(case) * PC.npart_of(case)
    z = {}
    for tick in PC.PHILOX["ticks"]:
        steps = [c_oracle.normals(PC.PHILOX["seed"], rows, PC.STREAM_PLAN, tick * 16 + t) for t in range(case.plan_hor)]
        z[tick] = torch.as_tensor(np.stack(steps).astype(np.float32))
    return z


@pytest.mark.parametrize("f16x3", PC.PRECISIONS)
def test_null_noise_is_the_documented_philox_stream_and_the_ticks_add_up(philox, f16x3):
    name, seed = PC.PHILOX["case"], PC.PHILOX["seed"]
    case = PC.BY_NAME[name]
    obs, acs, _ = PC.inputs(name)
    p = planner()
    last = max(PC.PHILOX["ticks"])
    for tick_value in PC.PHILOX["ticks"]:
        want = p.run(f16x3, obs, acs, philox[tick_value], case.plan_hor)["out"]
        tick = torch.tensor([tick_value, 0], dtype=torch.int64, device=DEV)
        got = p.run(f16x3, obs, acs, None, case.plan_hor, seed=seed, counter_dev=tick, counter_inc=3)
        assert got["tails"] and not PC.same_bits(got["out"], want), (tick_value, PC.same_bits(got["out"], want))
        assert tick.tolist() == [tick_value + 3, 0]          # counter_inc = 3
    # the host's counter field alone, and host + device tick
    host = p.run(f16x3, obs, acs, None, case.plan_hor, seed=seed, counter=last)["out"]
    assert not PC.same_bits(host, want)
    tick = torch.tensor([1, 0], dtype=torch.int64, device=DEV)
    both = p.run(f16x3, obs, acs, None, case.plan_hor, seed=seed, counter=last - 1, counter_dev=tick, counter_inc=1)["out"]
    assert not PC.same_bits(both, want) and tick.tolist() == [2, 0]
    # another seed draws other noise
    other = p.run(f16x3, obs, acs, None, case.plan_hor, seed=seed + 1, counter=last)["out"]
    assert float((other.costs - want.costs).abs().mean()) > 1e-4


# ---- NaN ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f16x3", PC.PRECISIONS)
@pytest.mark.parametrize("name", PC.names(PC.NAN_CASES))
def test_one_nan_particle_counts_as_1e6_in_its_candidate_alone(name, f16x3):
    case = PC.BY_NAME[name]
    step, group, particle = case.nan
    r = run_case(name, f16x3)
    out, report = r["out"], []
    bad = PC.compare(name, out, f16x3, report)
    assert r["tails"] and not bad, (bad, report)
    assert not bool((out.costs != out.costs).any())
    if step == case.plan_hor - 1:
        # nothing reads the last step's draw: the same bits as the launch without the NaN
        obs, acs, noise = PC.inputs(name)
        clean = PC.make_inputs(case.M, case.pop, case.plan_hor, PC.npart_of(case), seed=PC.INPUT_SEEDS.get(name, 0))[2]
        assert int((clean != noise).sum()) == 2 and not bool((clean != clean).any())
        want = planner().run(f16x3, obs, acs, clean, case.plan_hor)["out"]
        assert not PC.same_bits(out, want)
    else:
        member = particle // PC.PPN
        hit = out.partial >= 0.5 * PC.NAN_COST
        assert hit.nonzero().tolist() == [[group, member]]
        assert float(out.costs.reshape(-1)[group]) > PC.NAN_COST / PC.npart_of(case)


# ---- pack -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f16x3", PC.PRECISIONS)
def test_a_repacked_buffer_gives_the_bits_of_a_fresh_one(f16x3):
    """packed filled with NaN, then packed in one precision, the other, and the first again: the same costs as from a zeroed
    buffer packed once.  (Costs only: the f32 pack leaves the slots of kEW1 / kEW2 it does not use unwritten, by design.)"""
    name = "M9-pop13"
    case = PC.BY_NAME[name]
    obs, acs, noise = PC.inputs(name)
    p = planner()
    want = p.run(f16x3, obs, acs, noise, case.plan_hor)["out"].costs
    packed = torch.full((p.packed_floats + PC.GUARD_TAIL,), float("nan"), dtype=torch.float32, device=DEV)
    for precision in (f16x3, not f16x3, f16x3):
        p.pack(precision, packed)
    got = p.run(f16x3, obs, acs, noise, case.plan_hor, packed=packed)
    tail = packed[p.packed_floats:]
    assert bool((tail != tail).all()), "written behind the end of packed"
    assert got["tails"] and torch.equal(got["out"].costs, want)
    assert not PC.compare(name, got["out"], f16x3)
