"""Cases, float64 restatement, launch helper, launch facts and the two comparison rules for the planner cost kernels
(csrc/plan_kernels.hip: plan_first_step_kernel, plan_cost_kernel, plan_finish_kernel in both precisions and the five pack kernels,
behind rrl_plan_pack / rrl_plan_cost), shared by test_plan_paths_cpu.py and test_plan_paths_gpu.py.

restate() is the whole operation from raw tensors -- the specification above rrl_plan_cost in include/rrl_hip.h with
MPC._compile_cost_chunk, _predict_next_obs and _expand_to_ts_format: every (env m, candidate c, particle p) row runs plan_hor
steps of
    cost += max(sigmoid Q1, sigmoid Q2)(obs, ac_t);   obs += mean_e(obs, ac_t) + z_t sqrt(var_e(obs, ac_t)),   e = p // 4,
a NaN particle cost counts as 1e6, and costs[m, c] is the mean over the particles.  It is the literal loop: no step is shared
between the particles and the last step's prediction is computed although nothing reads it.  Besides the costs it returns what
the kernels leave in `scratch`: q0[group], e0[group][member] = {mean dx, mean dy, sd x, sd y} of step 0 and
partial[group][member] = the sum of the member's four particle costs.  dtype = torch.float32 runs the same code in f32: the
plain f32 reference of rule 1.

The library does not say which workgroup computed what.  launch_facts() restates what a launch depends on (the tile counts of
both kernels, the tiles with the flipped phase order, the groups that share a tile with another env, the groups of a ragged
last block) with the constants as literals; test_plan_paths_cpu.py parses the constants out of the sources and proves that the
case table reaches every edge.

Rule 1 (against float64, per case and per quantity -- costs, partial, q0, the means of e0, the sds of e0): the kernel's largest
absolute deviation from float64 is at most FACTOR = 4 times the basis, the basis the larger of the f32 restatement's largest
absolute deviation from float64 on the same case and 2^-23 times the largest float64 magnitude of the quantity.  The factor: the
kernel's sigmoid and swish go through the 1-ulp v_rcp_f32 and __expf where torch divides and calls expf, and its reductions run
in another order -- a few ulp per activation against one; it is a margin over the reference, not a measurement of the kernel.
An f16x3 launch adds the agreement the project claims between its two kernels (2e-5 absolute on costs, test_plan_gpu.py): the
same on q0 (one of the cost's terms), times 4 on partial (a sum of four costs), and 2e-5 of the quantity's largest magnitude on
e0.  The f32 restatement must itself lie within CAP = 5e-6 of float64 on the costs of every case (test_plan_paths_cpu.py), so
the f32 bound never exceeds 2e-5.  Rule 2 is torch.equal wherever the sources promise the same bits.

A candidate that holds a NaN particle is compared by nan_bound() instead: its sums hold 1e6, whose ulp is 0.0625."""
import collections
import ctypes as C
import functools

import torch
from torch.nn import functional as F

# ---- the launch's constants, as literals (test_plan_paths_cpu.py compares them with the sources) ---------------------------
CONSTANTS = dict(kRows=64, cost_block=16, order_shift=8, max_plan_hor=16, kHQ=256, kHE=200, kHEPad=208, kEBlocks32=7,
                 particles_per_net=4)
FIRST_ROWS, COST_GROUPS, ORDER_SHIFT, MAX_HOR, HQ, HE, PPN = 64, 16, 8, 16, 256, 200, 4
STREAM_PLAN = 7               # RRL_STREAM_PLAN

WEIGHT_NAMES = ("q_w1", "q_b1", "q_w2", "q_b2", "q_w3", "q_b3", "e_w0", "e_b0", "e_w1", "e_b1", "e_w2", "e_b2", "e_w3", "e_b3",
                "inputs_mu", "inputs_sigma", "max_logvar", "min_logvar")
QUANTITIES = ("costs", "partial", "q0", "e0_mean", "e0_sd")
FACTOR, CAP = 4.0, 5e-6
F16X3_COSTS = 2e-5            # the agreement of the two kernels on costs (tests/test_plan_gpu.py)
NAN_COST = 1e6
GUARD = -1234.5               # no cost, sum, sigmoid or sd can be negative: a float that was written cannot hold it
GUARD_TAIL = 256              # floats of GUARD behind every output

Out = collections.namedtuple("Out", "costs partial q0 e0")


def ceil_div(a, b):
    return -(-a // b)


# ---- the case table -----------------------------------------------------------------------------------------------------------
# nan: None, or (step, group, particle) of the one noise row that is NaN.  npart = 4 n_nets.
Case = collections.namedtuple("Case", "name M pop plan_hor n_nets nan", defaults=(5, 5, None))


def _cases():
    out = []
    # ragged last blocks of 16 and of 64 groups around one block
    for pop in (1, 15, 16, 17, 63, 64, 65):
        out.append(Case("M1-pop%d" % pop, 1, pop))
    # env boundaries inside tiles, the groups' parity (bit 2 of the group index) shifts from env to env
    out += [Case("M5-pop7", 5, 7), Case("M9-pop13", 9, 13)]
    # 52 blocks of 16 groups x 5 members = 260 tiles: tiles 256..259 run the flipped phase order, the last block is ragged
    out += [Case("M1-pop821", 1, 821), Case("M821-pop1", 821, 1), Case("M7-pop117", 7, 117)]
    for hor in (1, 2, 3, 16):
        out.append(Case("hor%d" % hor, 3, 23, plan_hor=hor))
    for nets in (1, 2, 7):
        out.append(Case("nets%d" % nets, 3, 23, plan_hor=3, n_nets=nets))
    return out


VALUE_CASES = _cases()
# one NaN noise row: particle 7 (member 1, its last particle) of group 30 (env 1, in the middle of a 16-group block)
NAN_CASES = [Case("nan-step0", 3, 23, nan=(0, 30, 7)), Case("nan-step3", 3, 23, nan=(3, 30, 7)),
             Case("nan-last", 3, 23, nan=(4, 30, 7))]
CASES = VALUE_CASES + NAN_CASES
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
PRECISIONS = (False, True)                                   # rrl_plan_cost_t.f16x3
# launches that are no value cases (test_plan_paths_gpu.py): the device count, the in-kernel Philox noise, the placement
DEVICE_COUNT = dict(M=40, pop=23, live=(0, 1, 39, 40))
PHILOX = dict(case="M7-pop117", ticks=(0, 3), seed=0x706C616E ^ 12345)
PLACEMENT = dict(bases=8, launches=((821, 1), (103, 8)))       # (M, pop): pop = 1 and pop = 8, 821 and 824 groups


def names(cases=None):
    return [c.name for c in (VALUE_CASES if cases is None else cases)]


def npart_of(case):
    return PPN * case.n_nets


def groups_of(case):
    return case.M * case.pop


# ---- the launch, restated -----------------------------------------------------------------------------------------------------
def supported(n_nets, npart):
    """rrl_plan_supported at hq = 256, he = 200, 2-D obs and actions."""
    return n_nets > 0 and npart % n_nets == 0 and npart // n_nets == PPN


def launch_facts(M, pop, n_nets, plan_hor):
    """What rrl_plan_cost launches for M x pop groups, from the host code and the two kernels' index arithmetic.
    cost kernel: tile = blockIdx.x, e = tile % n_nets, gblock = tile / n_nets, group = 16 gblock + tid / 4,
    order = (blockIdx.x >> 8) & 1; first-step kernel: net = tile % (n_nets + 1), gblock = tile / (n_nets + 1),
    group = 64 gblock + tid; both: m = group / pop."""
    groups = M * pop
    cost_blocks, first_blocks = ceil_div(groups, COST_GROUPS), ceil_div(groups, FIRST_ROWS)
    cost_tiles, first_tiles = cost_blocks * n_nets, first_blocks * (n_nets + 1)
    order1_tiles = [t for t in range(cost_tiles) if (t >> ORDER_SHIFT) & 1]
    block_groups = lambda b, size: range(b * size, min(groups, (b + 1) * size))
    order_of_group = {}                                    # group -> the set of `order` its members' tiles run with
    for t in range(cost_tiles):
        for g in block_groups(t // n_nets, COST_GROUPS):
            order_of_group.setdefault(g, set()).add((t >> ORDER_SHIFT) & 1)
    shared = lambda size, blocks: sorted(g for b in range(blocks) if len({g // pop for g in block_groups(b, size)}) > 1
                                         for g in block_groups(b, size))
    ragged = lambda size, blocks: list(block_groups(blocks - 1, size)) if groups % size else []
    return dict(groups=groups, cost_tiles=cost_tiles, first_tiles=first_tiles, order1_tiles=order1_tiles,
                orders={o for s in order_of_group.values() for o in s},
                groups_order1=sorted(g for g, s in order_of_group.items() if 1 in s),
                shared16=shared(COST_GROUPS, cost_blocks), shared64=shared(FIRST_ROWS, first_blocks),
                ragged16=ragged(COST_GROUPS, cost_blocks), ragged64=ragged(FIRST_ROWS, first_blocks),
                parities={(g >> 2) & 1 for g in range(groups)},
                # bit 2 of the group index of candidate 0 of every env: a per-env launch would change it where it is 1
                env_start_parities={((m * pop) >> 2) & 1 for m in range(M)},
                members_run=plan_hor > 1, loop_steps=max(0, plan_hor - 1), predicts=max(0, plan_hor - 2))


def case_facts(case):
    return launch_facts(case.M, case.pop, case.n_nets, case.plan_hor)


def scratch_floats(n_nets, M, pop):
    return M * pop * (5 * n_nets + 1)


def split_scratch(scratch, groups, n_nets):
    """The comment in rrl_plan_cost: e0 [groups][n_nets][4] | partial [groups][n_nets] | q0 [groups] -> (e0, partial, q0)."""
    a, b = groups * n_nets * 4, groups * n_nets * 5
    return scratch[:a].view(groups, n_nets, 4), scratch[a:b].view(groups, n_nets), scratch[b:b + groups]


# ---- weights and inputs -------------------------------------------------------------------------------------------------------
# Both soft clamps must bite at step 0 (test_plan_paths_cpu.py: 5 % of the raw log-variances above MAX_LOGVAR, 5 % below
# MIN_LOGVAR).  With lin3_w x 3 alone a member's raw log-variance is its own level +- 0.02 whatever the input; the two
# log-variance columns of lin3_w are therefore x LOGVAR_GAIN more, which spreads a member's values by about 0.1 (standard
# deviation) around its level, the members' levels over about +- 1
LOGVAR_GAIN = 5.0
MAX_LOGVAR, MIN_LOGVAR = (0.12, 0.1), (-0.14, -0.1)
INPUTS_MU, INPUTS_SIGMA = (-0.5, 0.3, 0.05, -0.04), (1.5, 1.0, 0.6, 0.55)


# the seed of an ensemble size's weights where seed 0 is not fair (one member alone: all its raw log-variances on one side)
WEIGHT_SEEDS = {1: 8}


@functools.lru_cache(maxsize=None)
def weights(n_nets, seed=None):
    """The 18 tensors of rrl_plan_weights_t (f32, on the host; shapes as include/rrl_hip.h lists them), spread like build() of
    test_plan_gpu.py: Xavier critic weights x 2.5 (default inits give sigmoid ~ 0.5 everywhere), ensemble weights
    N(0, 1 / (4 fan_in)) with lin3_w x 3 and biases N(0, 0.1), mu and sigma not 0 and 1.  Shared, never modified."""
    seed = WEIGHT_SEEDS.get(n_nets, 0) if seed is None else seed
    g = torch.Generator().manual_seed(7919 * seed + n_nets)
    uni = lambda bound, *shape: (torch.rand(*shape, generator=g) * 2 - 1) * bound
    nrm = lambda std, *shape: torch.randn(*shape, generator=g) * std
    xav = lambda out, inp: 2.5 * (6.0 / (out + inp)) ** 0.5
    w = dict(q_w1=uni(xav(HQ, 4), 2, HQ, 4), q_b1=uni(0.25, 2, HQ), q_w2=uni(xav(HQ, HQ), 2, HQ, HQ), q_b2=uni(0.25, 2, HQ),
             q_w3=uni(xav(1, HQ), 2, 1, HQ), q_b3=uni(0.25, 2, 1),
             e_w0=nrm(0.5 / 4 ** 0.5, n_nets, 4, HE), e_b0=nrm(0.1, n_nets, 1, HE),
             e_w1=nrm(0.5 / HE ** 0.5, n_nets, HE, HE), e_b1=nrm(0.1, n_nets, 1, HE),
             e_w2=nrm(0.5 / HE ** 0.5, n_nets, HE, HE), e_b2=nrm(0.1, n_nets, 1, HE),
             e_w3=nrm(3 * 0.5 / HE ** 0.5, n_nets, HE, 4), e_b3=nrm(0.1, n_nets, 1, 4),
             inputs_mu=torch.tensor(INPUTS_MU), inputs_sigma=torch.tensor(INPUTS_SIGMA),
             max_logvar=torch.tensor(MAX_LOGVAR), min_logvar=torch.tensor(MIN_LOGVAR))
    w["e_w3"][:, :, 2:] *= LOGVAR_GAIN
    assert tuple(w) == WEIGHT_NAMES and all(t.dtype == torch.float32 for t in w.values())
    return w


def make_inputs(M, pop, plan_hor, npart, seed):
    """cur_obs [M, 2], ac_seqs [M, pop, 2 plan_hor], noise [plan_hor, M pop npart, 2] (f32, on the host), spread like inputs()
    of test_plan_gpu.py."""
    g = torch.Generator().manual_seed(104729 * seed + 1000 * M + pop + 31 * plan_hor + 7 * npart)
    acs = torch.rand(M, pop, plan_hor * 2, generator=g) * 2 - 1
    obs = torch.randn(M, 2, generator=g) * torch.tensor([1.5, 1.0]) + torch.tensor([-0.5, 0.3])
    noise = torch.randn(plan_hor, M * pop * npart, 2, generator=g)
    return obs, acs, noise


# the seed of a case's inputs where seed 0 is not fair to the kernel (fairness(): a single candidate sees one observation, so
# one critic head may win every row, or no raw log-variance may reach a clamp), to be found by trying 1, 2, ... on the host;
# seed 0 is fair for every case of the present table
INPUT_SEEDS = {}


@functools.lru_cache(maxsize=None)
def inputs(name):
    """The inputs of a table case (a NaN case: its one noise row planted): computed once, shared, never modified."""
    case = BY_NAME[name]
    obs, acs, noise = make_inputs(case.M, case.pop, case.plan_hor, npart_of(case), seed=INPUT_SEEDS.get(name, 0))
    if case.nan:
        step, group, particle = case.nan
        noise[step, group * npart_of(case) + particle] = float("nan")
    return obs, acs, noise


# ---- the restatement ----------------------------------------------------------------------------------------------------------
MUTATIONS = ("member_mod", "noise_swap", "action_prev", "min_heads", "drop_last_q", "obs_not_accumulated", "no_max_clamp",
             "noise_group_offset", "nan_after_mean")


def restate(w, cur_obs, ac_seqs, noise, npart, n_nets, plan_hor, dtype=torch.float64, mutation=None, trace=None):
    """-> Out(costs [M, pop], partial [groups, n_nets], q0 [groups], e0 [groups, n_nets, 4]) in `dtype`.
    mutation: one of MUTATIONS, a way of being wrong (test_plan_paths_cpu.py shows that rule 1 catches each).
    trace: a dict that receives q [plan_hor, groups, npart] (the critic's value along the rollout), heads [plan_hor, groups,
    npart, 2] (the two heads), logvar0 [groups, n_nets, 2] (the raw log-variances of step 0) and particle_costs [groups,
    npart] (before the NaN replacement)."""
    assert mutation is None or mutation in MUTATIONS
    W = {k: v.to(dtype) for k, v in w.items()}
    M, pop = ac_seqs.shape[0], ac_seqs.shape[1]
    G, ppn = M * pop, npart // n_nets
    acs = ac_seqs.to(dtype).reshape(G, plan_hor, 2)
    obs = cur_obs.to(dtype)[:, None, None, :].expand(M, pop, npart, 2).reshape(G, npart, 2)
    z = noise.to(dtype).reshape(plan_hor, G, npart, 2)            # row = (m pop + c) npart + p
    if mutation == "noise_swap" and n_nets > 1:                   # particle 0 (member 0) <-> particle ppn (member 1)
        z = z.clone()
        z[:, :, [0, ppn]] = z[:, :, [ppn, 0]]
    if mutation == "noise_group_offset":
        z = z.roll(1, dims=1)
    p = torch.arange(npart)
    member = p % n_nets if mutation == "member_mod" else p // ppn     # TS-infinity: particle p rides member p // 4
    owned = [(member == e).nonzero().flatten() for e in range(n_nets)]
    cost = torch.zeros(G, npart, dtype=dtype)
    q0 = e0 = None
    for t in range(plan_hor):
        ac = acs[:, max(t - 1, 0) if mutation == "action_prev" else t]
        x = torch.cat((obs, ac[:, None, :].expand(G, npart, 2)), dim=-1)            # [G, P, 4]
        # Q_risk: twin heads 4 -> 256 relu -> 256 relu -> 1 sigmoid, the larger of the two (torch.max: NaN propagates)
        heads = []
        for h in range(2):
            a = F.relu(x @ W["q_w1"][h].T + W["q_b1"][h])
            a = F.relu(a @ W["q_w2"][h].T + W["q_b2"][h])
            heads.append(torch.sigmoid(a @ W["q_w3"][h].T + W["q_b3"][h]).squeeze(-1))
        q = torch.minimum(*heads) if mutation == "min_heads" else torch.maximum(*heads)
        if not (mutation == "drop_last_q" and t == plan_hor - 1):
            cost = cost + q
        # the particle's member: 4 -> 200 swish -> 200 swish -> 200 swish -> 4 on the standardised (obs, ac)
        xn = (x - W["inputs_mu"]) / W["inputs_sigma"]
        mean, sd, raw = torch.empty(G, npart, 2, dtype=dtype), torch.empty(G, npart, 2, dtype=dtype), torch.empty(G, npart, 2, dtype=dtype)
        for e in range(n_nets):
            a = xn[:, owned[e]]
            for k in range(3):
                a = a @ W["e_w%d" % k][e] + W["e_b%d" % k][e]
                a = a * torch.sigmoid(a)
            a = a @ W["e_w3"][e] + W["e_b3"][e]
            lv = a[..., 2:]
            raw[:, owned[e]] = lv
            if mutation != "no_max_clamp":
                lv = W["max_logvar"] - F.softplus(W["max_logvar"] - lv)
            lv = W["min_logvar"] + F.softplus(lv - W["min_logvar"])
            mean[:, owned[e]] = a[..., :2]
            sd[:, owned[e]] = torch.exp(lv).sqrt()
        if t == 0:
            first = torch.stack([o[0] for o in owned])                               # every particle of a member agrees at t = 0
            q0 = q[:, 0]
            e0 = torch.cat((mean[:, first], sd[:, first]), dim=-1)
            if trace is not None:
                trace["logvar0"] = raw[:, first]
        if trace is not None:
            trace.setdefault("q", []).append(q)
            trace.setdefault("heads", []).append(torch.stack(heads, -1))
        pred = mean + z[t] * sd
        obs = pred if mutation == "obs_not_accumulated" else obs + pred              # obs_postproc: obs + prediction
    if trace is not None:
        trace["q"], trace["heads"], trace["particle_costs"] = torch.stack(trace["q"]), torch.stack(trace["heads"]), cost
    if mutation == "nan_after_mean":
        partial = torch.stack([cost[:, o].sum(1) for o in owned], dim=1)
        costs = cost.mean(1)
        costs = torch.where(costs != costs, torch.full_like(costs, NAN_COST), costs)
    else:
        cost = torch.where(cost != cost, torch.full_like(cost, NAN_COST), cost)      # per particle, before the mean
        partial = torch.stack([cost[:, o].sum(1) for o in owned], dim=1)
        costs = partial.sum(1) / npart
    return Out(costs.reshape(M, pop), partial, q0, e0)


@functools.lru_cache(maxsize=None)
def reference(name, dtype=torch.float64):
    """restate() of a table case: computed once per dtype, shared, never modified."""
    case = BY_NAME[name]
    obs, acs, noise = inputs(name)
    return restate(weights(case.n_nets), obs, acs, noise, npart_of(case), case.n_nets, case.plan_hor, dtype=dtype)


def fairness(name):
    """What makes a value case a fair test, from the float64 restatement: the spread of the costs (a single candidate: of its
    particles' costs), the smaller head's share of the rows (every step) on which it wins the max, the share of step 0's raw
    log-variances above MAX_LOGVAR and below MIN_LOGVAR, the number of NaN among the results, and the f32 restatement's
    largest deviation from float64 on costs (the cap of rule 1)."""
    case, trace = BY_NAME[name], {}
    obs, acs, noise = inputs(name)
    out = restate(weights(case.n_nets), obs, acs, noise, npart_of(case), case.n_nets, case.plan_hor, trace=trace)
    spread = out.costs if out.costs.numel() > 1 else trace["particle_costs"]
    wins = (trace["heads"][..., 0] > trace["heads"][..., 1]).double().mean()
    lv = trace["logvar0"]
    return dict(std=float(spread.std()), head_share=float(torch.minimum(wins, 1 - wins)),
                above=float((lv > torch.tensor(MAX_LOGVAR)).double().mean()), below=float((lv < torch.tensor(MIN_LOGVAR)).double().mean()),
                nans=sum(int((t != t).sum()) for t in out),
                cap=float((reference(name, torch.float32).costs.double() - out.costs).abs().max()))


def is_fair(f):
    return f["std"] > 0.05 and f["head_share"] >= 0.10 and f["above"] >= 0.05 and f["below"] >= 0.05 and f["nans"] == 0 and f["cap"] <= CAP


# ---- rule 1 -------------------------------------------------------------------------------------------------------------------
def quantities(out):
    """Out -> {quantity: float64 tensor on the host, the group first}."""
    q = dict(costs=out.costs.reshape(-1), partial=out.partial, q0=out.q0, e0_mean=out.e0[..., :2], e0_sd=out.e0[..., 2:])
    return {k: v.detach().double().cpu() for k, v in q.items()}


def f16x3_allowance(quantity, magnitude):
    return dict(costs=F16X3_COSTS, q0=F16X3_COSTS, partial=4 * F16X3_COSTS, e0_mean=F16X3_COSTS * magnitude,
                e0_sd=F16X3_COSTS * magnitude)[quantity]


def basis_of(r64, r32):
    """The bound basis of one quantity: the f32 restatement's largest deviation from float64, at least one ulp of the largest
    float64 magnitude."""
    return max(float((r32.double() - r64).abs().max()), 2.0 ** -23 * float(r64.abs().max()))


def deviation(got, r64):
    dev = (got.double() - r64).abs().max()
    return float("inf") if bool(dev != dev) else float(dev)               # a NaN where float64 has a number


def rule1(got, ref64, ref32, f16x3=False, keep=None, skip=()):
    """{quantity: (deviation, bound, deviation / basis)} of `got` (an Out) against the float64 and f32 restatements; keep: the
    groups (a bool mask) whose costs and partial are compared."""
    g, r64, r32 = quantities(got), quantities(ref64), quantities(ref32)
    res = {}
    for k in QUANTITIES:
        if k in skip:
            continue
        a, b, c = ((t[keep] for t in (g[k], r64[k], r32[k])) if keep is not None and k in ("costs", "partial")
                   else (g[k], r64[k], r32[k]))
        if b.numel() == 0:
            continue
        basis = basis_of(b, c)
        dev = deviation(a, b)
        res[k] = (dev, FACTOR * basis + (f16x3_allowance(k, float(b.abs().max())) if f16x3 else 0.0), dev / basis)
    return res


def broken(res):
    return [k for k, (dev, bound, _) in res.items() if not dev <= bound]


def skipped_quantities(case):
    """plan_hor = 1: the first-step kernel skips the members, nothing writes e0."""
    return ("e0_mean", "e0_sd") if case.plan_hor == 1 else ()


def nan_roundings(n_nets):
    """Roundings between the particle costs and costs[g] where one of them is 1e6: the two shuffle-adds of plan_cost_kernel, the
    member adds of plan_finish_kernel (s = 0 + partial[0] is exact: n_nets - 1) and the division by npart."""
    return 2 + (n_nets - 1) + 1


def nan_bound(ref64, group, n_nets):
    """(bound on partial[group, e] per member, bound on costs[group]): roundings x 2^-24 x the float64 sum of magnitudes."""
    sums = ref64.partial[group].abs().double()
    return 2 * 2.0 ** -24 * sums, nan_roundings(n_nets) * 2.0 ** -24 * float(sums.sum()) / (PPN * n_nets)


def compare(name, got, f16x3=False, report=None):
    """Every way in which `got` (an Out) misses the float64 restatement of table case `name`: the quantities that break rule 1
    and, for a candidate that holds a NaN particle, what exceeds nan_bound().  report: a list that receives
    (quantity, deviation, bound, deviation / basis)."""
    case = BY_NAME[name]
    r64, r32 = reference(name), reference(name, torch.float32)
    holds_nan = (r64.partial >= 0.5 * NAN_COST).any(1)
    res = rule1(got, r64, r32, f16x3, keep=~holds_nan if bool(holds_nan.any()) else None, skip=skipped_quantities(case))
    if report is not None:
        report.extend((k,) + v for k, v in res.items())
    bad = broken(res)
    g = quantities(got)
    for group in holds_nan.nonzero().flatten().tolist():
        pb, cb = nan_bound(r64, group, case.n_nets)
        if not bool(((g["partial"][group] - r64.partial[group]).abs() <= pb).all()):
            bad.append("partial of the NaN candidate %d" % group)
        if not abs(float(g["costs"][group]) - float(r64.costs.reshape(-1)[group])) <= cb:
            bad.append("cost of the NaN candidate %d" % group)
    return bad


# ---- device side (used by the GPU tests only) ---------------------------------------------------------------------------------
def guarded(dev, n):
    """A GUARD-filled f32 buffer of n floats with GUARD_TAIL more behind it -> (whole buffer, the n floats)."""
    flat = torch.full((n + GUARD_TAIL,), GUARD, dtype=torch.float32, device=dev)
    return flat, flat[:n]


def tail_intact(flat, n):
    return bool((flat[n:] == GUARD).all())


class Planner:
    """rrl_plan_pack and rrl_plan_cost through their descriptors, as FusedPlanner.pack and _launch fill them; the caller owns
    `packed`, `scratch` and `costs`."""

    def __init__(self, w, dev):
        from recovery_rl_amd import _lib
        self._lib, self.lib, self.dev = _lib, _lib.load(), dev
        self.n_nets = int(w["e_w0"].shape[0])
        self.npart = PPN * self.n_nets
        self.w = {k: w[k].to(device=dev, dtype=torch.float32).contiguous() for k in WEIGHT_NAMES}
        self.packed_floats = int(self.lib.rrl_plan_pack_floats(HQ, HE, self.n_nets))
        assert self.packed_floats > 0 and self.lib.rrl_plan_supported(HQ, HE, self.n_nets, self.npart, 2, 2)
        self._packed = {}

    def pack(self, f16x3, packed=None):
        """Pack into `packed` (default: a zeroed buffer of its own) -> packed."""
        _lib = self._lib
        if packed is None:
            packed = torch.zeros(self.packed_floats, dtype=torch.float32, device=self.dev)
        desc = _lib.rrl_plan_weights_t(HQ, HE, self.n_nets, *[self.w[k].data_ptr() for k in WEIGHT_NAMES])
        _lib.check(self.lib.rrl_plan_pack(C.byref(desc), int(f16x3), _lib.ptr(packed), _lib.current_stream()), "rrl_plan_pack")
        return packed

    def packed(self, f16x3):
        """The weights packed once per precision from a zeroed buffer."""
        if f16x3 not in self._packed:
            self._packed[f16x3] = self.pack(f16x3)
        return self._packed[f16x3]

    def launch(self, f16x3, M, pop, plan_hor, cur_obs, ac_seqs, scratch, costs, noise=None, m_dev=None, seed=0, counter=0,
               counter_dev=None, counter_inc=1, packed=None, n_nets=None, npart=None):
        """One rrl_plan_cost with every field of rrl_plan_cost_t settable -> the return code."""
        _lib, p = self._lib, self._lib.ptr
        for t in (cur_obs, ac_seqs, noise):
            assert t is None or (t.dtype == torch.float32 and t.is_contiguous() and t.device.type == "cuda")
        a = _lib.rrl_plan_cost_t(p(self.packed(f16x3) if packed is None else packed), HQ, HE,
                                 self.n_nets if n_nets is None else n_nets, self.npart if npart is None else npart, int(f16x3),
                                 M, p(m_dev), pop, plan_hor, p(cur_obs), p(ac_seqs), p(noise), seed, counter, p(counter_dev),
                                 counter_inc, p(scratch), p(costs))
        return self.lib.rrl_plan_cost(C.byref(a), _lib.current_stream())

    def run(self, f16x3, cur_obs, ac_seqs, noise, plan_hor, **kw):
        """A launch into guarded buffers of its own from host or device inputs -> dict(out=Out (device views), costs_flat,
        scratch_flat, groups).  Keyword arguments as launch()'s; M: the launch bound (default: ac_seqs' M)."""
        dev = self.dev
        pop = int(ac_seqs.shape[1])
        M = int(kw.pop("M", ac_seqs.shape[0]))
        groups = M * pop
        put = lambda t: None if t is None else t.to(device=dev, dtype=torch.float32).contiguous()
        cur_obs, ac_seqs, noise = put(cur_obs), put(ac_seqs), put(noise)
        costs_flat, costs = guarded(dev, groups)
        n_scratch = int(self.lib.rrl_plan_scratch_floats(self.n_nets, M, pop))
        assert n_scratch == scratch_floats(self.n_nets, M, pop)
        scratch_flat, scratch = guarded(dev, n_scratch)
        rc = self.launch(f16x3, M, pop, plan_hor, cur_obs, ac_seqs, scratch, costs, noise=noise, **kw)
        assert rc == 0, rc
        torch.cuda.synchronize()
        e0, partial, q0 = split_scratch(scratch, groups, self.n_nets)
        return dict(out=Out(costs.view(M, pop), partial, q0, e0), costs_flat=costs_flat, scratch_flat=scratch_flat, groups=groups,
                    tails=tail_intact(costs_flat, groups) and tail_intact(scratch_flat, n_scratch))


def same_bits(a, b, skip_e0=False):
    """The quantities of two Outs that differ in any bit."""
    return [k for k in Out._fields if not (skip_e0 and k == "e0") and not torch.equal(getattr(a, k), getattr(b, k))]
