"""rrl_cem_sample / rrl_cem_update / rrl_cem_begin / rrl_cem_finish at kernel level, each alone through its descriptor, on every
case of cem_cases.py, bit for bit against the C oracle and the NumPy restatements, with sentinels in and guard elements behind
every output; then the chain as production launches it (begin, five rounds of sample and update with sticky, the device count
and the device tick, finish) followed through the rounds in which problems have gone inactive, and one round captured into a
hipGraph and replayed.  test_cem_paths_cpu.py proves that the tables reach every launch edge and that the oracle is the float64
restatement."""
import numpy as np
import pytest
import torch

import cem_cases as CC
from oracle import c_oracle as co
from recovery_rl_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def same(a, b):
    """Bit for bit, NaN and the sign of zero included."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ---- sample -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c.name for c in CC.SAMPLE_CASES])
def test_sample_case(name):
    c, x = CC.SAMPLE_BY_NAME[name], CC.sample_inputs(name)
    n = CC.live_of(c)
    ref_s, ref_a = CC.sample_oracle(name)
    r = CC.run_sample(name, DEV)
    assert r["tails"], "written behind the end of a buffer"
    for k in ("mean", "var", "lb", "ub"):                                    # the sample step writes none of its inputs
        assert same(r[k], x[k]), k
    assert same(r["active"][:n], ref_a) and same(r["active"][n:], r["active_in"][n:])
    if x["expect_active"] is not None:
        assert r["active"][:n].tolist() == x["expect_active"][:n]
    # an inactive problem's samples are not drawn: the oracle leaves zeros, this buffer its sentinel; so does a row past m_dev
    want = np.full((c.M, c.pop, c.dim), CC.S_SAMPLE, np.float32)
    on = ref_a.astype(bool)
    want[:n][on] = ref_s[on]
    assert same(r["samples"], want)
    assert on.any() or n == 0 or "act" in c.setup
    if c.tick is None:
        assert r["tick"] is None
    else:
        assert r["tick"] == [CC.tick_after(c), 0]                            # the tick advanced, the ticket word is back at 0


# ---- update -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c.name for c in CC.UPDATE_CASES])
def test_update_case(name):
    c, x = CC.UPDATE_BY_NAME[name], CC.update_inputs(name)
    ne, live = CC.num_elites_of(c), c.M + 1
    ref_m, ref_v = (a.copy() for a in CC.update_reference(name))
    ref_m[live:], ref_v[live:] = x["mean"][live:], x["var"][live:]           # problem M + 1: past the count, or not launched
    ora_m, ora_v = co.cem_update(x["samples"][:live], x["costs"][:live], x["mean"][:live], x["var"][:live], ne, c.alpha,
                                 active=x["active"][:live])
    assert same(ora_m, ref_m[:live]) and same(ora_v, ref_v[:live])
    assert same(ref_m[c.M], x["mean"][c.M]) and same(ref_v[c.M], x["var"][c.M])        # the inactive problem
    for device_count in (False, True):
        r = CC.run_update(name, DEV, device_count)
        assert r["tails"] and r["inputs_unchanged"], device_count
        assert np.abs(r["mean"]).max() < 1e3 and np.abs(r["var"]).max() < 1e3, "a padding key was chosen as an elite"
        assert same(r["mean"], ref_m) and same(r["var"], ref_v), device_count


# ---- begin and finish ---------------------------------------------------------------------------------------------------------
BEGIN_OUT = ("count", "idx", "mean", "var", "cur_obs", "active")


@pytest.mark.parametrize("name", [c.name for c in CC.SET_CASES])
def test_begin_case(name):
    c, x, ref = CC.SET_BY_NAME[name], CC.set_inputs(name), CC.set_reference(name)["begin"]
    r = CC.run_begin(name, DEV)
    assert r["tails"], "written behind the end of a buffer"
    count = int(ref["count"][0])
    assert count == int((x["mask"] != 0).sum())
    for k in BEGIN_OUT:                                                      # the whole buffers: rows past count hold their sentinels
        assert same(r[k], ref[k]), k
    assert (r["idx"][count:] == CC.S_IDX).all() and (r["active"][count:] == CC.S_ACTIVE).all()
    for k in ("mask", "prev_sol", "init_var", "obs"):
        assert same(r[k], x[k]), k
    assert (r["action"] == CC.S_ACTION).all()


@pytest.mark.parametrize("name", [c.name for c in CC.SET_CASES])
def test_finish_case(name):
    c, x, ref = CC.SET_BY_NAME[name], CC.set_inputs(name), CC.set_reference(name)
    r = CC.run_finish(name, DEV)
    assert r["tails"], "written behind the end of a buffer"
    assert same(r["action"], ref["action"]) and same(r["prev_sol"], ref["prev_sol"])
    assert not (r["action"] == CC.S_ACTION).any() and np.abs(r["prev_sol"]).max() <= 1.0          # every action written, no POISON read
    if c.mask == "zeros":                                                    # nothing planned: zeros, prev_sol untouched
        assert not r["action"].any() and same(r["prev_sol"], x["prev_sol"])
    assert same(r["idx"], ref["begin"]["idx"]) and same(r["count"], ref["begin"]["count"]) and same(r["mean"], x["mean"])
    assert same(r["mask"], x["mask"])
    assert (r["var"] == CC.S_F64).all() and (r["cur_obs"] == CC.S_OBS).all() and (r["active"] == CC.S_ACTIVE).all()


# ---- the chain as production launches it ----------------------------------------------------------------------------------------
class Chain:
    """The buffers of one planning set of n envs and the two descriptors over them, as MPC._act_device_count and
    CEMOptimizer._describe fill them: the launch bound is n, the count lives on the device, sticky = 1, the host counter is 0,
    the device tick advances by 1."""

    def __init__(self, n, pop, dim, du, num_elites, alpha, t0, mask, seed):
        rng = np.random.RandomState(seed)
        self.n, self.pop, self.dim, self.du, self.ne, self.alpha = n, pop, dim, du, num_elites, alpha
        self.lb, self.ub = -np.ones(dim), np.ones(dim)
        self.host = dict(mask=mask, prev_sol=rng.uniform(-0.5, 0.5, (n, dim)), init_var=np.full(dim, 0.25),
                         obs=rng.randn(n, 2).astype(np.float32))
        B = lambda a, fill: CC.Buf(a, fill, DEV)
        b = {k: B(v, dict(idx=CC.S_IDX, count=CC.S_IDX, mean=CC.S_F64, var=CC.S_F64, cur_obs=CC.S_OBS, active=CC.S_ACTIVE)[k])
             for k, v in CC.begin_buffers(n, dim).items()}
        b.update(mask=B(mask, 0), prev_sol=B(self.host["prev_sol"], CC.S_F64), init_var=B(self.host["init_var"], CC.S_F64),
                 obs=B(self.host["obs"], CC.S_OBS), action=B(np.full((n, du), CC.S_ACTION, np.float32), CC.S_ACTION))
        self.set_bufs = dict(b)
        self.samples = B(np.full((n, pop, dim), CC.S_SAMPLE, np.float32), CC.S_SAMPLE)
        self.costs = B(np.zeros((n, pop), np.float32), np.float32(0))
        self.lb_d, self.ub_d = B(self.lb, CC.S_F64), B(self.ub, CC.S_F64)
        self.tick = torch.tensor([t0, 0], dtype=torch.int64, device=DEV)
        self.b = b
        self.set = CC.describe(_lib.rrl_cem_set_t, n=n, dim=dim, du=du, **b)
        self.cem = CC.describe(_lib.rrl_cem_t, M=n, m_dev=b["count"], pop=pop, dim=dim, mean=b["mean"], var=b["var"], lb=self.lb_d,
                               ub=self.ub_d, epsilon=CC.EPSILON, sticky=1, active=b["active"], seed=CC.SEED, counter=0,
                               counter_dev=self.tick, counter_inc=1, samples=self.samples, num_elites=num_elites, alpha=alpha,
                               costs=self.costs)
        self.lib = _lib.load()

    def call(self, what):
        fn = getattr(self.lib, "rrl_cem_" + what)
        _lib.check(fn(self.set if what in ("begin", "finish") else self.cem, _lib.current_stream()), "rrl_cem_" + what)

    def everything(self):
        """Every buffer, guards included, and the tick, on the host."""
        torch.cuda.synchronize()
        out = {k: v.flat.cpu().numpy() for k, v in self.b.items()}
        out.update(samples=self.samples.flat.cpu().numpy(), costs=self.costs.flat.cpu().numpy(), tick=self.tick.cpu().numpy())
        return out

    def tails(self):
        return all(v.tail_intact() for v in list(self.b.values()) + [self.samples, self.costs, self.lb_d, self.ub_d])


# the compacted problems that start with a variance just above epsilon and a target on their warm start: alpha = 0 leaves the
# elites' variance, about 0.4 of the sampling variance for the 40 nearest of 400 in 10 dimensions, so the first go inactive after
# one update and the others after two
TIGHT = {0: 1.5e-3, 2: 1.5e-3, 5: 4e-3, 7: 4e-3}


@pytest.mark.parametrize("n,kind", CC.CHAIN["cases"])
def test_five_iterations_as_production_launches_them(n, kind):
    P = CC.CHAIN
    pop, dim, du, ne, rounds, t0 = P["pop"], P["dim"], P["du"], P["num_elites"], P["rounds"], P["t0"]
    mask = CC.chain_mask(n, kind)
    ch = Chain(n, pop, dim, du, ne, 0.0, t0, mask, seed=n)
    h = ch.host
    ch.call("begin")
    torch.cuda.synchronize()
    ref = CC.restate_begin(mask, h["prev_sol"], h["init_var"], h["obs"])
    count = int(ref["count"][0])
    assert count > max(TIGHT) and all(same(ch.b[k].host(), ref[k]) for k in BEGIN_OUT)
    if n > CC.K_BEGIN_BLOCK:
        assert 0 < int((mask[:CC.K_BEGIN_BLOCK] != 0).sum()) < count                              # both passes compact rows
    # the planner's inputs of the tight problems, written between begin and the first sample on both sides
    mean_o, var_o, act_o = ref["mean"][:count].copy(), ref["var"][:count].copy(), ref["active"][:count].copy()
    target = np.random.RandomState(n + 1).uniform(-0.5, 0.5, (count, dim))
    for j, v in TIGHT.items():
        var_o[j] = v
        target[j] = mean_o[j]
    ch.b["var"].t[:count] = torch.from_numpy(var_o).to(DEV)
    samples_o = np.full((count, pop, dim), CC.S_SAMPLE, np.float32)
    went = {}
    for r in range(rounds):
        before = (mean_o.copy(), var_o.copy(), samples_o.copy())
        ch.call("sample")
        torch.cuda.synchronize()
        s_new, act_o = co.cem_sample(mean_o, var_o, ch.lb, ch.ub, pop, epsilon=CC.EPSILON, sticky=True, active=act_o, seed=CC.SEED,
                                     counter=t0 + r)
        on = act_o.astype(bool)
        samples_o[on] = s_new[on]
        got_s = ch.samples.host()
        assert same(got_s[:count], samples_o) and (got_s[count:] == CC.S_SAMPLE).all(), r
        assert same(ch.b["active"].host()[:count], act_o) and (ch.b["active"].host()[count:] == CC.S_ACTIVE).all(), r
        assert ch.tick.tolist() == [t0 + r + 1, 0]
        for j in np.flatnonzero(~on):
            went.setdefault(int(j), r)
        # the costs once, on the host, from the samples both sides hold: the kernel and the oracle sort identical costs
        costs = CC.quadratic_costs(got_s[:count], target)
        ch.costs.t[:count] = torch.from_numpy(costs).to(DEV)
        ch.call("update")
        torch.cuda.synchronize()
        mean_o, var_o = co.cem_update(samples_o, costs, mean_o, var_o, ne, 0.0, active=act_o)
        got_m, got_v = ch.b["mean"].host(), ch.b["var"].host()
        assert same(got_m[:count], mean_o) and same(got_v[:count], var_o), r
        assert (got_m[count:] == CC.S_F64).all() and (got_v[count:] == CC.S_F64).all(), r
        # a problem that has gone inactive stays frozen: mean, variance and samples, on the device as in the oracle
        for a, b in zip((got_m[:count], got_v[:count], got_s[:count]), before):
            assert same(a[~on], b[~on]), r
        assert same(mean_o[~on], before[0][~on]) and same(var_o[~on], before[1][~on])
    # not vacuous: the tight problems went inactive in the oracle, the early ones before the second update, the others before the
    # third, stayed inactive (sticky), and other problems were still being planned in the last round
    assert {j: went.get(j) for j in TIGHT} == {0: 1, 2: 1, 5: 2, 7: 2}, went
    assert not act_o[list(TIGHT)].any() and act_o.sum() > count // 2
    assert ch.tick.tolist() == [t0 + rounds, 0]
    ch.call("finish")
    torch.cuda.synchronize()
    mean_full = ch.b["mean"].host()
    assert same(mean_full[:count], mean_o)
    action, prev_sol = CC.restate_finish(mask, ref["idx"], count, mean_full, h["prev_sol"], np.full((n, du), CC.S_ACTION, np.float32), du)
    assert same(ch.b["action"].host(), action) and same(ch.b["prev_sol"].host(), prev_sol)
    assert not (action == CC.S_ACTION).any() and ch.tails()


# ---- one round captured into a graph ----------------------------------------------------------------------------------------
def test_captured_round_replays_as_eager():
    """begin, sample, update and finish on one stream in one graph (no parallel branches), the costs fixed, the device tick used:
    two replays from tick t0 leave what two eager rounds leave -- the second round starts from the warm starts the first one
    shifted and draws at tick t0 + 1."""
    P = CC.CAPTURE
    n, t0 = P["n"], P["t0"]
    mask = CC.chain_mask(n, "spread")
    costs = np.random.RandomState(3).randn(n, P["pop"]).astype(np.float32)

    def fresh():
        ch = Chain(n, P["pop"], P["dim"], P["du"], P["num_elites"], P["alpha"], t0, mask, seed=77)
        ch.costs.t[:] = torch.from_numpy(costs).to(DEV)
        return ch

    def one_round(ch):
        for what in ("begin", "sample", "update", "finish"):
            ch.call(what)

    eager, want = fresh(), []
    for _ in range(P["replays"]):
        one_round(eager)
        want.append(eager.everything())
    assert want[-1]["tick"].tolist() == [t0 + P["replays"], 0]
    assert not same(want[0]["samples"], want[1]["samples"]) and not same(want[0]["prev_sol"], want[1]["prev_sol"])
    count = int(want[0]["count"][0])
    assert count == int(mask.sum()) and (want[0]["active"][:count] == 1).all()
    ch = fresh()
    start = ch.everything()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        one_round(ch)
    assert all(same(v, start[k]) for k, v in ch.everything().items())        # the capture executed nothing
    for turn in range(P["replays"]):
        g.replay()
        got = ch.everything()
        assert sorted(got) == sorted(want[turn])
        for k, v in got.items():
            assert same(v, want[turn][k]), (turn, k)
    assert ch.tick.tolist() == [t0 + P["replays"], 0] and ch.tails() and eager.tails()
