"""The conditions under which test_step_push_gpu.py means something, checked on the host: the composite reference of
step_push_cases.py run alone for K steps per case.  The table covers what its comment says; no gate decision is near its
threshold; every event the kernel branches on occurs; every ring wraps where the table says; the small episode table
overflows; the vectorised episode log equals log_oracle.EpisodeLogOracle; and with every option off the composite reference
reproduces what test_nav_gpu.py::test_fused_step_push_matches_oracle_step_plus_pushes computes inline."""
import functools

import numpy as np
import pytest

import step_push_cases as SP
from oracle import c_oracle as co
from oracle.log_oracle import EpisodeLogOracle

CASES = {c.name: c for c in SP.CASES}
ALL = SP.CASES + [s for cls in ("nav", "maze") for r in (0, 1) for s in SP.packed_seeds(cls, r)]


@functools.lru_cache(maxsize=None)
def _run(name):
    c = {c.name: c for c in ALL}[name]
    return SP.run_reference(c, SP.K)


def _options(c):
    """The (option, value) pairs the table's comment promises in every regime and with both env classes."""
    o = {("layout", c.layout), ("gate", c.gate), ("ld_task", c.ld_task), ("push_real_action", c.push_real_action),
         ("recovery_memory", c.rmem is not None), ("pinned", bool(c.mem[1] or (c.rmem and c.rmem[1]))),
         ("outputs", c.outputs), ("log", c.log), ("auto_reset", c.auto_reset), ("tick", c.tick),
         ("reward_penalty", c.reward_penalty)}
    if c.gate != "off":
        o |= {("sel_n_part", c.sel_n_part), ("eps_safe", c.eps_safe)}
    if c.gate == "head":
        o |= {("head_n_part", c.head_n_part), ("head_eps", c.head_eps), ("log_std", c.log_std)}
    return o


PROMISED = {("layout", "arrays"), ("layout", "status"), ("gate", "off"), ("gate", "action"), ("gate", "head"),
            ("sel_n_part", 1), ("sel_n_part", 3), ("sel_n_part", 4), ("head_n_part", 1), ("head_n_part", 4),
            ("head_eps", True), ("head_eps", False), ("log_std", "above"), ("log_std", "mixed"), ("ld_task", 2),
            ("ld_task", 4), ("push_real_action", 0), ("push_real_action", 1), ("recovery_memory", True),
            ("recovery_memory", False), ("pinned", True), ("pinned", False), ("outputs", "all"), ("outputs", "none"),
            ("outputs", "two"), ("log", "off"), ("log", "on"), ("log", "small"), ("auto_reset", 0), ("auto_reset", 1),
            ("tick", "dev"), ("tick", "host"), ("reward_penalty", 0.0), ("reward_penalty", 2.5), ("eps_safe", 0.3),
            ("eps_safe", 0.65)}


def test_the_table_covers_every_option_in_every_regime_and_env_class():
    assert 20 <= len(SP.CASES) <= 28
    for regime in (0, 1, 2):
        seen = set().union(*(_options(c) for c in SP.CASES if SP.regime_of(c.n) == regime))
        assert PROMISED <= seen, (regime, sorted(PROMISED - seen, key=str))
    for maze in (False, True):
        seen = set().union(*(_options(c) for c in SP.CASES if SP.is_maze(c) == maze))
        assert PROMISED <= seen, ("maze" if maze else "nav", sorted(PROMISED - seen, key=str))
    ns = {c.n for c in SP.CASES}
    assert {1, 63, 257, 16384, 16385} <= ns and ns & {262144, 262145}
    assert sum(c.n > SP.MID for c in SP.CASES) <= 4
    assert {c.env for c in SP.CASES} == {"navigation1", "navigation2", "maze"}
    assert any(c.sel_n_part == 2 for c in SP.CASES) and any(c.head_n_part == 2 for c in SP.CASES)
    assert any(c.horizon == 4095 and c.layout == "status" for c in SP.CASES)
    for regime in (0, 1, 2):            # everything on at once, with a pinned ring that wraps
        assert any(SP.regime_of(c.n) == regime and c.layout == "status" and c.gate == "head" and c.sel_n_part == 3 and
                   c.head_n_part == 4 and c.ld_task == 4 and c.push_real_action == 1 and c.log == "on" and c.rmem and
                   c.rmem[1] > 0 for c in SP.CASES)
    for regime in (1, 2):               # both branches of block_sums
        rings = [c.rmem for c in SP.CASES if SP.regime_of(c.n) == regime and c.rmem]
        assert any(cap % 1024 and pinned % 1024 for cap, pinned in rings)
        # ... and in one of them the workgroup that straddles the wrap (step 3, cursor at pinned + 2 n) starts before the
        # last super-chunk: it touches three super-chunks, which two workgroup sums cannot hold
        block = 256 if regime == 1 else 1024
        assert any(c.rmem[1] % 1024 and 2 * c.n < c.rmem[0] - c.rmem[1] < 3 * c.n and
                   (c.rmem[0] - c.rmem[1] - 2 * c.n) % block > c.rmem[0] % 1024 > 0
                   for c in SP.CASES if SP.regime_of(c.n) == regime and c.rmem)
        assert any(cap % 1024 == 0 and pinned % 1024 == 0 and pinned for cap, pinned in rings)
    for c in ALL:
        for ring in (c.mem, c.rmem):
            assert ring is None or c.n <= ring[0] - ring[1]
        assert c.eps_safe in (0.3, 0.65) and c.log_std in ("above", "mixed")


@pytest.mark.parametrize("name", [c.name for c in ALL])
def test_the_reference_run_exercises_what_the_case_is_for(name):
    c = {c.name: c for c in ALL}[name]
    ref, outs, inps = _run(name)
    n, ev = c.n, ref["events"]
    # no gate decision within NEAR of the threshold (the kernel's f32 sigmoid is ~1e-7 off: the flag is then decided)
    for o in outs:
        if c.gate != "off":
            assert np.abs(o["risk"] - float(np.float32(c.eps_safe))).min() >= SP.NEAR
    if c.gate != "off":
        for inp in inps:                # the partials are real partials: no single one is the sum
            assert c.sel_n_part == 1 or not np.array_equal(inp["z_parts"][0], SP.summed(inp["z_parts"]))
        if n >= 257:
            assert 0.1 * SP.K * n <= ev["flag"] <= 0.9 * SP.K * n, ev["flag"] / (SP.K * n)
    if n >= 16384 and c.gate != "off" and c.sel_n_part >= 3:
        # the order of the partial sums shows: added last to first, some row's flag comes out the other way
        for inp, o in zip(inps, outs):
            back = SP.risk64(inp["z_parts"][::-1]) > float(np.float32(c.eps_safe))
            assert (back != (o["flag"] != 0)).sum() >= 3
    if n >= 16384 and c.gate == "head" and c.head_n_part >= 3:
        for inp, o in zip(inps, outs):      # ... and some chosen recovery action moves by more than 0.1
            moved = np.abs(SP.summed(inp["head_parts"][::-1]) - SP.summed(inp["head_parts"])).max(1) > 0.1
            assert (moved & (o["flag"] != 0)).sum() >= 3
    if n >= 257:
        for what in ("constraint", "done", "horizon"):
            assert ev[what] > 0, what
        assert ev["reset"] > 0 or not c.auto_reset
        assert ev["success"] > 0 or SP.is_maze(c)
        assert ref["positives_overwritten"] > 0 or c.rmem is None
        assert all(o["at_horizon"].any() for o in outs)      # the horizon is reached in each of the K steps
    if c.horizon == 4095:
        assert any(((o["ep_done"] != 0) & (o["done"] == 0)).any() for o in outs)     # t = 4094 -> 4095 = horizon
    # every ring wraps in step 2 or 3
    for key, ring in (("mem", c.mem), ("rmem", c.rmem)):
        if ring is not None:
            assert ref["wraps"][key] and ref["wraps"][key][0] in (2, 3), (key, ref["wraps"][key])
            assert ref[key].pos >= ring[1] and ref[key].size == ring[0]
    if c.name in ("r1_all_on", "r2_all_on"):
        # the workgroup that straddles the safety ring's wrap holds positives in the LAST super-chunk as well as in the one
        # before it (rows of step 3, not overwritten by step 4): two workgroup sums cannot stand for its three super-chunks
        cap, block = c.rmem[0], 256 if SP.regime_of(n) == 1 else 1024
        start = cap - (cap - c.rmem[1] - 2 * n) % block
        last = cap - cap % 1024
        assert start < last and (ref["rmem"].r[start:last] != 0).sum() >= 2 and (ref["rmem"].r[last:cap] != 0).sum() >= 2
    if c.log != "off":
        log = ref["log"]
        assert sum(log.per_step[:-1]) > 0 or n == 1          # an episode ends in a step other than the last
        if c.log == "small":
            assert len(log.rec_i32) > SP.log_cap(c)           # the small table really overflows
        else:
            assert len(log.rec_i32) <= SP.log_cap(c)


@pytest.mark.parametrize("name", [c.name for c in ALL if c.log != "off" and c.n <= 257])
def test_the_vectorised_log_equals_the_episode_log_oracle(name):
    c = {c.name: c for c in ALL}[name]
    ref, outs, _ = _run(name)
    init = SP.initial_state(c)
    ora = EpisodeLogOracle(c.n)
    ora.len[:], ora.ret[:], ora.viol[:], ora.rec[:] = init["log_len"], init["log_ret"], init["log_viol"], init["log_rec"]
    ora.iteration = SP.LOG_ITER0
    for o in outs:
        ora.append(o["reward"], o["constraint"], o["success"], o["ep_done"], o["flag"])
    log = ref["log"]
    assert ora.records == log.records() and ora.iteration == log.iteration
    for a, b in ((ora.len, log.len), (ora.ret, log.ret), (ora.viol, log.viol), (ora.rec, log.rec)):
        assert np.array_equal(a, b)


def test_the_vectorised_log_without_recovery_flags():
    rng = np.random.RandomState(0)
    ora, vec = EpisodeLogOracle(100), SP.VecLog(100)
    for _ in range(6):
        rew, flags = rng.randn(100).astype(np.float32), rng.randint(0, 2, (3, 100)).astype(np.uint8)
        ora.append(rew, *flags)
        vec.append(rew, *flags)
    assert ora.records == vec.records() and len(ora.records) > 50


def test_with_every_option_off_the_reference_is_the_inline_computation_of_test_nav_gpu():
    """test_nav_gpu.py::test_fused_step_push_matches_oracle_step_plus_pushes, its host side restated line by line on the
    inputs of the PLAIN case, against reference_step."""
    c = SP.PLAIN
    n, cap = c.n, c.mem[0]
    init = SP.initial_state(c)
    ref = SP.reference_state(c, init)
    for ring in (ref["mem"], ref["rmem"]):
        for arr in (ring.s, ring.a, ring.r, ring.s2, ring.m):
            arr[...] = 0
    omem, ormem = co.OracleReplay(cap), co.OracleReplay(cap)
    pos, t, obs = init["pos"].copy(), init["t"].copy(), init["obs"].copy()
    ref_stats = np.zeros(8, np.int64)
    ref_ep, ref_sums = init["ep_reward"].copy(), np.zeros(2)
    tick = SP.TICK0
    for k in range(5):
        inp = SP.make_inputs(c, k)
        out = SP.reference_step(c, ref, inp)
        task, real, r = inp["task"], inp["real"], inp["recovery"].astype(bool)
        o = co.nav_step(c.env, pos, real, t, seed=c.seed, counter=SP.BASE_COUNTER + tick, horizon=100, auto_reset=True)
        tick += SP.TICK_INC
        for key in ("next_obs", "reward", "done", "constraint", "success", "ep_done"):
            assert np.array_equal(out[key], o[key]), key
        mask = 1.0 - o["done"].astype(np.float32)
        cons = o["constraint"].astype(np.float32)
        omem.push(obs, task, o["reward"] - 2.5 * cons, o["next_obs"], mask)
        ormem.push(obs, real, cons, o["next_obs"], mask)
        pos, t, obs = o["pos"], o["t"], o["obs"]
        epd, cc, s_ = o["ep_done"].astype(bool), o["constraint"].astype(bool), o["success"].astype(bool)
        ref_stats += [n, epd.sum(), (epd & cc).sum(), (epd & cc & r).sum(), (epd & cc & ~r).sum(), (epd & s_).sum(), r.sum(),
                      cc.sum()]
        ref_ep += o["reward"]
        ref_sums += [o["reward"].astype(np.float64).sum(), ref_ep[epd].astype(np.float64).sum()]
        ref_ep[epd] = 0
    assert omem.size == cap and ref_stats[1] > 0 and ref_stats[7] > 0
    for got, want in ((ref["mem"], omem), (ref["rmem"], ormem)):
        assert got.pos == want.pos and got.size == want.size
        for a, b in ((got.s, want.s), (got.a, want.a), (got.r, want.r), (got.s2, want.s2), (got.m, want.m)):
            assert np.array_equal(a, b)
    assert np.array_equal(ref["stats"] - SP.STATS0, ref_stats)
    assert np.array_equal(ref["pos"], pos) and np.array_equal(ref["t"], t) and np.array_equal(ref["obs"], obs)
    assert np.array_equal(ref["ep_reward"], ref_ep)
    (s0, b0), (s1, b1) = SP.reward_sums(ref)
    assert abs(s0 - ref_sums[0]) <= b0 and abs(s1 - ref_sums[1]) <= b1
    assert ref["tick"] == tick


def test_count_tables_restate_the_layout_of_the_header():
    """count_tables() against the three regions as test_replay_gpu.assert_count_tables reads them."""
    rng = np.random.RandomState(1)
    for cap, size in ((100, 70), (1024, 1024), (5000, 4999), (100424, 3)):
        r = (rng.uniform(size=cap) < 0.3).astype(np.float32)
        got = SP.count_tables(r, size, cap)
        n_chunks, n_super = (cap + 63) // 64, (cap + 1023) // 1024
        base = (n_chunks + 3) // 4 * 4
        mbase = (base + n_super + 1) // 2 * 2
        want = np.zeros(n_chunks * 64, bool)
        want[:size] = r[:size] != 0
        assert len(got) == mbase + 2 * n_chunks == SP.count_table_len(cap)
        assert np.array_equal(got[:n_chunks], want.reshape(-1, 64).sum(1))
        first = np.r_[got[:n_chunks], np.zeros((-n_chunks) % 16, np.int32)]
        assert np.array_equal(got[base:base + n_super], first.reshape(-1, 16).sum(1))
        assert np.array_equal(got[mbase:].view(np.uint64),
                              np.packbits(want.reshape(-1, 64), axis=1, bitorder="little").view(np.uint64).ravel())
