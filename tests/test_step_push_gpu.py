"""The fused env step (rrl_nav_step_push_x / rrl_maze_step_push_x and their packed forms) against the composite host reference
of step_push_cases.py, on every option the lock-step driver switches on and in all three launch shapes.

Each test fills an rrl_step_push_t by hand over raw tensors.  Every device buffer is PAD rows longer than it has to be and
those rows hold a sentinel.  After each of the K steps every buffer -- inputs, outputs, env state, both rings over their whole
capacity, cursors, count tables, counters, accumulators, the episode table -- is compared bit for bit (np.array_equal) with
what the reference says it holds, sentinel rows included; what the kernel may not touch is thereby checked with the rest.
Exceptions, each with its own rule: the two f64 reward sums (atomics in arrival order: the derived bound of
step_push_cases.reward_sums), the order of the episode records (sorted), and which records an overflowing table keeps.
The recovery action of gate = "head" cases is the output of a stand-alone rrl_policy_heads_fwd_multi launch on the same
partials (the header promises the same bits) and is compared with update_oracle.stoch_head under the pooled rule of
test_update_pieces_gpu.py."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

import step_push_cases as SP
import update_pieces as UP
from oracle import c_oracle as co
from oracle import update_oracle as O
from recovery_rl_amd import _lib
from test_replay_gpu import assert_count_tables
from test_update_pieces_gpu import Pool

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PAD = 5
SENT = {np.dtype(np.float32): -7.0, np.dtype(np.float64): -7.0, np.dtype(np.int32): -77, np.dtype(np.int64): -77,
        np.dtype(np.uint8): 0xAB, np.dtype(np.int16): -0x5433}
EINVAL = -1
p = _lib.ptr


def padded(arr, pad=PAD):
    """`arr` with `pad` sentinel rows behind it."""
    arr = np.ascontiguousarray(arr)
    tail = np.full((pad,) + arr.shape[1:], SENT[arr.dtype], arr.dtype)
    return np.concatenate([arr, tail])


class Run:
    """The device state of one case (or of one seed of a packed launch) next to its reference state."""

    def __init__(self, c, inputs=None):
        self.c, n = c, c.n
        self.inputs = inputs if inputs is not None else [None] * SP.K
        init = SP.initial_state(c)
        self.ref = SP.reference_state(c, init)
        self.pinned_rows = init["rmem_rows"]
        self.buf, self.want, self.keep, self.pool = {}, {}, [], Pool()
        self.sums = torch.zeros(2 + 2, dtype=torch.float64, device=DEV)
        new = self.new
        new("pos", init["pos"])
        if c.layout == "status":
            new("status", self.ref["status"].view(np.int16))
        else:
            new("t", init["t"])
        new("obs", init["obs"])
        new("ep_reward", init["ep_reward"])
        new("stats", SP.STATS0, pad=2)
        if c.tick == "dev":
            new("tick", np.array([SP.TICK0], np.int64), pad=1)
        wanted = dict(all=("next_obs", "reward", "done", "constraint", "success", "ep_done"), none=(),
                      two=("reward", "ep_done"))[c.outputs]
        for key in wanted:
            dt = np.float32 if key in ("next_obs", "reward") else np.uint8
            new(key, np.full((n, 2) if key == "next_obs" else (n,), SENT[np.dtype(dt)], dt))
        if c.gate != "off":
            new("real_out", np.full((n, 2), -7.0, np.float32))
            new("recovery_out", np.full(n, 0xAB, np.uint8))
            scale, bias, log_std, _ = SP.head_consts(c)
            new("scale", scale, pad=1), new("bias", bias, pad=1), new("log_std", log_std, pad=1)
        if c.log != "off":
            for key in ("log_len", "log_ret", "log_viol", "log_rec"):
                new(key, init[key])
            self.log_cap = SP.log_cap(c)
            new("log_state", np.array([0, SP.LOG_ITER0, 0], np.int64), pad=1)
            self.rec_i32 = torch.full((self.log_cap + PAD, 6), -77, dtype=torch.int32, device=DEV)
            self.rec_f64 = torch.full((self.log_cap + PAD, 2), -7.0, dtype=torch.float64, device=DEV)
        self.rings = {}
        for key, spec in (("mem", c.mem), ("rmem", c.rmem)):
            if spec is None:
                continue
            cap, pinned = spec
            ora = self.ref[key]
            for f in "s a r s2 m".split():
                new(key + "." + f, getattr(ora, f))
            new(key + ".state", np.array([pinned, pinned, 0, 0], np.int64), pad=1)
            cnt = None
            if key == "rmem":
                cnt = new(key + ".pos_cnt", SP.count_tables(ora.r, pinned, cap), pad=2)
            b = self.buf
            self.rings[key] = _lib.rrl_replay_t(p(b[key + ".s"]), p(b[key + ".a"]), p(b[key + ".r"]), p(b[key + ".s2"]),
                                                p(b[key + ".m"]), cap, p(b[key + ".state"]), p(cnt), 0, pinned)
        self.head = None

    def new(self, name, arr, pad=PAD):
        full = padded(arr, pad)
        self.want[name] = full
        self.buf[name] = torch.from_numpy(full.copy()).to(DEV)
        return self.buf[name]

    def expect(self, name, arr):
        arr = np.asarray(arr)
        assert arr.dtype == self.want[name].dtype, (name, arr.dtype)
        self.want[name][:len(arr)] = arr

    # -- one step -----------------------------------------------------------------------------------------------------------
    def args(self, k):
        """Upload the inputs of step k and fill the rrl_step_push_t."""
        c, n, b, new = self.c, self.c.n, self.buf, self.new
        if self.inputs[k] is None:
            self.inputs[k] = SP.make_inputs(c, k)
        inp = self.inp = dict(self.inputs[k])
        for name in ("task", "real", "recovery", "z", "rec", "head", "head_eps"):       # the previous step's inputs
            self.buf.pop(name, None), self.want.pop(name, None)
        a = _lib.rrl_step_push_t()
        a.n, a.pos, a.obs = n, p(b["pos"]), p(b["obs"])
        a.t, a.status = p(b.get("t")), p(b.get("status"))
        task = new("task", inp["task4"] if c.ld_task == 4 else inp["task"])
        a.task_action, a.ld_task = task.data_ptr() + (8 if c.ld_task == 4 else 0), c.ld_task
        a.real_action, a.recovery = p(new("real", inp["real"])), p(new("recovery", inp["recovery"]))
        if c.gate != "off":
            np_, ps = c.sel_n_part, 2 * n + 11
            z = np.full((np_ - 1) * ps + 2 * n + PAD, -7.0, np.float32)
            for j in range(np_):
                z[j * ps:j * ps + 2 * n] = inp["z_parts"][j].reshape(-1)
            a.sel_z, a.sel_n_part, a.sel_part_stride = p(new("z", z, pad=0)), np_, ps
            a.sel_eps_safe = c.eps_safe
            a.real_action_out, a.recovery_out = p(b["real_out"]), p(b["recovery_out"])
            if c.gate == "action":
                a.sel_rec_action = p(new("rec", inp["rec"]))
            else:
                hn, hs = c.head_n_part, 2 * n + 7
                h = np.full((hn - 1) * hs + 2 * n + PAD, -7.0, np.float32)
                for j in range(hn):
                    h[j * hs:j * hs + 2 * n] = inp["head_parts"][j].reshape(-1)
                head = new("head", h, pad=0)
                eps = new("head_eps", inp["head_eps"])
                self.head = _lib.rrl_policy_head_t(_lib.HEAD_STOCH, n, p(head), hn, hs, p(eps) if c.head_eps else None,
                                                   p(b["scale"]), p(b["bias"]), None, 2, None, None, None, None,
                                                   p(b["log_std"]), UP.MIN_LOG_STD)
                a.sel_rec_head = C.pointer(self.head)
        a.seed = c.seed
        if c.tick == "dev":
            a.counter, a.counter_dev, a.counter_inc = SP.BASE_COUNTER, p(b["tick"]), SP.TICK_INC
        else:
            a.counter = SP.BASE_COUNTER + 3 * k
        a.horizon, a.auto_reset, a.reward_penalty, a.push_real_action = c.horizon, c.auto_reset, c.reward_penalty, c.push_real_action
        a.memory = C.pointer(self.rings["mem"])
        if c.rmem:
            a.recovery_memory = C.pointer(self.rings["rmem"])
        for key in ("next_obs", "reward", "done", "constraint", "success", "ep_done"):
            setattr(a, key, p(b.get(key)))
        a.stats, a.reward_sums, a.ep_reward = p(b["stats"]), p(self.sums), p(b["ep_reward"])
        if c.log != "off":
            a.log_rec_i32, a.log_rec_f64, a.log_cap, a.log_state = p(self.rec_i32), p(self.rec_f64), self.log_cap, p(b["log_state"])
            a.log_len, a.log_ret, a.log_viol, a.log_rec = p(b["log_len"]), p(b["log_ret"]), p(b["log_viol"]), p(b["log_rec"])
        self.keep = [a]
        return a

    def launch(self, k):
        lib, a = _lib.load(), self.args(k)
        if SP.is_maze(self.c):
            rc = lib.rrl_maze_step_push_x(C.byref(a), _lib.current_stream())
        else:
            rc = lib.rrl_nav_step_push_x(co.ENV_KIND[self.c.env], C.byref(a), _lib.current_stream())
        assert rc == 0, rc
        torch.cuda.synchronize()

    def stand_alone_gate(self):
        """The recovery action (given, or from a stand-alone head launch on the same partials) and what a stand-alone
        rrl_recovery_select launch writes for the same inputs -> (rec, real, flag) device tensors [n + PAD, ...]."""
        c, n, b, lib = self.c, self.c.n, self.buf, _lib.load()
        if c.gate == "head":
            rec = torch.full((n + PAD, 2), -7.0, device=DEV)
            d = _lib.rrl_policy_head_t.from_buffer_copy(self.head)
            d.action = p(rec)
            _lib.check(lib.rrl_policy_heads_fwd_multi(1, C.byref(d), _lib.current_stream()), "rrl_policy_heads_fwd_multi")
        else:
            rec = b["rec"]
        ps = 2 * n + 11
        parts = torch.stack([b["z"][j * ps:j * ps + 2 * n] for j in range(c.sel_n_part)])
        z = O.fixed_order_sum(parts).contiguous()
        real = torch.full((n + PAD, 2), -7.0, device=DEV)
        flag = torch.full((n + PAD,), 0xAB, dtype=torch.uint8, device=DEV)
        task_out = torch.full((n + PAD, 2), -7.0, device=DEV)
        task_ptr = b["task"].data_ptr() + (8 if c.ld_task == 4 else 0)
        _lib.check(lib.rrl_recovery_select(n, p(z), c.eps_safe, task_ptr, c.ld_task, p(rec), p(real), p(flag), p(task_out),
                                           _lib.current_stream()), "rrl_recovery_select")
        torch.cuda.synchronize()
        return rec, real, flag

    def check(self, k):
        """Advance the reference by the step just launched and compare everything."""
        c, n, b, ref, inp = self.c, self.c.n, self.buf, self.ref, self.inp
        if c.gate != "off":
            rec, real, flag = self.stand_alone_gate()
            # the executed action and the flag: what the stand-alone launches leave, bit for bit
            assert torch.equal(b["recovery_out"], flag), "recovery_out differs from rrl_recovery_select"
            task = b["task"][:n, 2:4] if c.ld_task == 4 else b["task"][:n]
            assert torch.equal(b["real_out"][:n], torch.where(flag[:n].bool().unsqueeze(1), rec[:n], task))
            assert torch.equal(b["real_out"], real)
            if c.gate == "head":
                hs = 2 * n + 7
                raw = O.fixed_order_sum(torch.stack([b["head"][j * hs:j * hs + 2 * n].view(n, 2)
                                                     for j in range(c.head_n_part)])).contiguous()
                mod, _ = UP.module_stoch(raw, b["head_eps"][:n].contiguous() if c.head_eps else None, b["log_std"][:2])
                sel = flag[:n].bool().cpu()         # the fused kernel's own head output shows where the gate chose it
                want = SP.head_action64(c, inp)
                if bool(sel.any()):
                    self.pool.add("fused step stoch action", b["real_out"][:n].cpu()[sel], mod.cpu()[sel], want[sel],
                                  "%s step %d" % (c.name, k + 1))
                inp["rec"] = rec[:n].cpu().numpy()
        out = SP.reference_step(c, ref, inp)
        ex = self.expect
        ex("pos", ref["pos"]), ex("obs", ref["obs"]), ex("ep_reward", ref["ep_reward"]), ex("stats", ref["stats"])
        if c.layout == "status":
            ex("status", ref["status"].view(np.int16))
        else:
            ex("t", ref["t"])
        if c.tick == "dev":
            ex("tick", np.array([ref["tick"]], np.int64))
        for key in ("next_obs", "reward", "done", "constraint", "success", "ep_done"):
            if key in b:
                ex(key, out[key])
        if c.gate != "off":
            ex("real_out", out["act"]), ex("recovery_out", out["flag"])
        for key, ring in self.rings.items():
            ora = ref[key]
            for f in "s a r s2 m".split():
                ex(key + "." + f, getattr(ora, f))
            ex(key + ".state", np.array([ora.pos, ora.size, 0, 0], np.int64))
        if c.log != "off":
            log = ref["log"]
            ex("log_len", log.len), ex("log_ret", log.ret), ex("log_viol", log.viol), ex("log_rec", log.rec)
            ex("log_state", np.array([len(log.rec_i32), log.iteration, 0], np.int64))
        for name, t in b.items():
            if name.endswith(".pos_cnt"):
                continue
            got, want = t.cpu().numpy(), self.want[name]
            assert np.array_equal(got, want), "%s, step %d: %s differs in %d elements" % (
                c.name, k + 1, name, int((got != want).sum()))
        if c.rmem:
            cap, pinned = c.rmem
            cnt = b["rmem.pos_cnt"]
            assert_count_tables(types.SimpleNamespace(pos_cnt=cnt[:SP.count_table_len(cap)]), ref["rmem"], cap)
            assert bool((cnt[SP.count_table_len(cap):] == -77).all())
            for f, rows in zip("s a r s2 m".split(), self.pinned_rows if pinned else ()):
                assert np.array_equal(b["rmem." + f][:pinned].cpu().numpy(), rows)       # the pinned rows are still there
        if c.log != "off":
            self.check_records()
        got = self.sums.cpu().numpy()
        assert got[2] == 0 and got[3] == 0
        for j, (exact, bound) in enumerate(SP.reward_sums(ref)):
            print("%s step %d: reward_sums[%d] = %.17g, exact %.17g, off by %.3e (bound %.3e)"
                  % (c.name, k + 1, j, got[j], exact, abs(got[j] - exact), bound))
            assert abs(got[j] - exact) <= bound, (c.name, k + 1, j, got[j], exact, bound)

    def check_records(self):
        """The episode table: every written record is one of the reference's, none twice; without overflow all of them are
        there (= equal after sorting by (iteration, env)); with overflow exactly log_cap slots hold records; behind the
        written slots the table holds its sentinel."""
        log, cap = self.ref["log"], self.log_cap
        i32, f64 = self.rec_i32.cpu().numpy(), self.rec_f64.cpu().numpy()
        total = len(log.rec_i32)
        written = min(total, cap)
        assert (i32[written:] == -77).all() and (f64[written:] == -7.0).all()
        key = lambda r: r[:, 1].astype(np.int64) * (1 << 32) + r[:, 0]
        ref_key = key(log.rec_i32)
        order = np.argsort(ref_key, kind="stable")
        got_key = key(i32[:written])
        assert len(np.unique(got_key)) == written
        at = np.searchsorted(ref_key[order], got_key)
        assert (at < total).all() and np.array_equal(ref_key[order][at], got_key)
        assert np.array_equal(i32[:written], log.rec_i32[order][at]) and np.array_equal(f64[:written], log.rec_f64[order][at])

    def snapshot(self):
        """Every buffer's bits, the episode records in (iteration, env) order; without the reward sums, and without the
        records of a table that overflowed (which episodes it keeps depends on the arrival order)."""
        snap = {name: t.cpu().numpy() for name, t in self.buf.items()}
        if self.c.log == "on":
            i32, f64 = self.rec_i32.cpu().numpy(), self.rec_f64.cpu().numpy()
            count = int(snap["log_state"][0])
            order = np.lexsort((i32[:count, 0], i32[:count, 1]))
            snap["rec_i32"] = np.concatenate([i32[:count][order], i32[count:]])
            snap["rec_f64"] = np.concatenate([f64[:count][order], f64[count:]])
        return snap


def assert_same_bits(a, b, what):
    assert a.keys() == b.keys()
    for name in a:
        assert a[name].dtype == b[name].dtype and np.array_equal(a[name], b[name]), (what, name)


@pytest.mark.parametrize("name", [c.name for c in SP.CASES])
def test_fused_step_equals_the_composite_reference(name):
    c = {c.name: c for c in SP.CASES}[name]
    run = Run(c)
    for k in range(SP.K):
        run.launch(k)
        run.check(k)
    if c.gate == "head":
        run.pool.check()
    # the same case again from the same initial state: identical bits everywhere (the reward sums aside)
    again = Run(c, run.inputs)
    for k in range(SP.K):
        again.launch(k)
    assert_same_bits(run.snapshot(), again.snapshot(), "second run")
    for j, (exact, bound) in enumerate(SP.reward_sums(run.ref)):
        assert abs(float(again.sums[j]) - exact) <= bound


def packed_launch(runs, k, env_class):
    lib = _lib.load()
    arr = (_lib.rrl_step_push_t * len(runs))(*[r.args(k) for r in runs])
    if env_class == "maze":
        rc = lib.rrl_maze_step_push_packed(len(runs), arr, _lib.current_stream())
    else:
        rc = lib.rrl_nav_step_push_packed(len(runs), co.ENV_KIND[runs[0].c.env], arr, _lib.current_stream())
    torch.cuda.synchronize()
    return rc


def packed_case(env_class, regime):
    lib = _lib.load()
    lib.rrl_pack_clear()
    try:
        seeds = SP.packed_seeds(env_class, regime)
        runs = [Run(c) for c in seeds]
        for k in range(3):
            assert packed_launch(runs, k, env_class) == 0
            for r in runs:
                r.check(k)
        for r in runs:
            if r.c.gate == "head":
                r.pool.check()
            solo = Run(r.c, r.inputs)               # the seed alone, from a copy of the initial state
            for k in range(3):
                solo.launch(k)
            assert_same_bits(r.snapshot(), solo.snapshot(), r.c.name + " against its solo run")
            for j, (exact, bound) in enumerate(SP.reward_sums(r.ref)):
                assert abs(float(solo.sums[j]) - exact) <= bound
        # a seed of another regime in the call: refused, nothing written
        other = SP.packed_seeds(env_class, 1 - regime)[1]
        mixed = [Run(seeds[1]), Run(other)]
        before = [(m.snapshot(), m.sums.clone()) for m in mixed]
        assert packed_launch(mixed, 0, env_class) == EINVAL
        for m, (snap, sums) in zip(mixed, before):
            now = m.snapshot()
            assert_same_bits({key: now[key] for key in snap}, snap, "refused call")
            assert torch.equal(m.sums, sums)
    finally:
        lib.rrl_pack_clear()


@pytest.mark.parametrize("regime", (0, 1))
def test_packed_nav_step_equals_the_reference_and_the_solo_launches(regime):
    packed_case("nav", regime)


@pytest.mark.parametrize("regime", (0, 1))
def test_packed_maze_step_equals_the_reference_and_the_solo_launches(regime):
    packed_case("maze", regime)
