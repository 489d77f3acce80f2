"""rrl_ens_train_grad / rrl_ens_train_grad_big at kernel level, through a hand-made rrl_ens_t, on every case of
ens_train_cases.py: the loss and the ten gradients against the float64 restatement under rule 1, with sentinels in and guard
tails behind every output, a NaN-filled scratch of exactly the size the library asks for, and NaN in the one dataset row the
dead index columns point to; then what the sources promise bit for bit -- a dead second half writes zeros, a strided index view
is its contiguous copy, a repeated launch repeats, epoch() is its per-step calls -- and the refusals, which touch nothing.
test_ens_train_paths_cpu.py proves that the table reaches every launch edge and that rule 1 catches a kernel that is wrong."""
import pytest
import torch

import ens_train_cases as EC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_devices = {}


def device(name):
    if name not in _devices:
        _devices[name] = EC.Device(EC.operands(name), DEV)
    return _devices[name]


def _dirty(b, fields):
    """The outputs among `fields` that hold a sentinel or a non-finite number."""
    return [f for f in fields if not (bool(torch.isfinite(b[f]).all()) and bool((b[f] != EC.SENT).all()))]


# ---- values ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", EC.names())
def test_loss_and_gradients_against_float64(name):
    """Rule 1 on every quantity, and the memory discipline of the launch.  The largest ratios measured (3.38 and 3.54 on lin3_b at
    60 members, 3.57 on lin0_b) and the two cases that missed the rule at operand seed 0 (lin3_b at 4.42 and 5.32): LAB_NOTES.md
    and the comment above ens_train_cases.SEEDS."""
    c, d = EC.BY_NAME[name], device(name)
    b = d.buffers(c.entry, c.batch)
    assert b["scratch_n"] == EC.case_facts(c)["scratch"]          # the host sizes the scratch as launch_facts() restates it
    assert d.launch(c.entry, b) == EC.RRL_OK
    report = []
    bad = EC.compare(name, EC.out_of(c.entry, b), report)
    for k, dev, bound, ratio, member in report:                   # (kept by the run that fills LAB_NOTES.md)
        print("RATIO %s %s dev=%.3e bound=%.3e ratio=%.2f member=%d" % (name, k, dev, bound, ratio, member))
    assert not EC.tails_touched(b), EC.tails_touched(b)
    if c.entry == "small":
        assert not _dirty(b, EC.OUTPUT_FIELDS), _dirty(b, EC.OUTPUT_FIELDS)
    else:                                                         # gradients land in g_* alone
        fields = EC.GRAD_FIELDS + ("loss",)
        assert not _dirty(b, fields), _dirty(b, fields)
        assert not EC.touched(b, EC.SMALL_ONLY_FIELDS, scratch=False)
    # written, not added to: rule 1 holds from sentinels (below), and a second launch into the same buffers -- which now hold
    # the first one's results, the scratch its intermediates instead of NaN -- leaves the same bits
    first = {f + "_flat": b[f + "_flat"].clone() for f in EC.OUTPUT_FIELDS}
    assert d.launch(c.entry, b) == EC.RRL_OK
    assert not EC.same_bits(first, b), EC.same_bits(first, b)
    assert not EC.tails_touched(b)
    assert not bad, (bad, report)


# ---- what the sources promise bit for bit ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [n for n in EC.names("small") if EC.BY_NAME[n].batch <= EC.SMALL_R])
def test_a_dead_second_half_writes_zeros(name):
    c, d = EC.BY_NAME[name], device(name)
    assert EC.case_facts(c)["live"][1] == 0
    b = d.run("small")
    for f in EC.GRAD2_FIELDS:
        assert bool((b[f] == 0).all()), f
    half1 = torch.arange(c.E, device=DEV) * EC.HALVES + 1
    assert bool((b["g_logvar_part"][half1] == 0).all()) and bool((b["loss_part"][half1] == 0).all())
    assert not EC.tails_touched(b)


@pytest.mark.parametrize("entry,name", [("small", "small-E5-b1-plain-strided"), ("small", "small-E5-b17-wide-strided"),
                                        ("small", "small-E60-b32-plain-strided"), ("big", "big-E5-b65-thresh-strided"),
                                        ("big", "big-E7-b1100-plain-strided"), ("big", "big-E60-b300-plain-strided")])
def test_a_strided_index_view_is_its_contiguous_copy(entry, name):
    d = device(name)
    assert EC.BY_NAME[name].strided and not d.idx.is_contiguous() and d.idx.stride(0) == d.idx.shape[1] + EC.TABLE_EXTRA
    a, b = d.run(entry), d.run(entry, idx=d.idx.contiguous())
    assert not EC.same_bits(a, b), EC.same_bits(a, b)


@pytest.mark.parametrize("entry,name", [("small", "small-E5-b17-plain-contig"), ("small", "small-E5-b32-wide-contig"),
                                        ("small", "small-E60-b32-plain-strided"), ("big", "big-E5-b3300-plain-contig"),
                                        ("big", "big-E5-b65-wide-contig")])
def test_a_repeated_launch_into_fresh_buffers_repeats(entry, name):
    d = device(name)
    a, b = d.run(entry), d.run(entry)
    assert not EC.same_bits(a, b), EC.same_bits(a, b)


def test_the_large_batch_epoch_in_c_equals_the_per_step_calls():
    """epoch() at batch 128 over 300 columns = step_big on columns 0..127, 128..255 and 256..299 (44 rows: one tile, the scratch
    of the 128-row launches behind it): parameters, moments and step counts."""
    from recovery_rl_amd.ensemble_train import FusedEnsembleTrainer
    p = EC.operands("big-E5-b65-plain-contig")
    table = torch.randint(EC.N_ROWS, (5, 300), generator=torch.Generator().manual_seed(300)).to(DEV)
    train_in, train_targ = p["train_in"].to(DEV), p["train_targ"].to(DEV)
    trainers = []
    for _ in range(2):
        model = EC.model_of(p).to(DEV)
        assert FusedEnsembleTrainer.supported(model, 128)
        tr = FusedEnsembleTrainer(model)
        tr.begin(train_in, train_targ)
        trainers.append(tr)
    ta, tb = trainers
    ta.epoch(table, 128)
    for lo in range(0, 300, 128):
        tb.step_big(table[:, lo:lo + 128])
    torch.cuda.synchronize()
    for k, name in enumerate(EC.PARAMS):
        assert torch.equal(ta.params[k], tb.params[k]), name
        assert torch.equal(ta.m[k], tb.m[k]) and torch.equal(ta.v[k], tb.v[k]), name
        assert torch.equal(ta.steps[k], tb.steps[k]) and int(ta.steps[k][0].item()) == 3, name
        assert bool(torch.isfinite(ta.params[k]).all()) and not torch.equal(ta.params[k], p[name].to(DEV)), name
    assert torch.equal(ta.loss, tb.loss)


# ---- refusals -----------------------------------------------------------------------------------------------------------------
REFUSED = "small-E5-b32-lower-strided"        # its index table is 37 columns wide: 33 columns are in range
REFUSALS = {
    # what: (entry -> the code, the launch's keyword arguments)
    "n_nets = 61": (dict(small=EC.RRL_EINVAL, big=EC.RRL_EINVAL), dict()),
    "batch = 0": (dict(small=EC.RRL_ERANGE, big=EC.RRL_EINVAL), dict(batch=0)),
    "batch = 33": (dict(small=EC.RRL_ERANGE), dict(batch=33)),
    "hidden = 256": (dict(small=EC.RRL_ERANGE, big=EC.RRL_ERANGE), dict(hidden=256)),
    "a null gradient pointer": (dict(small=EC.RRL_EINVAL, big=EC.RRL_EINVAL), dict(g_w2=None)),
}


# (batch = 33 is the large-batch entry's to run)
@pytest.mark.parametrize("what,entry", [(what, entry) for what, (codes, _) in REFUSALS.items() for entry in codes])
def test_a_refused_call_returns_its_code_and_touches_nothing(what, entry):
    codes, kw = REFUSALS[what]
    if what == "n_nets = 61":                                     # operands of 61 members: every buffer is as large as it says
        if "E61" not in _devices:
            _devices["E61"] = EC.Device(EC.make_operands(EC.MAX_NETS + 1, 32, "plain", True, 0), DEV)
        d = _devices["E61"]
    else:
        d = device(REFUSED)
    assert d.table.shape[1] >= 33
    b = d.buffers(entry, 32)
    assert d.launch(entry, b, **kw) == codes[entry]
    assert not EC.touched(b), EC.touched(b)
