"""The stack backward family (csrc/mlp_kernels.hip) at kernel level, through its descriptors alone and on every kernel its host
dispatch can choose -- the case table of backward_cases.py, which test_backward_paths_cpu.py proves complete -- against torch
float64: torch.equal for the exact cases, the derived bound n 2^-23 A for the rounded ones (backward_cases.py has both
rules).  Every case also checks what a kernel must not do: the floats behind every output keep their sentinel, an output no
descriptor asks for is allocated all the same and stays untouched, and NaN rows lie behind every input.  Then the promises of
include/rrl_hip.h, bit for bit: n members in one launch against n launches of one, the paired launch against head launch +
hidden launch, every seed of a packed launch against its solo launch, folded dx partials against ((p0 + p1) + p2) + p3 of the
tile partials."""
import pytest
import torch

import backward_cases as BC
from recovery_rl_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module", autouse=True)
def plans_do_not_outlive_their_buffers():
    """Packed plans are keyed by the descriptors' bytes, pointers included."""
    yield
    torch.cuda.synchronize()
    _lib.load().rrl_pack_clear()


def _fresh(groups, fold=None):
    return [[mb.outputs(fold) for mb in g] for g in groups]


def _run(entry, groups, fold=None):
    outs = _fresh(groups, fold)
    rc = BC.launch(entry, groups, outs)
    torch.cuda.synchronize()
    return rc, outs


def _label(entry, seeds):
    try:
        return BC.backward_path(entry, tuple(tuple(g) for g in seeds))
    except BC.Refused as e:
        return e.rc


def _solo(entry, group, main_outs, main_paired, what):
    """The same members through the solo entry: bit for bit the outputs of the launch under test.  A folding member goes
    unfolded where the solo entry takes the one-tile-per-workgroup form; heads[k].dh2 is compared only where both launches
    write it (or neither)."""
    label = _label(entry, [[mb.m for mb in group]])
    paired = label in BC.PAIRED_LABELS
    fold = None if paired else False
    rc, (outs,) = _run(entry, [group], fold)
    assert rc == BC.RRL_OK, (what, rc)
    for mb, a, b in zip(group, main_outs, outs):
        BC.same_bits(a, b, what, skip=() if paired == main_paired else ("dh2",))


@pytest.mark.parametrize("name", BC.names())
def test_backward_case(name):
    case = BC.BY_NAME[name]
    removed = BC.removed_by_env(case)
    if removed:
        pytest.skip("an RRL_PACK_PAIR_* setting takes this case off the label %s" % removed)
    label = _label(case.entry, case.seeds)
    assert (label if isinstance(label, int) else None) == case.opts.get("refused"), label
    groups = [[BC.Member(case.entry, m, 10 * s + k, DEV) for k, m in enumerate(g)] for s, g in enumerate(case.seeds)]
    rc, outs = _run(case.entry, groups)
    if isinstance(label, int):          # refused before anything is launched: the predicted code, nothing written
        assert rc == label, (name, rc)
        assert not [BC.untouched(o) for og in outs for o in og if BC.untouched(o)]
        return
    assert rc == BC.RRL_OK, (name, rc)
    paired = label in BC.PAIRED_LABELS
    for s, (g, og) in enumerate(zip(groups, outs)):
        for k, (mb, o) in enumerate(zip(g, og)):
            what = (name, label, "seed %d member %d" % (s, k))
            written = [x for x in mb.asked() if not (paired and x == "dh2")]
            BC.check_member(mb, o, written, what)
            if case.entry == "pair" and mb.m.dh2:
                # one launch: the link between the stages is not written; two launches: it holds dh2
                assert bool((o["dh2"] == BC.SENT).all()) == paired, what
    # every seed of a packed launch equals its solo launch
    if len(groups) > 1:
        for s, (g, og) in enumerate(zip(groups, outs)):
            _solo(case.entry, g, og, paired, (name, "seed %d against its solo launch" % s))
    # a launch of n members equals n launches of one member each
    for s, (g, og) in enumerate(zip(groups, outs)):
        if len(g) > 1:
            for k, (mb, o) in enumerate(zip(g, og)):
                if case.entry == "input" and not (mb.m.need_w or mb.m.need_x):
                    continue
                _solo(case.entry, [mb], [o], paired, (name, "seed %d member %d against a launch of its own" % (s, k)))
    # the paired launch equals the head launch followed by the hidden launch (which cannot fold: the tile partials, folded here)
    if paired:
        for s, (g, og) in enumerate(zip(groups, outs)):
            two = _fresh([g], False)
            assert BC.launch("head", [g], two) == BC.RRL_OK and BC.launch("hidden", [g], two) == BC.RRL_OK
            torch.cuda.synchronize()
            for k, (mb, a, b) in enumerate(zip(g, og, two[0])):
                what = (name, "seed %d member %d against head launch + hidden launch" % (s, k))
                BC.same_bits(a, b, what, skip=("dh2",))
                BC.check_member(mb, b, mb.asked(), what)
    # folded dx partials equal ((p0 + p1) + p2) + p3 of the tile partials: the solo hidden launches above ran unfolded, and so
    # did the two launches of a paired case; what is left is the fold inside the paired form against the same form unfolded
    if paired and any(mb.m.fold for g in groups for mb in g):
        rc, flat = _run(case.entry, groups, False)
        assert rc == BC.RRL_OK
        for g, og, fg in zip(groups, outs, flat):
            for mb, a, b in zip(g, og, fg):
                BC.same_bits(a, b, (name, "folded against the same launch unfolded"))


def test_the_table_runs_every_label_here():
    """With RRL_PACK_PAIR_* unset nothing is skipped above; a setting that moves a case says which label it leaves."""
    moved = {c.name: BC.removed_by_env(c) for c in BC.CASES if BC.removed_by_env(c)}
    if moved:
        pytest.skip("RRL_PACK_PAIR_* removes %s" % sorted(set(moved.values())))
    hit = {_label(c.entry, c.seeds) for c in BC.CASES}
    assert hit >= set(BC.LABELS)
