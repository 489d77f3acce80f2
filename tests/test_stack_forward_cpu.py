"""The case table of stack_cases.py reaches every kernel of the stack forward's dispatch, with ragged last blocks of both
kinds -- proven on the host from the constants parsed out of the sources, so that a retuned constant fails here instead of
moving a case of test_stack_forward_gpu.py onto another path unnoticed."""
import os
import re

import pytest
import torch

import stack_cases as SC

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "recovery_rl_amd", "csrc")


def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _one(pattern, text, what):
    found = re.findall(pattern, text)
    assert len(found) == 1, "%s: expected one definition in the source, found %r" % (what, found)
    return found[0]


def test_the_restated_constants_are_the_sources():
    fwd, pack, common = _src("mlp_fwd_kernels.hip"), _src("pack.hpp"), _src("mlp_common.hpp")
    got = {}
    for name in ("kStackRows", "kSplit", "kSplitSmallM", "kBigR", "kPackSmallR2MinSeeds", "kStackMaxH"):
        got[name] = int(_one(r"constexpr\s+int\s+%s\s*=\s*(\d+)\s*;" % name, fwd, name))
    got["RRL_FWD_LOOP_WAVES"] = int(_one(r"#define\s+RRL_FWD_LOOP_WAVES\s+(\d+)", fwd, "RRL_FWD_LOOP_WAVES"))
    mx, mn = _one(r"constexpr\s+int\s+kLoopMaxBlocks\s*=\s*(\d+)\s*,\s*kLoopMinBlocks\s*=\s*(\d+)\s*;", fwd, "kLoop*Blocks")
    got["kLoopMaxBlocks"], got["kLoopMinBlocks"] = int(mx), int(mn)
    assert _one(r"constexpr\s+int\s+kResidentWorkgroups\s*=\s*([^;]+);", fwd, "kResidentWorkgroups").strip() == "256 * RRL_FWD_LOOP_WAVES"
    # the plain path takes two row tiles per workgroup above 256 sixteen-row tiles x heads: in rrl_mlp3_forward and in
    # build_stack_group
    plain = re.findall(r"kStackRows\s*-\s*1\)\s*/\s*kStackRows\)\s*\*\s*G\s*>\s*(\d+)|tiles16\s*\*\s*p\.G\s*>\s*(\d+)", fwd)
    assert len(plain) == 2, plain
    assert {int(a or b) for a, b in plain} == {SC.CONSTANTS["plain_r2_above"]}
    got["plain_r2_above"] = SC.CONSTANTS["plain_r2_above"]
    got["kMaxGroup"] = int(_one(r"constexpr\s+int\s+kMaxGroup\s*=\s*(\d+)\s*;", common, "kMaxGroup"))
    got["kMaxSeeds"] = int(_one(r"constexpr\s+int\s+kMaxSeeds\s*=\s*(\d+)\s*;", pack, "kMaxSeeds"))
    assert got == SC.CONSTANTS
    assert (SC.ROWS, SC.SPLIT, SC.SMALL_M, SC.BIG_R, SC.PACK_SMALL_R2_MIN_SEEDS, SC.LOOP_WAVES, SC.LOOP_MIN, SC.LOOP_MAX,
            SC.PLAIN_R2_ABOVE, SC.MAX_GROUP, SC.MAX_H) == tuple(SC.CONSTANTS[k] for k in (
                "kStackRows", "kSplit", "kSplitSmallM", "kBigR", "kPackSmallR2MinSeeds", "RRL_FWD_LOOP_WAVES", "kLoopMinBlocks",
                "kLoopMaxBlocks", "plain_r2_above", "kMaxGroup", "kStackMaxH"))
    assert SC.RESIDENT == 768
    # the split condition and the rule that sends a split member to the one-row tiles
    assert "(H % (16 * kSplit)) == 0 && H <= kStackMaxH" in fwd
    assert fwd.count("M <= kSplitSmallM || H != 256") == 1 and fwd.count("p.M <= kSplitSmallM || p.H != 256") == 1
    # the pinned-mapping rule of pack.hpp, by its three decisions
    assert "if (8 * ((S + 7) / 8) - S > 2) return false;" in pack
    assert "if (!always && sp == 8 && S <= 6) {" in pack
    assert "return pinned_mapping(S, sp, p, r) ? sp * r : 1;" in pack


def test_the_pinned_mapping_restated():
    """pack.hpp's table: S <= 4 and 7, 8 pinned on sp XCD groups, 5 and 6 linear, above 8 pinned when at most two XCDs lack a
    seed of the last round."""
    share = {S: SC.seed_share(S) for S in range(1, 17)}
    assert share == {1: 1, 2: 2, 3: 4, 4: 4, 5: 1, 6: 1, 7: 8, 8: 8, 9: 1, 10: 1, 11: 1, 12: 1, 13: 1, 14: 16, 15: 16, 16: 16}


def test_every_dispatch_label_and_every_ragged_block_has_a_case():
    hit = {label: [] for label in SC.LABELS}
    for case in SC.CASES:
        path = SC.case_path(case)
        assert path.label in hit, (case.name, path.label)
        hit[path.label].append((case, path))
    missing = [label for label, cases in hit.items() if not cases]
    assert not missing, "no case reaches %r" % missing

    def rests(label, rows):
        """M modulo the block, over the members of the label's cases that run on blocks of `rows` rows."""
        return {m.M % rows for case, path in hit[label] for m, r in zip(SC.flat_members(case), path.rows) if r == rows}
    for label in SC.TWO_ROW_LABELS:
        got = rests(label, 32)
        assert got & set(range(1, 16)), (label, "no last block without its second row tile", sorted(got))
        assert got & set(range(17, 32)), (label, "no last block with a partial second row tile", sorted(got))
    for label in SC.ONE_ROW_LABELS:
        got = rests(label, 16)
        assert got - {0}, (label, "no ragged last block", sorted(got))
    # both bodies of path 0, and the flat grid with its large member first and last
    assert {m.H for case, _ in hit["0/gen"] for m in case.members} >= {64, 128, 192}
    order = {tuple(m.M > SC.SMALL_M for m in case.members) for case, _ in hit["5"]}
    assert any(o[0] and not o[-1] for o in order) and any(o[-1] and not o[0] for o in order)
    assert any(len(case.members) == SC.MAX_GROUP for case, _ in hit["0/256"])
    # the small members of a packed launch on two-row tiles: from three seeds on, and beside a large member
    assert any(path.small_r == SC.BIG_R and len(case.members) >= SC.PACK_SMALL_R2_MIN_SEEDS for case, path in hit["packed3/small2"])
    assert any(path.small_r == 1 and len(case.members) == 2 for case, path in hit["packed3/small2"])
    assert {m.H for case, _ in hit["packed0"] for g in case.members for m in g} >= {128, 256}
    # the loop form: at least kLoopMinBlocks blocks per workgroup, a last workgroup that walks fewer, ragged last blocks; once
    # with the input head, whose values it keeps in LDS of its own
    for case, path in hit["packed4"]:
        assert path.loop and path.nb >= SC.LOOP_MIN and path.small_r == SC.BIG_R
        assert all(0 < w < path.nb for w in path.walks), (case.name, path.walks)
        assert all(m.M % 32 != 0 for m in SC.flat_members(case))
    assert any(case.opts.get("heads") for case, _ in hit["packed4"])
    # an input head on paths 0 (both bodies), 3 and 5
    assert {SC.case_path(SC.BY_NAME[n]).label for n in SC.names("multi", heads=True)} == {"0/256", "0/gen", "3", "5"}
    # one strided x (ldx 7 > din) per label whose kernel reads x through ldx: all but the keyed riders, which read the ring
    # (the packed kernels take ldx from the plan's device copy of the arguments, the loop form fetches x one block ahead)
    strided = {SC.case_path(c).label for c in SC.CASES if c.opts.get("strided")}
    assert strided == set(SC.LABELS) - {"riders_keyed"}, sorted(set(SC.LABELS) - strided)
    assert {SC.case_path(c).path for c in SC.CASES if c.entry == "riders" and c.opts.get("strided")} == {0, 3}
    # h1 and h2 null (the target networks' forwards) on every label, and saved on every label
    for save in (False, True):
        got = {SC.case_path(c).label for c in SC.CASES if c.opts.get("save", True) == save and not c.opts.get("heads")}
        assert got == set(SC.LABELS), (save, sorted(set(SC.LABELS) - got))
    # the path number the host stores in a packed plan
    assert {path.path for _, path in hit["packed0"]} == {0} and {path.path for _, path in hit["packed4"]} == {4}
    assert {path.path for label in ("packed3", "packed3/small2") for _, path in hit[label]} == {3}


def test_the_issue_s_loop_case_by_hand():
    """8 pinned seeds may hold 768 / 8 = 96 workgroups each: 86 blocks x 2 heads x 4 column groups fit from 8 blocks per
    workgroup on (11 x 8 = 88), and the eleventh workgroup walks 86 - 80 = 6."""
    path = SC.case_path(SC.BY_NAME["packed-S8-loop"])
    assert (path.label, path.nb, set(path.tiles), set(path.walks)) == ("packed4", 8, {86}, {6})
    assert {m.M % 32 for m in SC.flat_members(SC.BY_NAME["packed-S8-loop"])} == {5, 21}
    # and what does not loop: two seeds of the same members are resident at once
    two = SC.forward_path([[SC.Member(2, 2725, 256, 4, 1)]] * 2, packed_S=2)
    assert (two.label, two.nb) == ("packed3", 1)


def test_what_the_host_refuses_is_refused_here():
    with pytest.raises(ValueError):      # a split member and a plain one
        SC.forward_path([SC.Member(2, 200, 256, 4, 1), SC.Member(2, 200, 48, 4, 1, False)])
    with pytest.raises(ValueError):      # paths 0 and 3 outside hidden width 256 do not mix
        SC.forward_path([SC.Member(2, 200, 128, 4, 1), SC.Member(2, 1057, 256, 4, 1)])
    with pytest.raises(ValueError):      # the packed entry covers the column-split kernels only
        SC.forward_path([[SC.Member(2, 200, 48, 4, 1, False)]] * 2, packed_S=2)


def test_the_integer_bound_holds_for_every_case():
    worst = 0
    for case in SC.CASES:
        for m in SC.flat_members(case):
            b1, b2, b3 = SC.bound(m)
            assert b1 <= 18 and b2 <= 9218 and b3 <= 4719618 < 2 ** 24, (case.name, m)
            worst = max(worst, b3)
    assert worst == 4719618               # H = 256, din = 4 is among the cases


def _last_block(M, rows, clamp=True, slack=0):
    """Rows the last block of `rows` rows reads and stores, by the kernels' rule: lane r reads row m0 + min(r, last) and stores
    row m0 + r where r <= last; `clamp` False drops the read clamp, `slack` widens the store guard by that many rows."""
    m0 = (SC.ceil_div(M, rows) - 1) * rows
    last = M - 1 - m0
    return [m0 + (min(r, last) if clamp else r) for r in range(rows)], [m0 + r for r in range(rows) if r <= last + slack]


def test_a_broken_store_guard_would_show_and_no_broken_guard_or_clamp_could_leave_the_buffers():
    """What the GPU cases rest on, member by member on the host.  As written the last block reads and stores rows below M only.
    A store guard too wide, by one row or by the whole block, writes rows M .. M + 31 at most: for the last head those are the
    guard rows -- inside the allocation, and a sentinel that no integer result equals; G = 1 members exist on every label, so no
    next head's rows hide it.  That is what the GPU cases would show.
    A dropped `M - 1 - m0` read clamp alone they would NOT show: its dead lanes read rows M .. M + 31 at most, NaN rows INSIDE
    the input buffer, and as rows are independent and the store guards keep dead rows out, the NaN reaches nothing that is
    compared.  The NaN rows make such a read harmless by construction and show a kernel that mixes rows; no more is claimed."""
    g1 = set()
    for case in SC.CASES:
        path = SC.case_path(case)
        for m, rows in zip(SC.flat_members(case), path.rows):
            if m.M % rows == 0:
                continue
            reads, stores = _last_block(m.M, rows)
            assert max(reads) == m.M - 1 and max(stores) == m.M - 1
            reads, _ = _last_block(m.M, rows, clamp=False)
            assert m.M <= max(reads) < m.M + SC.DEAD_ROWS
            _, stores = _last_block(m.M, rows, slack=1)
            assert max(stores) == m.M                 # the last head's row M: the first guard row of h1, h2, out and a partial
            _, stores = _last_block(m.M, rows, slack=rows)
            assert m.M <= max(stores) < m.M + SC.GUARD_ROWS
            if m.G == 1:
                g1.add(path.label)
    assert g1 == set(SC.LABELS), sorted(set(SC.LABELS) - g1)
    assert SC.SENT != round(SC.SENT)


def test_the_reference_is_a_linear_chain():
    m = SC.Member(2, 33, 128, 4, 1)
    p, ref = SC.problem(m)
    for g in range(m.G):
        l1, l2, l3 = torch.nn.Linear(m.din, m.H), torch.nn.Linear(m.H, m.H), torch.nn.Linear(m.H, m.dout)
        with torch.no_grad():
            for lin, W, b in ((l1, "W1", "b1"), (l2, "W2", "b2"), (l3, "W3", "b3")):
                lin.double()
                lin.weight.copy_(p[W][g])
                lin.bias.copy_(p[b][g])
            h1 = torch.relu(l1(p["x"]))
            h2 = torch.relu(l2(h1))
            assert torch.equal(h1, ref["h1"][g]) and torch.equal(h2, ref["h2"][g]) and torch.equal(l3(h2), ref["out"][g])
    assert torch.equal(ref["partials"].sum(0), ref["out"])
    assert float(ref["h2"].abs().max()) > 100 and float(ref["out"].abs().max()) > 100      # not a degenerate problem
    assert bool((ref["h1"] == 0).any()) and bool((ref["h2"] == 0).any())                 # both relus cut
