"""The case table of backward_cases.py reaches every kernel of the stack backward's dispatch at the shapes where each can go
wrong -- proven on the host from the constants, the two seed thresholds and the `pair =` condition parsed out of the sources, so
that a retuned constant fails here instead of moving a case of test_backward_paths_gpu.py onto another path unnoticed -- and the
float64 reference it compares with is the backward of a three-layer stack as torch.autograd computes it."""
import os
import re

import pytest
import torch

import backward_cases as BC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "recovery_rl_amd", "csrc")


def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _one(pattern, text, what, flags=0):
    found = re.findall(pattern, text, flags)
    assert len(found) == 1, "%s: expected one definition in the source, found %r" % (what, found)
    return found[0]


def _squash(text):
    return re.sub(r"\s+", " ", text).strip()


def _labels():
    """label (or the refusal's code) -> [case]."""
    hit = {}
    for case in BC.CASES:
        try:
            label = BC.case_path(case, env={})
        except BC.Refused as e:
            label = e.rc
        hit.setdefault(label, []).append(case)
    return hit


def _members(cases):
    return [m for c in cases for m in BC.flat_members(c)]


# ---- the restatement is the source's ------------------------------------------------------------------------------------------
def test_the_restated_constants_are_the_sources():
    mlp, common, pack = _src("mlp_kernels.hip"), _src("mlp_common.hpp"), _src("pack.hpp")
    got = {}
    for name in ("kTile", "kPanel", "kPairPanel", "kPairDsh", "kBlkPanel"):
        got[name] = int(_one(r"constexpr\s+int\s+%s\s*=\s*(\d+)\s*;" % name, mlp, name))
    cols = _one(r"constexpr\s+int\s+kCols\s*=\s*(\d+)\s*,\s*kSlices\s*=\s*(\d+)\s*,\s*kUnroll\s*=\s*(\d+)\s*;", mlp, "kCols, kSlices, kUnroll")
    got["kCols"], got["kSlices"], got["kUnroll"] = (int(v) for v in cols)
    got["kMaxGroup"] = int(_one(r"constexpr\s+int\s+kMaxGroup\s*=\s*(\d+)\s*;", common, "kMaxGroup"))
    got["kMaxSeeds"] = int(_one(r"constexpr\s+int\s+kMaxSeeds\s*=\s*(\d+)\s*;", pack, "kMaxSeeds"))
    for name in ("RRL_PACK_PAIR_MAX_SEEDS", "RRL_PACK_PAIR_BLOCK_MAX_SEEDS"):
        got[name] = int(_one(r'env_int\("%s",\s*(-?\d+)\)' % name, mlp, name))
    tail = _one(r"const bool tail_free = B \* dout <= ([^;]+);", mlp, "tail_free")
    assert tail.strip() == "1024 * 4 - 6 * 16"
    got["tail_floats"] = 1024 * 4 - 6 * 16
    assert got == BC.CONSTANTS
    assert (BC.TILE, BC.PANEL, BC.PAIR_PANEL, BC.PAIR_DSH, BC.BLK_PANEL, BC.COLS, BC.CHUNK, BC.MAX_GROUP, BC.MAX_SEEDS,
            BC.TAIL_FLOATS) == (got["kTile"], got["kPanel"], got["kPairPanel"], got["kPairDsh"], got["kBlkPanel"], got["kCols"],
                                got["kSlices"] * got["kUnroll"], got["kMaxGroup"], got["kMaxSeeds"], got["tail_floats"])
    # the head backward's chunk loop and the environment's reading
    assert "for (int b0 = 0; b0 < B; b0 += kSlices * kUnroll) {" in mlp
    assert "return e ? atoi(e) : fallback;" in mlp


def test_the_restated_decisions_are_the_sources():
    mlp = _src("mlp_kernels.hip")
    assert _one(r"static int pack_panel\(int S\) \{\s*([^}]+?)\s*\}", mlp, "pack_panel") == BC.PACK_PANEL_BODY
    assert _one(r"static int pack_block\(int S\) \{\s*([^}]+?)\s*\}", mlp, "pack_block") == BC.PACK_BLOCK_BODY
    assert [BC.pack_panel(S) for S in (1, 2, 3, 4, 16)] == [128, 64, 32, 32, 32]
    assert [BC.pack_block(S) for S in (1, 2, 3, 4, 16)] == [0, 0, 12, 12, 12]
    # hidden_args' FAST geometry, hidden_blocks, wants_fold and where a fold is refused
    assert ("return (H % kTile) == 0 && (B % kTile) == 0 && (H % kPanel) == 0 && (B % kPanel) == 0 && al(p.dh2) && al(p.h1) && "
            "al(p.W2);") in mlp
    assert "if (!hg.fast[k] || p.H % bm || p.H % bn || p.B % bm || p.H % kBlkPanel || p.B % kBlkPanel) return false;" in mlp
    assert "if (ps[k].first.x && ps[k].first.dx_part && ps[k].first.dx_fold) return true;" in mlp
    assert mlp.count("if (wants_fold(n, ps)) return RRL_ERANGE;") == 1 and mlp.count("if (wants_fold(n, hidden)) return RRL_ERANGE;") == 1
    assert "if (shape != 12)" in mlp and "if (wants_fold(n[s], members[s])) return RRL_ERANGE;" in mlp
    assert "if (first && !hg.fast[k]) return RRL_ERANGE;" in mlp
    assert "if (shape) ok = hidden_blocks(n[s], members[s], hg, shape / 10, shape % 10);" in mlp
    assert "l.i1 = shape ? -shape : pack_panel(S);" in mlp
    # launch_head_group: one member with a loss description has a kernel of its own
    body = _one(r"static void launch_head_group\(.*?\) \{(.*?)\n\}", mlp, "launch_head_group", re.S)
    assert _squash(body).startswith("if (n == 1) {") and body.count("head_bwd_loss_kernel<") == 6
    assert "case RRL_LOSS_DGD_QRISK: hipLaunchKernelGGL((head_bwd_loss_kernel<RRL_LOSS_QRISK_POLICY>)" in _squash(body)
    # the paired entries
    assert "const bool blocks = S > pack_pair_max_seeds();" in mlp and "bool pair = S <= pack_pair_block_max_seeds();" in mlp
    assert "if (pair && blocks) pair = hidden_blocks(n, hidden, hd, 1, 2);" in mlp
    assert "pair = pair && (dout == 0 || dout == my);" in mlp
    cond = _one(r"\n\s+pair = (my != 0.*?);", mlp, "the `pair =` condition", re.S)
    assert tuple(_squash(c) for c in cond.split("&&")) == BC.PAIR_CLAUSES
    assert ("const int my = ((kind >= RRL_LOSS_SAC_CRITIC && kind <= RRL_LOSS_QRISK_POLICY) || kind == RRL_LOSS_DGD_QRISK) ? 1 : "
            "kind == RRL_LOSS_GAUSS_HEAD ? 4 : kind == RRL_LOSS_STOCH_HEAD ? 2 : 0;") in _squash(mlp)
    assert set(BC.SOLE_CLAUSES) | set(BC.IMPLIED_BY_FAST) | set(BC.UNREACHED_CLAUSES) == set(BC.PAIR_CLAUSES)
    assert len(BC.SOLE_CLAUSES) + len(BC.IMPLIED_BY_FAST) + len(BC.UNREACHED_CLAUSES) == len(BC.PAIR_CLAUSES)


def test_the_environment_is_read_as_the_host_reads_it():
    assert [BC._atoi(t) for t in ("4", " 12x", "x", "", "-1", "+3 ", "0")] == [4, 12, 0, 0, -1, 3, 0]
    two = (tuple([BC.loss("sac_critic", 128, 128)]),) * 2
    assert BC.backward_path("pair", two, env={}) == "pair-pack<1>"
    assert BC.backward_path("pair", two, env={"RRL_PACK_PAIR_MAX_SEEDS": "1"}) == "pair-block-pack<1>"
    assert BC.backward_path("pair", two, env={"RRL_PACK_PAIR_BLOCK_MAX_SEEDS": "1"}) == "pair-split"
    assert BC.backward_path("pair", two * 2, env={"RRL_PACK_PAIR_MAX_SEEDS": "junk"}) == "pair-block-pack<1>"
    case = BC.BY_NAME["pair-S2-pack"]
    assert BC.removed_by_env(case, env={}) is None
    assert BC.removed_by_env(case, env={"RRL_PACK_PAIR_MAX_SEEDS": "0"}) == "pair-pack<1>"


# ---- the table reaches every path and every edge ------------------------------------------------------------------------------
def test_every_label_has_a_case_and_every_refusal_is_the_predicted_one():
    hit = _labels()
    assert not [label for label in BC.LABELS if not hit.get(label)], [label for label in BC.LABELS if not hit.get(label)]
    assert set(hit) - set(BC.LABELS) == {BC.RRL_ERANGE}
    for label, cases in hit.items():
        for case in cases:
            assert case.opts.get("refused") == (label if isinstance(label, int) else None), case.name
            assert all(m.B <= 1024 and m.H <= 256 for m in BC.flat_members(case)), case.name
            assert all(0 < len(g) <= BC.MAX_GROUP for g in case.seeds) and len(case.seeds) <= BC.MAX_SEEDS
    # what the issue names: the same description folds in the block form from three seeds on and is refused at two
    assert BC.BY_NAME["hidden-S3-block-fold"].seeds[:2] == BC.BY_NAME["hidden-S2-fold-refused"].seeds
    assert BC.BY_NAME["hidden-S3-block-fold"] in hit["pack-block"] and BC.BY_NAME["hidden-S4-block-fold"] in hit["pack-block"]
    for label in BC.LABELS:       # every label has an exact case but those whose kinds are never exact
        rounded_only = label in ("loss-kernel-qrisk_critic", "loss-kernel-qrisk_policy", "loss-kernel-dgd_qrisk",
                                 "loss-kernel-gauss", "loss-kernel-stoch") or label.endswith("<2>") or label.endswith("<4>")
        assert any(BC.case_exact(c) for c in hit[label]) != rounded_only, label
    for label in ("head-group", "head-pack", "pair<1>", "pair-fallback", "pair-pack<1>", "pair-block-pack<1>", "pair-split"):
        assert any(not BC.case_exact(c) for c in hit[label]), label


def test_the_sizes_of_the_issue_are_in_the_table():
    hit = _labels()
    solo = lambda entry: [c for c in BC.CASES if c.entry == entry and len(c.seeds) == 1 and not c.opts.get("refused")]
    shapes = lambda cases: {(m.H, m.B) for m in _members(cases)}
    assert shapes(solo("hidden")) >= {(48, 40), (128, 64), (128, 256), (256, 128)}
    assert {m.G for m in _members(solo("hidden"))} >= {1, 2, 3}
    four = [c for c in solo("hidden") if len(c.seeds[0]) == BC.MAX_GROUP]
    assert any(len({(m.G, m.B, m.H) for m in c.seeds[0]}) == 4 for c in four)
    firsts = {(m.first, m.dh1) for m in _members(solo("hidden")) if m.first}
    assert firsts >= {("w", True), ("x", True), ("wx", True), ("wx", False)}
    assert {m.din for m in _members(solo("hidden")) if m.first} >= {2, 4} and any(m.first and m.strided for m in _members(solo("hidden")))
    assert any(not m.dW2 for m in _members(solo("hidden")))
    # hidden, packed
    packed = [c for c in BC.CASES if c.entry == "hidden" and len(c.seeds) > 1]
    for S in (2, 3):
        assert any(len(c.seeds) == S and len({len(g) for g in c.seeds}) > 1 for c in packed), S
    assert any(len(c.seeds) == 3 and any(m.H == 48 for m in BC.flat_members(c)) for c in hit["pack-panel32"])
    assert {len(c.seeds) for c in hit["pack-block"] if any(m.fold and m.first for m in BC.flat_members(c))} >= {3, 4}
    # head
    plain_heads = {(m.H, m.B) for m in _members(hit["head-group"]) if m.kind == "plain"}
    assert plain_heads >= {(H, B) for H in (16, 40, 256) for B in (1, 17, 256, 257, 1024)}
    for kind in BC.KINDS:
        assert any(m.H == 40 for m in _members(hit["loss-kernel-" + kind])), kind
    assert {m.B for m in _members(hit["head-group"]) if m.kind == "plain" and m.dout == 4} >= {1000, 1001, 1024}
    assert any(not m.dh2 for m in _members(solo("head"))) and any(not m.dW3 for m in _members(solo("head")))
    assert any(len(c.seeds[0]) == 4 and {m.kind == "plain" for m in c.seeds[0]} == {True, False} for c in hit["head-group"])
    assert {len(c.seeds) for c in hit["head-pack"]} >= {2, 3}
    # pair
    assert shapes(hit["pair<1>"]) >= {(128, 128), (128, 256), (256, 128), (128, 384), (128, 1024)}
    assert shapes(hit["pair<2>"]) >= {(128, 256), (256, 512)} and shapes(hit["pair<4>"]) >= {(256, 128), (128, 256)}
    assert {len(c.seeds[0]) for c in hit["pair<1>"]} >= {1, 3}
    for label in ("pair<1>", "pair<4>"):
        assert {m.fold for m in _members(hit[label]) if m.first} == {False, True}, label
    assert {len(c.seeds) for label in BC.PAIR_LABELS for c in hit[label] if len(c.seeds) > 1} >= {2, 3, 8, 9}
    assert {len(c.seeds) for c in hit["pair-pack-fallback"]} == {3} and {len(c.seeds) for c in hit["pair-split"]} == {9}
    # input
    inputs = _members(solo("input"))
    assert {(m.need_w, m.need_x) for m in inputs} == {(True, False), (False, True), (True, True), (False, False)}
    assert {m.B for m in inputs} >= {1, 5, 200} and {m.H for m in inputs} == {16, 40} and any(m.strided for m in inputs)
    assert any([(m.need_w or m.need_x) for m in c.seeds[0]] == [True, False, True] for c in solo("input"))
    assert any(len({m.G for m in c.seeds[0]}) == 4 for c in solo("input"))


def test_every_clause_of_the_pair_condition_has_its_fallback():
    """For every clause that can fail alone, a case of the two-launch path on which only that clause (and what follows from it) is
    false; the clauses that follow from hd.fast[k] do follow from it and fail in the table with it."""
    failing = {}
    for case in _labels()["pair-fallback"]:
        dout, bad = 0, None
        for m in case.seeds[0]:
            vals = BC.pair_clauses(m, dout)
            if not all(vals.values()):
                bad = frozenset(k for k, v in vals.items() if not v)
                break
            dout = BC.KIND_DOUT[m.kind]
        assert bad, case.name
        failing[case.name] = bad
    for clause in BC.SOLE_CLAUSES:
        allowed = {clause} | (set(BC.IMPLIED_BY_FAST) if clause == "hd.fast[k]" else set())
        assert any(clause in bad and bad <= allowed for bad in failing.values()), clause
    assert frozenset(["hd.fast[k]"]) in failing.values()                  # and alone: an operand off its 16-byte boundary
    for clause in BC.IMPLIED_BY_FAST:
        assert any(clause in bad for bad in failing.values()), clause
    for B in range(1, 1025):
        for H in range(1, 257):
            m = BC.loss("sac_critic", B, H)
            vals = BC.pair_clauses(m, 0)
            if vals["hd.fast[k]"]:
                assert all(vals[c] for c in BC.IMPLIED_BY_FAST), (B, H)
                assert all(BC.pair_clauses(m._replace(dW2=False), 0)[c] for c in BC.IMPLIED_BY_FAST), (B, H)
    assert all(isinstance(why, str) and why for why in BC.UNREACHED_CLAUSES.values())


def test_the_ragged_conditions_are_reached_on_every_label_they_apply_to():
    hit = _labels()
    # the tile kernels' generic form: a ragged last tile in B and in H, a K that is no panel multiple
    for label in ("tile-ragged", "tile-mixed", "pack-panel64", "pack-panel32"):
        ms = [m for m in _members(hit[label]) if not BC.hidden_fast(m)]
        assert any(m.B % BC.TILE for m in ms) and any(m.H % BC.TILE for m in ms), label
        assert any(m.B % BC.TILE == 0 and m.H % BC.TILE == 0 for m in ms) or label != "tile-ragged", label
    for label in ("pair-fallback", "pair-pack-fallback"):
        assert any(m.B % BC.TILE for m in _members(hit[label])), label
    # the head backward: a partial last column block; a B % 256 remainder behind one whole chunk; tail_free from both sides
    for label in BC.HEAD_LABELS:
        ms = _members(hit[label])
        assert any(m.H % BC.COLS for m in ms), label
        assert any(m.B > BC.CHUNK and m.B % BC.CHUNK for m in ms), label
    assert any(m.H % BC.COLS for m in _members(hit["pair-fallback"]))
    for label in ("head-group", "head-pack", "loss-kernel-gauss"):
        sizes = {m.B * m.dout for m in _members(hit[label])}
        assert any(s <= BC.TAIL_FLOATS for s in sizes) and any(s > BC.TAIL_FLOATS for s in sizes), label
    plain4 = {m.B * m.dout for m in _members(hit["head-group"]) if m.kind == "plain"}
    assert BC.TAIL_FLOATS in plain4 and BC.TAIL_FLOATS + 4 in plain4                # B = 1000 against 1001 at dout = 4
    # the dOut tile of the paired launches exactly full, for every dout
    for dout in (1, 2, 4):
        assert any(m.B * m.dout == BC.PAIR_DSH for m in _members(hit["pair<%d>" % dout])), dout
    # the input backward: a ragged last block of four rows, and of sixteen columns
    inputs = _members(hit["input-group"])
    assert any(m.B % 4 for m in inputs if m.need_x) and any(m.H % BC.COLS for m in inputs if m.need_w)


# ---- the reference and the two comparison rules ---------------------------------------------------------------------------------
def _surrogate_dout(m, seed):
    """A stand-in for the f32 dOut of a rounded member (the GPU test takes rrl_loss_dout's): only its being f32 matters here."""
    gen = torch.Generator().manual_seed(seed)
    return torch.randn(m.G, m.B, m.dout, generator=gen).double()


def test_every_exact_member_satisfies_its_exactness_bound_and_every_rounded_one_its_condition():
    worst, seen = 0.0, set()
    for case in BC.CASES:
        for s, g in enumerate(case.seeds):
            for k, m in enumerate(g):
                key = (case.entry, m)
                if key in seen:
                    continue
                seen.add(key)
                p, r = BC.member_operands(case.entry, m, 10 * s + k)
                if BC.exact(m):
                    assert BC.closed_bound(case.entry, m, r) < 2 ** 24, (case.name, m)
                    ref, A = BC.chain(p, p["dOut"])
                    units = BC.exactness(case.entry, m, A)
                    assert units <= BC.closed_bound(case.entry, m, r) < 2 ** 24, (case.name, m, units)
                    worst = max(worst, units)
                    step = BC.step_of(m)
                    for name in BC.outputs_of(case.entry, m):       # every output a multiple of the step, and an f32 number
                        if name in ref:
                            assert torch.equal(ref[name] / step, (ref[name] / step).round()), (case.name, name)
                            assert torch.equal(ref[name].float().double(), ref[name]), (case.name, name)
                    assert float(p["dOut"].abs().max()) / step <= BC.dout_units(m, r)
                else:
                    # n 2^-23 A against 1e-3 A: a condition on n alone, and it holds elementwise on a stand-in dOut
                    assert max(BC.additions(m).values()) * 2.0 ** -23 < 1e-3, (case.name, m)
                    if (m.H, m.B) in ((128, 384), (256, 512), (40, 257)):
                        ref, A = BC.chain(p, _surrogate_dout(m, 10 * s + k))
                        for name, tol in BC.tolerance(m, A).items():
                            assert bool((tol <= 1e-3 * A[name]).all()) and float(A[name].max()) > 0, (case.name, name)
                            assert bool((ref[name].abs() <= A[name] * (1 + 1e-12)).all()), (case.name, name)
    assert 2 ** 10 < worst < 2 ** 24                    # (random signs and the masks keep the sums far below the closed form)


def test_the_narrow_range_is_taken_only_where_the_bound_asks_for_it():
    narrow = {(c.name, m) for c in BC.CASES for m in BC.flat_members(c) if BC.exact(m) and BC.operand_range(c.entry, m) == 1}
    for name, m in narrow:
        assert BC.closed_bound(BC.BY_NAME[name].entry, m, 2) >= 2 ** 24, (name, m)
    assert len(narrow) <= 4, sorted(n for n, _ in narrow)


@pytest.mark.parametrize("name", ("head-plain-H40-B257", "hidden-first-wx-ldx7", "pair-sac_critic-first", "input-both-B200-H16"))
def test_the_reference_is_autograd_s_backward_of_a_three_layer_stack(name):
    """One case per entry: x -> relu -> relu -> linear in float64 with the case's integer weights, the saved activations those the
    forward produces, L = sum(out * dOut); every gradient and every pre-activation gradient is chain()'s."""
    case = BC.BY_NAME[name]
    m = case.seeds[0][0]
    p, _ = BC.member_operands(case.entry, m, 0)
    gen = torch.Generator().manual_seed(5)
    b1, b2, b3 = BC.rints(gen, 2, m.G, m.H), BC.rints(gen, 2, m.G, m.H), BC.rints(gen, 2, m.G, m.dout)
    leaf = lambda t: t.clone().requires_grad_(True)
    x = leaf(p["x"].unsqueeze(0).repeat(m.G, 1, 1))          # a copy per head: dx [G,B,din] is per head
    W1, W2, W3, b1, b2, b3 = (leaf(t) for t in (p["W1"], p["W2"], p["W3"], b1, b2, b3))
    z1 = x @ W1.transpose(1, 2) + b1.unsqueeze(1)
    h1 = torch.relu(z1)
    z2 = h1 @ W2.transpose(1, 2) + b2.unsqueeze(1)
    h2 = torch.relu(z2)
    out = h2 @ W3.transpose(1, 2) + b3.unsqueeze(1)
    z1.retain_grad(), z2.retain_grad()
    (out * p["dOut"]).sum().backward()
    q = dict(p, h1=h1.detach(), h2=h2.detach())
    ref, A = BC.chain(q, p["dOut"])
    want = dict(dW3=W3.grad, db3=b3.grad, dh2=z2.grad, dW2=W2.grad, db2=b2.grad, dh1=z1.grad, dW1=W1.grad, db1=b1.grad, dx=x.grad)
    for k, v in want.items():
        assert torch.equal(ref[k], v), k
        assert bool((ref[k].abs() <= A[k]).all()), k
    if "first_part" in ref:
        n = m.G * m.H * m.din
        assert torch.equal(ref["first_part"].sum(0)[:n].reshape(m.G, m.H, m.din), W1.grad)
        assert torch.equal(ref["first_part"].sum(0)[n:].reshape(m.G, m.H), b1.grad)
        assert torch.equal(ref["dx_part"].sum(0), x.grad) and torch.equal(BC.fold4(ref["dx_part"]).sum(0), x.grad)
    assert bool((h1 == 0).any()) and bool((h2 == 0).any()) and float(ref["dx"].abs().max()) > 0      # both relus cut; not degenerate


def test_the_free_activations_of_the_table_cut_both_relus_and_differ_by_member():
    """The cases' h1 and h2 are free integers (a mask is a mask): both signs and zero occur, and two members of one shape get
    different operands."""
    m = BC.loss("sac_critic", 128, 128)
    a, _ = BC.member_operands("pair", m, 0)
    b, _ = BC.member_operands("pair", m, 10)
    for k in ("h1", "h2"):
        assert bool((a[k] > 0).any()) and bool((a[k] < 0).any()) and bool((a[k] == 0).any())
    assert not torch.equal(a["W2"], b["W2"]) and not torch.equal(a["dOut"], b["dOut"])
    ties = a["lo"]["q"][0] == a["lo"]["q"][1]
    pol, _ = BC.member_operands("pair", BC.loss("sac_policy", 128, 128), 0)
    assert bool(ties.any()) and set((pol["dOut"] * 128).unique().tolist()) == {-1.0, -0.5, 0.0}
