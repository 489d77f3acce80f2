"""The case table of ens_train_cases.py reaches every launch edge of the PETS ensemble training kernels -- proven on the host from
the constants and the bodies of parts_A / parts_B parsed out of csrc/ens_train_kernels.hip, csrc/ens_train_big_kernels.hip and the
csrc/ens_model.hpp they share, so that a retuned constant fails here instead of moving a case of test_ens_train_paths_gpu.py off its edge unnoticed --, its
restatement is PtModel's forward with MPC.train's loss, every operand kind reaches its regime, the f32 restatement stays inside
CAP, and rule 1 catches a kernel that is wrong in the ways of ens_train_cases.MUTATIONS."""
import os
import re

import pytest
import torch

import ens_train_cases as EC

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "recovery_rl_amd", "csrc")


def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _const(name, text):
    found = re.findall(r"constexpr\s+int\s+(?:\w+\s*=\s*[\w /*+-]+,\s*)*%s\s*=\s*(\d+)\s*[,;]" % name, text)
    assert len(found) == 1, "%s: found %r in the source" % (name, found)
    return int(found[0])


def _body(name, text):
    m = re.search(r"inline int %s\(long long rows_pad, int E\) \{\n(.*?)\n\}" % name, text, re.S)
    assert m, name
    return [line.split("//")[0].strip() for line in m.group(1).splitlines()]


# ---- the restatement is the sources' ------------------------------------------------------------------------------------------
def test_the_restated_constants_are_the_sources():
    small, big, model = _src("ens_train_kernels.hip"), _src("ens_train_big_kernels.hip"), _src("ens_model.hpp")
    got = dict(kH=_const("kH", model), kB=_const("kB", small), kR=_const("kR", small), kRbig=_const("kR", big),
               kGB=_const("kGB", big), kMaxP=_const("kMaxP", big), kMaxQ=_const("kMaxQ", big), kPartA=_const("kPartA", big))
    # one width for both files: the header's, and neither states a model constant of its own
    for text in (small, big):
        assert '#include "ens_model.hpp"' in text and "using namespace rrl_ens;" in text
        assert not re.search(r"constexpr\s+\w+\s[^;]*\b(kH|kDin|kDout|kMaxNets|kLogvarReg)\s*=", text)
    assert "constexpr int kHalves = kB / kR;" in small
    got["kHalves"] = got["kB"] // got["kR"]
    # one limit, in the check both entries call
    assert [x for x in re.findall(r"n_nets (?:>|<=) (\w+)", small + big + model) if x != "0"] == ["kMaxNets"]
    assert "if (!desc_complete(m, true)) return RRL_EINVAL;" in small and "if (!desc_complete(m, false)) return RRL_EINVAL;" in big
    got["max_nets"] = _const("kMaxNets", model)
    assert _body("parts_A", big) == ["long long tiles = rows_pad / kR;", "long long want = 256 / (E > 0 ? E : 1);",
                                     "if (want < 1) want = 1;", "long long P = tiles < want ? tiles : want;",
                                     "return int(P > kMaxP ? kMaxP : P);"]
    assert _body("parts_B", big) == ["long long groups = rows_pad / kGB;", "long long want = 256 / (2 * (E > 0 ? E : 1));",
                                     "if (want < 1) want = 1;", "long long Q = groups < want ? groups : want;",
                                     "return int(Q > kMaxQ ? kMaxQ : Q);"]
    got["wish"] = 256
    m = re.search(r"const long long n_small = \(long long\)E \* (\w+);", big)
    assert m.group(1) == "kOffLv" and "const int e = int(j / kOffLv), off = int(j % kOffLv);" in big
    assert "kOffLv = kOffB3 + kDout," in big
    got["small_total"] = _const("kOffB3", big) + _const("kDout", model)
    m = re.search(r"hipLaunchKernelGGL\(ens_big_reduce_kernel, dim3\((\d+)\), dim3\((\d+)\), 0, st, g, loss_out\);", big)
    got["reduce_grid"], got["reduce_block"] = int(m.group(1)), int(m.group(2))
    assert got == EC.CONSTANTS
    assert (EC.H, EC.SMALL_B, EC.SMALL_R, EC.HALVES, EC.MAX_NETS, EC.TILE, EC.GROUP, EC.MAX_P, EC.MAX_Q, EC.PART_A, EC.WISH,
            EC.SMALL_TOTAL, EC.REDUCE_THREADS) == (
        got["kH"], got["kB"], got["kR"], got["kHalves"], got["max_nets"], got["kRbig"], got["kGB"], got["kMaxP"], got["kMaxQ"],
        got["kPartA"], got["wish"], got["small_total"], got["reduce_grid"] * got["reduce_block"])
    # the index arithmetic and the sizes launch_facts() restates
    for line in ("const int e = blockIdx.x / kHalves, half = blockIdx.x % kHalves, tid = threadIdx.x;",
                 "const float live = half * kR + r < nb ? 1.f : 0.f;", "live, nb * 2);",       # nll's live and n2
                 "long long rrl_ens_scratch_floats(int n_nets) { return (long long)n_nets * kHalves * 3 * kR * kH + 64; }",
                 "return d_in == kDin && hidden == kH && d_out == kDout && batch >= 1 && batch <= kB;",
                 "hipLaunchKernelGGL(ens_logvar_grad_kernel, dim3(1), dim3(64), 0, st,",
                 "} else if (loss_out && k - 4 < n_nets) {"):
        assert line in small, line
    for line in ("inline long long rows_padded(long long batch) { return (batch + kR - 1) / kR * kR; }",
                 "for (long long tile = p; tile < n_tiles; tile += g.P) {", "const long long n_tiles = g.rows_pad / kR;",
                 "const long long groups = g.rows_pad / kGB;",
                 "const long long g_lo = groups * q / g.Q, g_hi = groups * (q + 1) / g.Q;",
                 "const float live = row0 + r < g.nb ? 1.f : 0.f;", "live, g.nb * 2);", "const long long n_big = 2LL * E * kH * kH;",
                 "const long long total = n_big + n_small + 4 + E;",
                 "for (long long i = blockIdx.x * 256LL + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {",
                 "return 6LL * n_nets * rp * kH + (long long)n_nets * parts_A(rp, n_nets) * kPartA +",
                 "2LL * n_nets * parts_B(rp, n_nets) * kH * kH;",
                 "hipLaunchKernelGGL(ens_big_fwd_bwd_kernel, dim3(E * g.P), dim3(kThreadsA), kLdsBytesA, st, g);",
                 "hipLaunchKernelGGL(ens_big_wgrad_kernel, dim3(2 * E * g.Q), dim3(kThreadsB), kLdsBytesB, st, g);"):
        assert line in big, line
    # the 64 threads of ens_logvar_grad_kernel: 4 bound sums + one loss per member
    assert 4 + got["max_nets"] == 64
    # the mean over the real rows and the two dims, F.softplus's threshold and the +-0.01 of the bound gradients: stated once,
    # in the header, and used by both files
    assert "const float scale = live / float(n2);" in model and "constexpr float kLogvarReg = 0.01f;" in model
    assert "return x > 20.f ? x : log1pf(expf(x));" in model and "return x > 20.f ? 1.f : sigm(x);" in model
    for text in (small, big):
        assert "const NllTerm t = nll(" in text and "log1pf(" not in text and "softplus(" not in text
        assert "= kLogvarReg + s;" in text and "= -kLogvarReg + s;" in text and "0.01f" not in text


def test_launch_facts_on_shapes_counted_by_hand():
    f = EC.launch_facts(5, 3300)["big"]
    assert (f["rows_pad"], f["tiles"], f["groups"], f["P"], f["Q"]) == (3328, 52, 104, 51, 25)
    assert f["walks"] == [2] + [1] * 50 and f["chunk_sizes"] == [4, 5] and f["chunks"][0] == (0, 4) and f["chunks"][-1] == (99, 104)
    assert f["last_tile_live"] == 3300 - 51 * 64
    f = EC.launch_facts(1, 4161)["big"]
    assert (f["rows_pad"], f["tiles"], f["groups"], f["wish_P"], f["wish_Q"], f["P"], f["Q"]) == (4224, 66, 132, 66, 128, 64, 32)
    assert f["walks"] == [2, 2] + [1] * 62 and f["chunk_sizes"] == [4, 5] and f["last_tile_live"] == 1
    f = EC.launch_facts(60, 300)["big"]
    assert (f["tiles"], f["P"], f["Q"], f["walks"]) == (5, 4, 2, [2, 1, 1, 1]) and f["reduce_total"] == 4800000 + 60 * 2204 + 64
    assert f["reduce_trips"] == 38 and f["scratch"] == 6 * 60 * 320 * 200 + 60 * 4 * 2304 + 2 * 60 * 2 * 40000
    f = EC.launch_facts(5, 17)
    assert f["small"]["live"] == [16, 1] and f["small"]["workgroups"] == 10 and f["small"]["scratch"] == 96064
    assert f["big"]["P"] == 1 and f["big"]["Q"] == 2 and f["big"]["chunks"] == [(0, 1), (1, 2)]
    assert EC.launch_facts(5, 16)["small"]["live"] == [16, 0] and EC.launch_facts(5, 1)["small"]["live"] == [1, 0]
    assert EC.launch_facts(5, 33)["small"] is None and EC.launch_facts(61, 32) == dict(small=None, big=None)
    assert EC.launch_facts(5, 0) == dict(small=None, big=None)


# ---- the table reaches every edge ---------------------------------------------------------------------------------------------
_small = lambda pred: lambda c, f: c.entry == "small" and pred(c, f)
_big = lambda pred: lambda c, f: c.entry == "big" and pred(c, f)
EDGES = {
    "small: one row": _small(lambda c, f: f["live"] == [1, 0]),
    "small: the second half all dead, the first ragged": _small(lambda c, f: f["live"] == [15, 0]),
    "small: the second half all dead, the first full": _small(lambda c, f: f["live"] == [16, 0]),
    "small: the second half holds one live row": _small(lambda c, f: f["live"] == [16, 1] and c.E == 5),
    "small: the second half ragged": _small(lambda c, f: f["live"] == [16, 15]),
    "small: the full batch": _small(lambda c, f: f["live"] == [16, 16] and c.E == 5),
    "small: one member": _small(lambda c, f: c.E == 1 and f["workgroups"] == 2),
    "small: 60 members": _small(lambda c, f: c.E == EC.MAX_NETS and c.batch == EC.SMALL_B),
    "big: one row": _big(lambda c, f: c.batch == 1 and f["tiles"] == 1),
    "big: the second tile holds one live row": _big(lambda c, f: f["tiles"] == 2 and f["last_tile_live"] == 1 and f["P"] == 2),
    "big: P = tiles, Q = groups / 2": _big(lambda c, f: f["P"] == f["tiles"] < EC.WISH // c.E and 2 * f["Q"] == f["groups"]),
    "big: P below the tiles, no cap: two tiles next to one": _big(lambda c, f: f["P"] == 51 < f["tiles"] and set(f["walks"]) == {1, 2}),
    "big: Q = 25, uneven chunks": _big(lambda c, f: f["Q"] == 25 and len(f["chunk_sizes"]) == 2),
    "big: both caps cut a larger wish, two tiles next to one": _big(
        lambda c, f: f["wish_P"] > f["P"] == EC.MAX_P and f["wish_Q"] > f["Q"] == EC.MAX_Q and set(f["walks"]) == {1, 2}),
    "big: both caps cut, Q's wish stems from 256 / (2 E)": _big(
        lambda c, f: f["wish_P"] > f["P"] == EC.MAX_P and f["groups"] > f["wish_Q"] > f["Q"] == EC.MAX_Q and c.E == 3),
    "big: both caps cut a wish that stems from the rows": _big(
        lambda c, f: f["tiles"] == f["wish_P"] > f["P"] == EC.MAX_P and f["wish_Q"] > f["Q"] == EC.MAX_Q and c.E == 1),
    "big: both caps met exactly, nothing cut": _big(lambda c, f: f["wish_P"] == f["P"] == EC.MAX_P and f["wish_Q"] == f["Q"] == EC.MAX_Q),
    "big: capped, chunks of 4 and 5 groups": _big(lambda c, f: f["Q"] == EC.MAX_Q and f["chunk_sizes"] == [4, 5]),
    "big: capped, a last tile with one live row": _big(lambda c, f: f["P"] == EC.MAX_P and f["last_tile_live"] == 1),
    "big: 60 members, P = 4 below 5 tiles, Q = 2": _big(lambda c, f: c.E == EC.MAX_NETS and f["P"] == 4 and f["tiles"] == 5 and f["Q"] == 2),
    "big: the reduce loop runs dozens of trips": _big(lambda c, f: f["reduce_trips"] > 30),
    "big: the size both entries accept": _big(lambda c, f: EC.launch_facts(c.E, c.batch)["small"] is not None and c.batch == EC.SMALL_B),
    "big: one member": _big(lambda c, f: c.E == 1),
}


def test_every_edge_has_a_plain_case():
    plain = [c for c in EC.CASES if c.kind == "plain"]
    hits = {edge: [c.name for c in plain if pred(c, EC.case_facts(c))] for edge, pred in EDGES.items()}
    assert not [e for e, names in hits.items() if not names], [e for e, names in hits.items() if not names]
    for c in EC.CASES:
        assert EC.case_facts(c) is not None, c.name                       # the entry accepts the case
        assert c.E * EC.case_facts(c).get("rows_pad", 32) <= 60 * 320     # the shapes stay small
    # the issue's shapes, all of them
    small = {(c.E, c.batch) for c in plain if c.entry == "small"}
    assert small >= {(5, b) for b in (1, 15, 16, 17, 31, 32)} | {(1, 17), (60, 32)}
    assert {(c.E, c.batch) for c in plain if c.entry == "big"} >= {(5, 1), (5, 65), (7, 1100), (5, 3300), (1, 4161), (3, 4097),
                                                                   (60, 300), (5, 32)}
    # the size both entries accept runs the same operands on both
    a, b = EC.operands("small-E5-b32-plain-contig"), EC.operands("big-E5-b32-plain-contig")
    assert all(torch.equal(a[k], b[k]) or k in ("train_in", "train_targ") for k in a)


def test_the_kinds_and_layouts_run_where_they_must():
    capped = lambda c: c.entry == "big" and EC.case_facts(c)["P"] == EC.MAX_P and EC.case_facts(c)["Q"] == EC.MAX_Q
    have = lambda kind, pred: any(c.kind == kind and pred(c) for c in EC.CASES)
    for kind in ("thresh", "wide"):
        assert have(kind, capped), kind
        assert have(kind, lambda c: (c.entry, c.E, c.batch) == ("big", 5, 65)), kind
        assert have(kind, lambda c: c.entry == "small" and c.batch == 17), kind
        assert have(kind, lambda c: c.entry == "small" and c.batch == 32), kind
    for kind in ("upper", "lower"):
        assert have(kind, lambda c: c.entry == "small") and have(kind, lambda c: c.entry == "big"), kind
    for entry in ("small", "big"):
        for strided in (False, True):
            assert any(c.entry == entry and c.strided == strided for c in EC.CASES)
    for c in EC.CASES:
        p = EC.operands(c.name)
        n = EC.N_ROWS
        assert p["idx"].shape == (c.E, c.batch) and int(p["idx"].min()) >= 0 and int(p["idx"].max()) < n     # no live index on it
        assert bool((p["train_in"][n] != p["train_in"][n]).all()) and bool((p["train_targ"][n] != p["train_targ"][n]).all())
        assert bool(torch.isfinite(p["train_in"][:n]).all()) and bool(torch.isfinite(p["train_targ"][:n]).all())
        if c.strided:                                                     # the poison is in range: it points to the NaN row
            assert p["idx"].stride(0) == c.batch + EC.TABLE_EXTRA and bool((p["table"][:, c.batch:] == n).all())
            assert int(p["table"].max()) == n == p["train_in"].shape[0] - 1
        else:
            assert p["idx"].is_contiguous()
        assert float(p["max_logvar"][0, 0]) != float(p["max_logvar"][0, 1]) and float(p["min_logvar"][0, 0]) != float(p["min_logvar"][0, 1])


@pytest.mark.parametrize("name", EC.names())
def test_every_kind_reaches_its_regime(name):
    facts = EC.kind_facts(name)
    assert len(facts) >= 2 and all(facts.values()), facts


# ---- the restatement is the module's ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["small-E5-b17-plain-contig", "small-E5-b32-lower-strided", "big-E5-b65-thresh-strided",
                                  "big-E5-b65-wide-contig", "small-E5-b17-upper-contig"])
def test_the_f32_restatement_is_ptmodel_forward_with_the_training_loss(name):
    """PtModel.forward(ret_logvar=True) on the host with the loss of MPC._train_step minus the decay terms, by .backward():
    the same f32 operations as restate(dtype=float32), so the same bits."""
    p = EC.operands(name)
    m = EC.model_of(p)
    loss = 0.01 * (m.max_logvar.sum() - m.min_logvar.sum())
    mean, logvar = m(p["train_in"][p["idx"]], ret_logvar=True)
    tl = ((mean - p["train_targ"][p["idx"]]) ** 2) * torch.exp(-logvar) + logvar
    nll = tl.mean(-1).mean(-1)
    (loss + nll.sum()).backward()
    r32 = EC.reference(name, torch.float32)
    assert torch.equal(nll.detach(), r32.loss)
    for k in EC.PARAMS[:8]:
        assert torch.equal(getattr(m, k).grad, r32.grads[k]), k
    # the bounds: autograd adds their three contributions in another order under .backward() -- two f32 evaluations, each
    # within the basis of rule 1 of float64, so at most twice that apart
    r64 = EC.reference(name)
    for k in EC.BOUNDS:
        basis = float(EC.basis_of(r64.grads[k].reshape(1, -1), r32.grads[k].double().reshape(1, -1)))
        assert float((getattr(m, k).grad.double() - r32.grads[k].double()).abs().max()) <= 2 * basis, k


def test_the_parameter_names_are_the_trainers():
    from recovery_rl_amd.ensemble_train import PARAMS
    assert EC.PARAMS == PARAMS


# ---- the f32 restatement stays inside CAP ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", EC.names())
def test_the_f32_restatement_lies_within_the_cap(name):
    ratios = EC.f32_cap_ratio(name)
    assert set(ratios) == set(EC.QUANTITIES)
    assert max(ratios.values()) * 2.0 ** -23 <= EC.CAP, ratios
    assert EC.FACTOR * EC.CAP < 1.6e-5                                 # below every bar of test_ens_train_gpu.py (2e-5 .. 3e-4)


def test_the_restatements_pass_their_own_rule():
    for name in EC.names():
        for dtype in (torch.float64, torch.float32):
            assert not EC.compare(name, EC.reference(name, dtype)), (name, dtype)


# ---- rule 1 catches a kernel that is wrong --------------------------------------------------------------------------------------
# mutation -> the named cases that catch it (each by a ratio of at least 4 x FACTOR: no near miss), and the kernel line whose
# breaking it restates
B32, B1100 = "small-E5-b32-plain-contig", "big-E7-b1100-plain-strided"
CAUGHT_BY = {
    "mean_over_padded": ("small-E5-b17-plain-contig", "small-E5-b1-plain-strided", "big-E5-b65-plain-contig",
                         "big-E1-b4161-plain-strided"),                                # live / float(nb * 2) -> / 64
    "k192_fwd1": (B32, B1100), "k192_fwd2": (B32, B1100), "k192_fwd3": (B32, B1100),   # chunks = 13 -> 12, kH -> 192
    "j192_bwd2": (B32, B1100), "j192_bwd1": (B32, B1100),
    "k192_wgrad1": (B32, B1100), "k192_wgrad2": (B32, B1100),                          # mtiles = 13 -> 12; tile 12 of kernel B
    "second_half_dropped": ("small-E5-b17-plain-contig", B32, "small-E60-b32-plain-strided"),     # Adam's g + g2 -> g
    "last_group_dropped": ("big-E5-b1-plain-strided", "big-E5-b3300-plain-contig", "big-E1-b4161-plain-strided",
                           "big-E60-b300-plain-strided"),                              # grp < g_hi -> grp + 1 < g_hi
    "softplus_grad_zero": ("small-E5-b32-lower-strided", "small-E5-b17-thresh-contig", "big-E5-b65-thresh-strided",
                           "big-E5-b3300-lower-contig"),                               # x > 20.f ? 1.f -> 0.f
    "dmin_dmax_swapped": (B32, "big-E60-b300-plain-strided"),                          # part * 4 + k <-> part * 4 + 2 + k
    "no_bound_001": (B32, "small-E5-b32-lower-strided", B1100, "big-E7-b1100-upper-strided"),     # 0.01f + s -> s
    "mu_sigma_rolled": (B32, "small-E5-b17-wide-strided", B1100),                      # m.mu[k] -> m.mu[(k + 3) % 4]
    "w3_of_member0": ("small-E60-b32-plain-strided", B32, "big-E3-b4097-plain-contig"),           # W3 without e * kH * kDout
}


@pytest.mark.parametrize("mutation", EC.MUTATIONS)
def test_rule_one_catches_every_mutation_on_its_named_cases(mutation):
    assert set(CAUGHT_BY) == set(EC.MUTATIONS)
    for name in CAUGHT_BY[mutation]:
        wrong = EC.restate(EC.operands(name), EC.BY_NAME[name].entry, dtype=torch.float32, mutation=mutation)
        report = []
        bad = EC.compare(name, wrong, report)
        assert bad, (mutation, name, "not caught")
        assert max(r[3] for r in report) >= 4 * EC.FACTOR, (mutation, name, "caught by a near miss only", report)


def test_a_mutation_is_no_mutation_where_its_code_does_not_run():
    """One member: member 0's W3 is its own.  The large-batch entry has no second half, the small one no split-K chunks."""
    for mutation, name in (("w3_of_member0", "small-E1-b17-plain-contig"), ("second_half_dropped", "big-E5-b65-plain-contig"),
                           ("last_group_dropped", "small-E5-b32-plain-contig"), ("mean_over_padded", "small-E5-b32-plain-contig")):
        wrong = EC.restate(EC.operands(name), EC.BY_NAME[name].entry, dtype=torch.float32, mutation=mutation)
        assert not EC.compare(name, wrong), (mutation, name)
