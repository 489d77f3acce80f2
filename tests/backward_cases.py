"""Cases, float64 reference, descriptors and a restatement of the host dispatch for the stack backward family
(csrc/mlp_kernels.hip: rrl_mlp_head_backward_multi, rrl_mlp_hidden_backward_multi, rrl_mlp_backward_pair_multi,
rrl_mlp_input_backward_multi and the packed forms of the first three), shared by test_backward_paths_cpu.py and
test_backward_paths_gpu.py.

The library does not say which kernel it launched.  backward_path() restates the host's decisions (hidden_args' FAST geometry,
build_hidden_group, wants_fold, pack_panel, pack_block, hidden_blocks, launch_head_group, build_pair_jobs and the two paired
entries) with their constants as literals; test_backward_paths_cpu.py parses the constants out of the sources and proves that
the case table reaches every label and every ragged condition.

A member of a case is EXACT or ROUNDED (exact(m)), a case exact when all its members are.

Exact: every operand is an integer in [-r, r] (r = 2, or 1 where the bound below asks for it) and dOut is a plain integer
tensor, or SAC_CRITIC with v2 = 0 (dOut = 2 (q - r) / B) or SAC_POLICY (dOut = -1/B, -0.5/B, 0; ties included) at a power of two
B: every product and every partial sum is then an integer multiple of one dyadic step (1, 2/B, 0.5/B) and stays below 2^24 of
them (closed_bound(): test_stack_backward_gpu.problem's bound for the entry's own outputs, dout, range and B; and, from the
float64 reference, the sum of the magnitudes of every output's terms), so f32 holds it exactly in whatever order a kernel
adds, and the comparison with float64 is torch.equal.

Rounded (the sigmoid kinds, the two policy heads, B no power of two): dOut is the f32 tensor rrl_loss_dout writes for the
same rrl_loss_t -- compared with float64 in test_update_pieces_gpu.py and shown there to be the head backward's dOut bit for
bit; h2, h1, W3, W2, W1 and x stay small integers.  The reference is the float64 chain from that f32 dOut, and the tolerance
is derived, not measured.  An output element is a sum of products evaluated in f32 by additions and fused multiply-adds in
some order; whatever the order, a term passes through at most n roundings, n the additions along the longest chain into
the element, each of relative size u = 2^-24, so the error is at most gamma_n A with gamma_n = n u / (1 - n u) and A the
sum of the magnitudes of the terms: the same chain evaluated on the absolute values of all operands with the relu masks
kept.  n: dout for dh2, dout + B for dW3 and db3, dout + H for dh1, dout + B for dW2 and db2, dout + 2 H for dx and its
partials, dout + H + B for dW1, db1 and their partials.  The tolerance is n 2^-23 A per element: twice gamma_n up to
n u < 1e-3, which test_backward_paths_cpu.py asserts for every case (so the bound cannot grow until it hides something).  A
structural error -- a wrong row, column, head or mask -- is of the order of A itself.

Whatever include/rrl_hip.h promises bit for bit is torch.equal in both classes: n members in one launch against n launches
of one, the paired launch against head launch + hidden launch, every seed of a packed launch against its solo launch, folded
dx partials against ((p0 + p1) + p2) + p3 of the tile partials."""
import collections
import ctypes as C
import functools
import os

import torch

from stack_cases import DEAD_ROWS, LDX_STRIDED, SENT, guard_of, guarded, ints, rows_then_nan

RRL_OK, RRL_EINVAL, RRL_ERANGE = 0, -1, -3

# ---- the host dispatch's constants, as literals (test_backward_paths_cpu.py compares them with the sources) -----------------
CONSTANTS = dict(kTile=16, kPanel=128, kPairPanel=64, kPairDsh=1024, kBlkPanel=32, kCols=16, kSlices=16, kUnroll=16,
                 kMaxGroup=4, kMaxSeeds=16, RRL_PACK_PAIR_MAX_SEEDS=2, RRL_PACK_PAIR_BLOCK_MAX_SEEDS=8, tail_floats=1024 * 4 - 6 * 16)
TILE, PANEL, PAIR_PANEL, PAIR_DSH, BLK_PANEL = 16, 128, 64, 1024, 32
COLS, CHUNK, MAX_GROUP, MAX_SEEDS, TAIL_FLOATS = 16, 16 * 16, 4, 16, 4000     # CHUNK = kSlices kUnroll rows of the head backward
PACK_PANEL_BODY = "return S >= 3 ? 32 : (S >= 2 ? 64 : kPanel);"
PACK_BLOCK_BODY = "return S >= 3 ? 12 : 0;"


def pack_panel(S):
    return 32 if S >= 3 else (64 if S >= 2 else PANEL)


def pack_block(S):
    return 12 if S >= 3 else 0


def _atoi(text):
    """C's atoi: optional blanks and sign, then the leading digits; nothing to convert: 0."""
    s, sign, v = text.lstrip(" \t\n\v\f\r"), 1, 0
    if s[:1] in ("+", "-"):
        sign, s = (-1 if s[0] == "-" else 1), s[1:]
    for ch in s:
        if not ch.isdigit():
            break
        v = 10 * v + int(ch)
    return sign * v


def env_int(name, fallback, env=None):
    e = (os.environ if env is None else env).get(name)
    return _atoi(e) if e is not None else fallback


# ---- members ----------------------------------------------------------------------------------------------------------------
# One stack per member.  kind: "plain" (dOut is a tensor) or a loss kind.  first: None or which outputs of the fused first
# layer are asked for ("w": first_part, "x": dx_part, "wx").  dW2 / dh1 / dh2 / dW3: the output is asked for.  link: the
# paired entries' heads[k].dh2 == hidden[k].dh2.  misalign: an operand whose base is 4 bytes past a 16-byte boundary.
# need_w / need_x: rrl_input_bwd_t's (dW1, db1) / dx.
Mem = collections.namedtuple("Mem", "G B H dout kind din first dW2 dh1 fold dh2 dW3 link strided misalign need_w need_x",
                             defaults=(1, "plain", 2, None, True, True, False, True, True, True, False, None, True, True))
KINDS = ("sac_critic", "sac_policy", "qrisk_critic", "qrisk_policy", "gauss", "stoch", "dgd_qrisk")     # RRL_LOSS_* order
KIND_DOUT = dict(sac_critic=1, sac_policy=1, qrisk_critic=1, qrisk_policy=1, dgd_qrisk=1, gauss=4, stoch=2)
ALPHA, GAMMA, GAMMA_SAFE, NU = 0.2, 0.99, 0.65, 3.5


def plain(G, B, H, dout=1, **kw):
    return Mem(G, B, H, dout, "plain", **kw)


def loss(kind, B, H, **kw):
    dout = KIND_DOUT[kind]
    return Mem(2 if dout == 1 else 1, B, H, dout, kind, **kw)


def pow2(n):
    return n > 0 and n & (n - 1) == 0


def exact(m):
    return m.kind == "plain" or (m.kind in ("sac_critic", "sac_policy") and pow2(m.B))


def case_exact(case):
    return all(exact(m) for g in case.seeds for m in g)


# ---- the dispatch, restated ---------------------------------------------------------------------------------------------------
class Refused(Exception):
    """The entry returns this code before anything is launched."""

    def __init__(self, rc):
        Exception.__init__(self, rc)
        self.rc = rc


def hidden_fast(m):
    """hidden_args: full tiles, K a panel multiple for both products, 16-byte aligned dh2, h1, W2."""
    return (m.H % TILE == 0 and m.B % TILE == 0 and m.H % PANEL == 0 and m.B % PANEL == 0
            and m.misalign not in ("dh2", "h1", "W2"))


def check_hidden_group(ms):
    """build_hidden_group's refusals."""
    if not 0 < len(ms) <= MAX_GROUP:
        raise Refused(RRL_EINVAL)
    for m in ms:
        if m.first and (not 0 < m.din <= 4):
            raise Refused(RRL_EINVAL)
        if not m.dh1 and not m.first:
            raise Refused(RRL_EINVAL)
        if m.first and not hidden_fast(m):
            raise Refused(RRL_ERANGE)


def check_head_group(ms):
    """build_head_group / head_args' refusals."""
    if not 0 < len(ms) <= MAX_GROUP:
        raise Refused(RRL_EINVAL)
    for m in ms:
        if m.B > 1024 or not 0 < m.dout <= 4:
            raise Refused(RRL_ERANGE)
        if m.kind != "plain" and (m.G, m.dout) != ((2, 1) if KIND_DOUT[m.kind] == 1 else (1, KIND_DOUT[m.kind])):
            raise Refused(RRL_EINVAL)


def wants_fold(ms):
    return any(m.first and "x" in m.first and m.fold for m in ms)


def hidden_blocks(ms, wm=1, wn=2):
    bm, bn = 32 * wm, 32 * wn
    return all(hidden_fast(m) and m.H % bm == 0 and m.H % bn == 0 and m.B % bm == 0 and m.H % BLK_PANEL == 0
               and m.B % BLK_PANEL == 0 for m in ms)


# the clauses of build_pair_jobs' `pair =` condition, in the source's order and spelling
PAIR_CLAUSES = ("my != 0", "(dout == 0 || dout == my)", "h.dout == my", "h.dh2", "h.dh2 == d.dh2", "h.G == d.G", "h.B == d.B",
                "h.H == d.H", "h.B * my <= kPairDsh", "h.H <= 256", "hd.fast[k]", "(h.H % kPairPanel) == 0",
                "(h.B % kPairPanel) == 0", "(nn_tiles % 4) == 0", "(hd.tn_tiles[k] % 4) == 0",
                "(reinterpret_cast<uintptr_t>(h.h2) & 15) == 0", "(reinterpret_cast<uintptr_t>(h.W3) & 15) == 0")
# clauses that the table fails one at a time
SOLE_CLAUSES = ("my != 0", "(dout == 0 || dout == my)", "h.dh2 == d.dh2", "h.B * my <= kPairDsh", "hd.fast[k]",
                "(reinterpret_cast<uintptr_t>(h.h2) & 15) == 0", "(reinterpret_cast<uintptr_t>(h.W3) & 15) == 0")
# clauses that follow from hd.fast[k] (H and B multiples of 128: test_backward_paths_cpu.py goes through the sizes); the table
# fails each of them together with it
IMPLIED_BY_FAST = ("(h.H % kPairPanel) == 0", "(h.B % kPairPanel) == 0", "(nn_tiles % 4) == 0", "(hd.tn_tiles[k] % 4) == 0")
# clauses no case of this table can fail alone, and why
UNREACHED_CLAUSES = {
    "h.dout == my": "head_args returns RRL_EINVAL for a loss kind on another dout before the condition is evaluated",
    "h.dh2": "a null heads[k].dh2 differs from hidden[k].dh2, which build_hidden_group requires: `h.dh2 == d.dh2` fails with it",
    "h.G == d.G": "a member of this table is ONE stack: its two descriptors share G, B and H",
    "h.B == d.B": "a member of this table is ONE stack: its two descriptors share G, B and H",
    "h.H == d.H": "a member of this table is ONE stack: its two descriptors share G, B and H",
    "h.H <= 256": "every case of this table has H <= 256 (the next FAST width is 384)",
}


def pair_clauses(m, dout_before):
    """The value of every clause of the `pair =` condition for member m, `dout_before` the launch's dout so far (0: none)."""
    my = 0 if m.kind == "plain" else KIND_DOUT[m.kind]
    tx, ny = -(-m.H // TILE), -(-m.B // TILE)
    tn_tiles = tx * tx if m.dW2 else 0
    return dict(zip(PAIR_CLAUSES, (
        my != 0, dout_before in (0, my), m.dout == my or my == 0, bool(m.dh2), bool(m.dh2) and m.link, True, True, True,
        m.B * my <= PAIR_DSH, m.H <= 256, hidden_fast(m), m.H % PAIR_PANEL == 0, m.B % PAIR_PANEL == 0, (tx * ny) % 4 == 0,
        tn_tiles % 4 == 0, m.misalign != "h2", m.misalign != "W3")))


def pairable(ms, blocks=False):
    """build_pair_jobs -> (pair, dout)."""
    check_head_group(ms)
    check_hidden_group(ms)
    dout = 0
    for m in ms:
        if not all(pair_clauses(m, dout).values()):
            return False, 0
        dout = KIND_DOUT[m.kind]
    if blocks and not hidden_blocks(ms):
        return False, dout
    return True, dout


def hidden_label(seeds):
    S = len(seeds)
    for g in seeds:
        check_hidden_group(g)
    if S == 1:
        (ms,) = seeds
        if wants_fold(ms):
            raise Refused(RRL_ERANGE)                  # one tile per workgroup: nothing to fold with
        fast = [hidden_fast(m) for m in ms]
        if any(m.first for m in ms):
            return "tile-fast-first"
        return "tile-fast" if all(fast) else ("tile-mixed" if any(fast) else "tile-ragged")
    if pack_block(S) and all(hidden_blocks(g) for g in seeds):
        return "pack-block"
    if any(wants_fold(g) for g in seeds):
        raise Refused(RRL_ERANGE)
    return "pack-panel%d" % pack_panel(S)


def head_label(seeds):
    for g in seeds:
        check_head_group(g)
    if len(seeds) > 1:
        return "head-pack"
    (ms,) = seeds
    if len(ms) == 1 and ms[0].kind != "plain":
        return "loss-kernel-" + ms[0].kind
    return "head-group"


def pair_label(seeds, env=None):
    S = len(seeds)
    if S == 1:
        (ms,) = seeds
        pair, dout = pairable(ms)
        if pair:
            return "pair<%d>" % dout
        if wants_fold(ms):
            raise Refused(RRL_ERANGE)
        return "pair-fallback"
    blocks = S > env_int("RRL_PACK_PAIR_MAX_SEEDS", CONSTANTS["RRL_PACK_PAIR_MAX_SEEDS"], env)
    few = S <= env_int("RRL_PACK_PAIR_BLOCK_MAX_SEEDS", CONSTANTS["RRL_PACK_PAIR_BLOCK_MAX_SEEDS"], env)
    pair, dout = few, 0
    would = True                      # every seed qualifies for the paired block form, were the seeds few enough
    for g in seeds:
        ok, my = pairable(g, blocks)
        would = would and ok and dout in (0, my)
        pair = pair and ok and dout in (0, my)
        dout = my
    if pair:
        return ("pair-block-pack<%d>" if blocks else "pair-pack<%d>") % dout
    head_label(seeds)
    hidden_label(seeds)               # its refusals are the entry's
    return "pair-split" if (would and not few) else "pair-pack-fallback"


def backward_path(entry, seeds, env=None):
    """The label of the kernel(s) the host launches for `entry` ("head", "hidden", "pair", "input") on `seeds` (a tuple of
    groups of Mem: one group for the solo entry, S for the packed one); raises Refused(rc) where the host returns rc."""
    if not 0 < len(seeds) <= MAX_SEEDS:
        raise Refused(RRL_EINVAL)
    if entry == "hidden":
        return hidden_label(seeds)
    if entry == "head":
        return head_label(seeds)
    if entry == "pair":
        return pair_label(seeds, env)
    assert entry == "input" and len(seeds) == 1
    return "input-group"


HIDDEN_LABELS = ("tile-fast", "tile-ragged", "tile-mixed", "tile-fast-first", "pack-panel64", "pack-block", "pack-panel32")
HEAD_LABELS = tuple("loss-kernel-" + k for k in KINDS) + ("head-group", "head-pack")
PAIR_LABELS = ("pair<1>", "pair<2>", "pair<4>", "pair-fallback", "pair-pack<1>", "pair-pack<2>", "pair-pack<4>",
               "pair-block-pack<1>", "pair-block-pack<2>", "pair-block-pack<4>", "pair-split", "pair-pack-fallback")
LABELS = HIDDEN_LABELS + HEAD_LABELS + PAIR_LABELS + ("input-group",)
PAIRED_LABELS = tuple(l for l in PAIR_LABELS if "<" in l)            # one launch: heads[k].dh2 is not written

# ---- the case table ---------------------------------------------------------------------------------------------------------
# opts: refused = the return code the entry must give (nothing launched, nothing written)
Case = collections.namedtuple("Case", "name entry seeds opts")
WX = dict(first="wx", din=4)


def _hidden():
    out = []

    def add(name, *seeds, **opts):
        out.append(Case("hidden-" + name, "hidden", tuple(tuple(g) for g in seeds), opts))
    add("ragged-H48-B40-G2", [plain(2, 40, 48)])                           # no full tile in either direction
    add("ragged-H128-B64-G1", [plain(1, 64, 128, dout=4)])                 # full tiles, K = B is no panel multiple
    add("fast-H128-B256-G3", [plain(3, 256, 128)])
    add("fast-H256-B128-G2", [plain(2, 128, 256, dout=2)])                 # with the one above: a swapped B / H shows
    add("ragged-H256-B200-G1", [plain(1, 200, 256)])
    add("ragged-H40-B24-G2", [plain(2, 24, 40, dout=3)])                   # H itself no tile multiple
    # kMaxGroup members that differ in G, B and H: the grid is the largest job's, the others' surplus workgroups leave
    add("four-fast", [plain(2, 256, 128), plain(1, 128, 256), plain(3, 128, 128), plain(1, 256, 256)])
    add("four-mixed", [plain(1, 128, 256), plain(3, 40, 40), plain(2, 256, 128, dW2=False), plain(1, 64, 128)])
    add("nodW2-H128-B256", [plain(2, 256, 128, dW2=False)])                # the input gradient only
    add("nodW2-H48-B40", [plain(3, 40, 48, dW2=False)])
    add("first-w", [plain(2, 256, 128, first="w", din=4)])
    add("first-x-ldx7", [plain(1, 256, 128, first="x", din=2, strided=True)])
    add("first-wx-ldx7", [plain(3, 128, 256, strided=True, **WX)])
    add("first-wx-nodh1", [plain(2, 256, 128, first="wx", din=2, dh1=False)])
    add("first-x-nodh1-nodW2", [plain(2, 128, 128, first="x", din=4, dh1=False, dW2=False)])
    add("first-beside-ragged", [plain(2, 128, 128, **WX), plain(1, 40, 48)])
    add("fold-solo-refused", [plain(2, 128, 128, fold=True, **WX)], refused=RRL_ERANGE)
    # packed: seeds of different member counts
    add("S2-panel64", [plain(2, 256, 128), plain(1, 256, 128, first="wx", din=2)], [plain(3, 128, 256, dW2=False)])
    add("S2-panel64-ragged", [plain(2, 24, 40)], [plain(1, 64, 128), plain(2, 128, 128, **WX)])
    add("S3-block", [plain(2, 128, 128), plain(1, 256, 128)], [plain(1, 128, 256, strided=True, **WX)],
        [plain(3, 128, 128, dW2=False), plain(1, 256, 256), plain(2, 256, 128, first="x", din=2, dh1=False)])
    add("S3-panel32", [plain(2, 128, 128, **WX), plain(1, 256, 128)], [plain(1, 40, 48), plain(2, 24, 40)], [plain(3, 128, 128, dW2=False)])
    fold = [[plain(2, 128, 128, fold=True, **WX)], [plain(1, 256, 128, first="x", din=2, dh1=False, fold=True), plain(1, 128, 128)],
            [plain(2, 128, 256, fold=True, strided=True, **WX)], [plain(1, 128, 128, fold=True, first="wx", din=2, dW2=False)]]
    add("S3-block-fold", *fold[:3])
    add("S4-block-fold", *fold)
    add("S2-fold-refused", *fold[:2], refused=RRL_ERANGE)                  # the tile form cannot fold: S = 2 has no block form
    return out


def _head():
    out = []

    def add(name, *seeds, **opts):
        out.append(Case("head-" + name, "head", tuple(tuple(g) for g in seeds), opts))
    for i, (H, B) in enumerate((H, B) for H in (16, 40, 256) for B in (1, 17, 256, 257, 1024)):
        add("plain-H%d-B%d" % (H, B), [plain(1 + i % 3, B, H, dout=1 + i % 4)])
    for kind in KINDS:                                 # general h2 and W3; H = 40: the last column block is partial
        add("%s-H40-B256" % kind, [loss(kind, 256, 40)])
        add("%s-H40-B257" % kind, [loss(kind, 257, 40)])                   # one whole chunk of 256 rows, then one row
    add("sac_policy-H16-B1024", [loss("sac_policy", 1024, 16)])
    add("gauss-H256-B1024", [loss("gauss", 1024, 256)])                    # B dout = 4096 fills dsh: the scalars go through red[]
    for B in (1000, 1001, 1024):                       # tail_free: B dout <= 4000
        add("plain-dout4-H40-B%d" % B, [plain(2, B, 40, dout=4)])
    add("plain-nodh2", [plain(2, 257, 40, dout=3, dh2=False)])
    add("qrisk_critic-nodh2", [loss("qrisk_critic", 257, 40, dh2=False)])
    add("plain-nodW3", [plain(3, 17, 40, dout=2, dW3=False)])
    add("sac_policy-nodW3", [loss("sac_policy", 256, 40, dW3=False)])
    add("four-mixed", [loss("sac_critic", 256, 40), plain(3, 17, 16, dout=4), loss("gauss", 257, 40), loss("qrisk_policy", 1024, 256)])
    add("three-exact", [loss("sac_critic", 256, 40), loss("sac_policy", 128, 16, dW3=False), plain(1, 257, 256, dout=2, dh2=False)])
    add("S2-pack", [loss("sac_critic", 256, 40), plain(2, 257, 16, dout=4)], [loss("sac_policy", 128, 256)])
    add("S3-pack", [loss("stoch", 257, 40)], [plain(3, 1001, 40, dout=4), loss("sac_critic", 256, 16)], [loss("dgd_qrisk", 17, 256, dh2=False)])
    return out


def _pair():
    out = []

    def add(name, *seeds, **opts):
        out.append(Case("pair-" + name, "pair", tuple(tuple(g) for g in seeds), opts))
    for B, H, kind in ((128, 128, "sac_critic"), (256, 128, "sac_policy"), (128, 256, "sac_critic"), (384, 128, "sac_critic"),
                       (1024, 128, "sac_critic"), (256, 128, "qrisk_critic"), (128, 128, "qrisk_policy"), (128, 256, "dgd_qrisk"),
                       (1024, 128, "qrisk_critic"), (384, 128, "sac_policy")):
        add("%s-B%d-H%d" % (kind, B, H), [loss(kind, B, H)])               # B = 1024: kPairDsh exactly
    for B, H in ((256, 128), (512, 256)):                                  # B dout = kPairDsh at 512
        add("stoch-B%d-H%d" % (B, H), [loss("stoch", B, H)])
    for B, H in ((128, 256), (256, 128)):                                  # B dout = kPairDsh at 256
        add("gauss-B%d-H%d" % (B, H), [loss("gauss", B, H)])
    add("three-exact", [loss("sac_critic", 128, 128), loss("sac_policy", 256, 128, dW2=False), loss("sac_critic", 128, 256)])
    add("three-kinds", [loss("qrisk_critic", 128, 128), loss("sac_policy", 256, 128), loss("dgd_qrisk", 128, 256, dW3=False)])
    add("three-stoch", [loss("stoch", 128, 128), loss("stoch", 256, 128), loss("stoch", 128, 256)])
    add("sac_critic-first", [loss("sac_critic", 128, 128, **WX)])
    add("sac_critic-first-fold-ldx7", [loss("sac_critic", 128, 128, fold=True, strided=True, **WX)])
    add("sac_policy-first-x-fold-nodh1-nodW2", [loss("sac_policy", 256, 128, first="x", din=4, fold=True, dh1=False, dW2=False)])
    add("gauss-first-fold", [loss("gauss", 128, 256, first="wx", din=2, fold=True)])
    add("gauss-first", [loss("gauss", 256, 128, first="x", din=2)])
    add("stoch-first", [loss("stoch", 256, 128, first="wx", din=2)])
    # the two launches, each for another clause of the `pair =` condition
    add("fallback-B200", [loss("sac_critic", 200, 128)])
    add("fallback-H48", [loss("sac_critic", 128, 48)])
    add("fallback-H48-B40", [loss("sac_policy", 40, 48)])
    add("fallback-H40", [loss("sac_critic", 128, 40)])                     # the head backward's last column block is partial
    add("fallback-plain", [plain(2, 128, 128)])
    add("fallback-unlinked", [loss("sac_critic", 128, 128, link=False)])
    add("fallback-dout-mix", [loss("sac_critic", 128, 128), loss("gauss", 128, 128)])
    add("fallback-stoch-B1024", [loss("stoch", 1024, 128)])                # B dout = 2 kPairDsh
    add("fallback-misaligned-h1", [loss("sac_critic", 128, 128, misalign="h1")])
    add("fallback-misaligned-h2", [loss("sac_critic", 128, 128, misalign="h2")])
    add("fallback-misaligned-W3", [loss("sac_policy", 128, 128, misalign="W3")])
    add("fallback-fold-refused", [loss("sac_critic", 200, 128), loss("sac_critic", 128, 128, fold=True, **WX)], refused=RRL_ERANGE)
    # packed
    kinds = ("sac_critic", "sac_policy", "qrisk_critic", "sac_critic", "dgd_qrisk", "sac_policy", "qrisk_policy", "sac_critic",
             "sac_policy")
    add("S2-pack", [loss("sac_critic", 128, 128, **WX), loss("sac_policy", 256, 128, dW2=False)], [loss("qrisk_critic", 128, 256)])
    add("S2-pack-fold", [loss("sac_critic", 128, 128, fold=True, **WX)], [loss("sac_policy", 128, 256, first="x", din=4, fold=True, dh1=False)])
    add("S3-block", [loss("sac_critic", 128, 128, **WX), loss("sac_policy", 256, 128, dW2=False)], [loss("qrisk_critic", 128, 256)],
        [loss("sac_critic", 256, 256, fold=True, strided=True, **WX)])
    add("S3-block-exact", [loss("sac_critic", 128, 128)], [loss("sac_policy", 256, 128), loss("sac_critic", 128, 256)],
        [loss("sac_policy", 128, 128, first="x", din=4, fold=True, dh1=False, dW2=False)])
    add("S8-block", *[[loss(k, 128, 128 if s % 2 else 256)] for s, k in enumerate(kinds[:8])])
    add("S9-split", *[[loss(k, 128, 128 if s % 2 else 256)] for s, k in enumerate(kinds)])
    add("S9-split-exact", *[[loss(("sac_critic", "sac_policy")[s % 2], 256 if s % 3 else 128, 128)] for s in range(9)])
    for kind in ("stoch", "gauss"):
        add("S2-pack-" + kind, [loss(kind, 128, 128), loss(kind, 128, 256)], [loss(kind, 256, 128, first="wx", din=2)])
        add("S3-block-" + kind, [loss(kind, 128, 128)], [loss(kind, 256, 128, first="wx", din=2, fold=True)], [loss(kind, 128, 256)])
    add("S3-fallback", [loss("sac_critic", 128, 128)], [loss("sac_policy", 200, 128), loss("sac_critic", 128, 128)],
        [loss("sac_policy", 256, 128)])
    add("S3-fallback-H48", [loss("sac_critic", 128, 128), loss("sac_policy", 128, 48)], [loss("sac_critic", 256, 128)],
        [loss("sac_policy", 128, 128, **WX)])
    return out


def _input():
    out = []

    def add(name, *ms, **opts):
        out.append(Case("input-" + name, "input", (tuple(ms),), opts))
    add("w-only", plain(2, 5, 16, din=4, need_x=False))
    add("x-only", plain(1, 200, 40, din=2, need_w=False))
    add("both-B1-ldx7", plain(3, 1, 40, din=4, strided=True))
    add("both-B200-H16", plain(2, 200, 16, din=2))
    add("both-B5-H40-din3", plain(2, 5, 40, din=3, strided=True))
    add("skipped-between", plain(2, 200, 40, din=2), plain(1, 5, 16, need_w=False, need_x=False), plain(1, 5, 16, din=4))
    add("four-G", plain(1, 200, 16, din=2), plain(2, 5, 40, din=4, need_x=False), plain(3, 1, 16, din=2, need_w=False),
        plain(4, 17, 40, din=4, strided=True))
    return out


CASES = _hidden() + _head() + _pair() + _input()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def names(entry=None):
    return [c.name for c in CASES if entry is None or c.entry == entry]


def case_path(case, env=None):
    return backward_path(case.entry, case.seeds, env)


def flat_members(case):
    return [m for g in case.seeds for m in g]


def removed_by_env(case, env=None):
    """The label an RRL_PACK_PAIR_* setting takes this case off, or None."""
    try:
        want = case_path(case, env={})
        got = case_path(case, env)
    except Refused:
        return None
    return want if got != want else None


# ---- integer problems and their float64 results -----------------------------------------------------------------------------
def outputs_of(entry, m):
    """The outputs the entry computes for member m (whether a descriptor asks for them or not)."""
    head, hidden = ("dW3", "db3", "dh2"), ("dW2", "db2", "dh1") + (("first_part", "dx_part") if m.first else ())
    return dict(head=head, hidden=hidden, pair=head + hidden, input=("dW1", "db1", "dx"))[entry]


def dout_units(m, r):
    """The largest |dOut| of an exact member in units of its dyadic step (1; 2 / B; 0.5 / B)."""
    return dict(plain=r, sac_critic=2 * r, sac_policy=2)[m.kind]


def step_of(m):
    return dict(plain=1.0, sac_critic=2.0 / m.B, sac_policy=0.5 / m.B)[m.kind]


def closed_bound(entry, m, r):
    """test_stack_backward_gpu.problem's bound for this entry's outputs: every partial sum is at most the sum of the magnitudes
    of its terms.  |dh2| <= dout d r, |dh1| <= H |dh2| r, and the sums over the batch / the width add B / H such terms times an
    operand of magnitude r."""
    d = dout_units(m, r)
    e2 = m.dout * d * r
    e1 = m.H * e2 * r
    worst = dict(dW3=m.B * d * r, db3=m.B * d, dh2=e2, dW2=m.B * e2 * r, db2=m.B * e2, dh1=e1, first_part=m.B * e1 * r,
                 dx_part=m.H * e1 * r, dW1=m.B * e1 * r, db1=m.B * e1, dx=m.H * e1 * r)
    return max(worst[k] for k in outputs_of(entry, m))


def operand_range(entry, m):
    """2, or 1 where the closed-form bound asks for the narrower range."""
    for r in (2, 1):
        if closed_bound(entry, m, r) < 2 ** 24:
            return r
    raise AssertionError("no integer range keeps %r exact" % (m,))


def rints(gen, r, *shape):
    return ints(gen, *shape) if r == 2 else torch.randint(-r, r + 1, shape, generator=gen).double()


@functools.lru_cache(maxsize=None)
def operands(G, B, H, din, dout, kind, r, seed):
    """Operands of one stack (float64, on the host), and for the exact kinds dOut: computed once, shared, never modified."""
    gen = torch.Generator().manual_seed(104729 * seed + 1000 * H + B + 31 * G + 7 * dout + din)
    p = dict(x=rints(gen, r, B, din), h1=rints(gen, r, G, B, H), h2=rints(gen, r, G, B, H), W1=rints(gen, r, G, H, din),
             W2=rints(gen, r, G, H, H), W3=rints(gen, r, G, dout, H))
    if kind == "plain":
        p["dOut"] = rints(gen, r, G, B, dout)
    elif kind in ("sac_critic", "sac_policy"):
        # integer q, q_target, r, log pi; the mask v2 = 0 takes the (inexact) target term out of SAC_CRITIC
        lo = dict(q=rints(gen, r, 2, B), qt=rints(gen, r, 2, B), rew=rints(gen, r, B), logp=rints(gen, r, B))
        p["lo"] = lo
        if kind == "sac_critic":
            p["dOut"] = (2.0 * (lo["q"] - lo["rew"].unsqueeze(0)) / B).unsqueeze(-1)
        else:
            w0 = (lo["q"][0] < lo["q"][1]).double() + 0.5 * (lo["q"][0] == lo["q"][1]).double()
            p["dOut"] = torch.stack([-w0 / B, -(1.0 - w0) / B]).unsqueeze(-1)
    return p


def member_operands(entry, m, seed):
    r = operand_range(entry, m) if exact(m) else 2
    return operands(m.G, m.B, m.H, m.din, m.dout, m.kind, r, seed), r


def fold4(parts):
    """((p0 + p1) + p2) + p3 of every four consecutive column-tile partials [T, ...] -> [T / 4, ...], in the dtype given."""
    return ((parts[0::4] + parts[1::4]) + parts[2::4]) + parts[3::4]


def first_stride(m):
    return m.G * m.H * (m.din + 1) + 4                 # four floats between the row tiles' partials that nothing writes


def _chain(dO, W3, W2, W1, h2, h1, x, m2, m1, tiles):
    dh2 = (dO @ W3) * m2
    dh1 = (dh2 @ W2) * m1
    out = dict(dW3=dO.transpose(1, 2) @ h2, db3=dO.sum(1), dh2=dh2, dW2=dh2.transpose(1, 2) @ h1, db2=dh2.sum(1), dh1=dh1,
               dW1=dh1.transpose(1, 2) @ x, db1=dh1.sum(1), dx=dh1 @ W1)
    if tiles:
        G, B, H = dh1.shape
        din = x.shape[1]
        t1 = dh1.reshape(G, B // 16, 16, H)
        dW1_t = torch.einsum("gtbh,tbd->tghd", t1, x.reshape(B // 16, 16, din)).reshape(B // 16, G * H * din)
        out["first_part"] = torch.cat([dW1_t, t1.sum(2).transpose(0, 1).reshape(B // 16, G * H)], 1)
        out["dx_part"] = torch.einsum("gbch,gchd->cgbd", dh1.reshape(G, B, H // 16, 16), W1.reshape(G, H // 16, 16, din))
    return out


def chain(p, dOut):
    """The backward of one stack from dOut [G,B,dout] in float64 -> (every output, A: the same chain on the absolute values of
    all operands with the relu masks kept -- the sum of the magnitudes of every output element's terms)."""
    m2, m1 = (p["h2"] > 0).double(), (p["h1"] > 0).double()
    tiles = p["h1"].shape[1] % 16 == 0 and p["h1"].shape[2] % 16 == 0
    ops = [dOut.double()] + [p[k] for k in ("W3", "W2", "W1", "h2", "h1", "x")]
    return _chain(*ops, m2, m1, tiles), _chain(*[o.abs() for o in ops], m2, m1, tiles)


def additions(m):
    """n of the tolerance n 2^-23 A, per output: the additions along the longest chain into an element."""
    d, B, H = m.dout, m.B, m.H
    return dict(dh2=d, dW3=d + B, db3=d + B, dh1=d + H, dW2=d + B, db2=d + B, dx=d + 2 * H, dx_part=d + 2 * H, dW1=d + H + B,
                db1=d + H + B, first_part=d + H + B)


def tolerance(m, A):
    return {k: n * 2.0 ** -23 * A[k] for k, n in additions(m).items() if k in A}


def exactness(entry, m, A):
    """The largest sum of magnitudes over the entry's outputs, in units of the member's dyadic step: < 2^24 keeps f32 exact."""
    return max(float(A[k].max()) for k in outputs_of(entry, m) if k in A) / step_of(m)


# ---- device side (used by the GPU tests only) ---------------------------------------------------------------------------------
OUTPUTS = ("dW3", "db3", "dh2", "dW2", "db2", "dh1", "first_part", "dx_part", "dW1", "db1", "dx", "loss")


def nan_tail(dev, live, misaligned=False):
    """`live` as f32 on the device with DEAD_ROWS NaN rows behind it (and one NaN float in front: a base 4 bytes past a 16-byte
    boundary) -> (buffer, view)."""
    live = live.to(dtype=torch.float32)
    off = 1 if misaligned else 0
    buf = torch.full((off + live.numel() + DEAD_ROWS * live.shape[-1],), float("nan"), dtype=torch.float32, device=dev)
    view = buf[off:off + live.numel()].view(live.shape)
    view.copy_(live)
    assert (view.data_ptr() % 16 == 4) == bool(misaligned)
    return buf, view


class Member:
    """One stack on the device: inputs (NaN behind each), its float64 reference and the loss description."""

    def __init__(self, entry, m, seed, dev):
        from recovery_rl_amd import _lib
        self.entry, self.m, self.dev = entry, m, dev
        self.p, self.r = member_operands(entry, m, seed)
        p, self.t = self.p, {}
        for k in ("h2", "W3", "h1", "W2", "W1"):
            self.t[k + "_buf"], self.t[k] = nan_tail(dev, p[k], m.misalign == k)
        self.t["x_buf"], self.t["x"] = rows_then_nan(dev, p["x"], LDX_STRIDED if m.strided else None, 2 if m.strided else 0)
        self._loss_operands()
        if exact(m):
            dOut = p["dOut"]
        else:                                          # a rounded member: the f32 dOut of the stand-alone launch
            got = torch.full((m.G, m.B, m.dout), SENT, dtype=torch.float32, device=dev)
            scalars = torch.full((2,), SENT, dtype=torch.float32, device=dev)      # (the stochastic head's launch requires them)
            desc = self.loss_desc(scalars)
            _lib.check(_lib.load().rrl_loss_dout(C.byref(desc), m.B, got.data_ptr(), _lib.current_stream()), "rrl_loss_dout")
            torch.cuda.synchronize()
            dOut = got.cpu().double()
            assert bool(torch.isfinite(dOut).all()) and float(dOut.abs().max()) > 0
        self.dOut = dOut
        self.ref, self.A = chain(p, dOut)
        self.tol = tolerance(m, self.A)
        if m.kind == "plain":
            self.t["dOut_buf"], self.t["dOut"] = nan_tail(dev, dOut)
        # the stage inputs of the entries that start behind the head: exact members only (their dh2 / dh1 are f32 numbers)
        if entry in ("hidden", "input") or not m.link:
            assert exact(m)
            self.t["dh2_in_buf"], self.t["dh2_in"] = nan_tail(dev, self.ref["dh2"], m.misalign == "dh2")
            self.t["dh1_in_buf"], self.t["dh1_in"] = nan_tail(dev, self.ref["dh1"])

    def _loss_operands(self):
        m, dev, t = self.m, self.dev, self.t
        if m.kind == "plain":
            return
        put = lambda k, v: t.__setitem__(k, nan_tail(dev, v)[1])
        t["alpha"] = torch.tensor([ALPHA], device=dev)
        if m.kind in ("sac_critic", "sac_policy"):
            lo = self.p["lo"]
            put("q", lo["q"]), put("qt", lo["qt"]), put("rew", lo["rew"]), put("logp", lo["logp"])
            put("mask", torch.zeros(m.B))
        elif m.kind in ("qrisk_critic", "qrisk_policy", "dgd_qrisk"):
            import update_pieces as UP
            rows = UP.critic_rows(m.B, wide=True)
            for k in ("a", "at", "c", "m"):
                put(k, rows[k])
        else:
            import update_pieces as UP
            rows = UP.gauss_rows(m.B) if m.kind == "gauss" else UP.stoch_rows(m.B)
            put("head", rows["head"] if m.kind == "gauss" else rows["raw"]), put("eps", rows["eps"])
            put("da", UP.d_action(m.B, 2, 4))          # two critic heads' dL/d(obs | action): the action in columns 2..3
            t["scale"] = torch.tensor(UP.SCALE, device=dev)
            t["log_std"] = torch.tensor(UP.stoch_log_stds()["mixed"], dtype=torch.float32, device=dev)
            self.min_log_std = UP.MIN_LOG_STD

    def loss_desc(self, loss_buf):
        from recovery_rl_amd import _lib
        m, t, q = self.m, self.t, _lib.ptr
        L = _lib.rrl_loss_t
        if m.kind == "plain":
            return L(kind=-1, n_part=1, out=q(t["dOut"]))
        if m.kind == "sac_critic":
            return L(kind=_lib.LOSS_SAC_CRITIC, n_part=1, out=q(t["q"]), out_t=q(t["qt"]), v0=q(t["logp"]), v1=q(t["rew"]),
                     v2=q(t["mask"]), alpha=q(t["alpha"]), f0=GAMMA, loss=q(loss_buf))
        if m.kind == "sac_policy":
            return L(kind=_lib.LOSS_SAC_POLICY, n_part=1, out=q(t["q"]), v0=q(t["logp"]), alpha=q(t["alpha"]), loss=q(loss_buf))
        if m.kind == "qrisk_critic":
            return L(kind=_lib.LOSS_QRISK_CRITIC, n_part=1, out=q(t["a"]), out_t=q(t["at"]), v0=q(t["c"]), v1=q(t["m"]),
                     f0=GAMMA_SAFE, loss=q(loss_buf))
        if m.kind in ("qrisk_policy", "dgd_qrisk"):
            dgd = m.kind == "dgd_qrisk"
            return L(kind=_lib.LOSS_DGD_QRISK if dgd else _lib.LOSS_QRISK_POLICY, n_part=1, out=q(t["a"]), f0=NU if dgd else 0.0,
                     loss=q(loss_buf))
        da = dict(ld=4, n_heads=2, head_stride=t["da"].stride(0), d_action=q(t["da"][0, :, 2:]))
        if m.kind == "gauss":
            return L(kind=_lib.LOSS_GAUSS_HEAD, n_part=1, out=q(t["head"]), v0=q(t["eps"]), v1=q(t["scale"]), f0=ALPHA / m.B,
                     loss=q(loss_buf), **da)
        return L(kind=_lib.LOSS_STOCH_HEAD, n_part=1, out=q(t["head"]), v0=q(t["eps"]), v1=q(t["log_std"]), v2=q(t["scale"]),
                 f0=self.min_log_std, loss=q(loss_buf), **da)

    # ---- outputs: every one allocated, SENT-filled with a guard tail, handed to a descriptor only where the member asks ----
    def outputs(self, fold=None):
        m, dev = self.m, self.dev
        fold = m.fold if fold is None else fold
        G, B, H, din, dout = m.G, m.B, m.H, m.din, m.dout
        shapes = dict(dW3=(G, dout, H), db3=(G, dout), dh2=(G, B, H), dW2=(G, H, H), db2=(G, H), dh1=(G, B, H),
                      first_part=(-(-B // 16), first_stride(m)), dx_part=(max(1, H // (64 if fold else 16)), G, B, din),
                      dW1=(G, H, din), db1=(G, H), dx=(G, B, din), loss=(2,))
        o = {"fold": bool(fold)}
        for k, shape in shapes.items():
            o[k + "_flat"], o[k] = guarded(dev, *shape)
        return o

    def asked(self, entry=None):
        """The outputs the member's descriptors of `entry` hand over."""
        m, entry = self.m, entry or self.entry
        head = (("dW3", "db3") if m.dW3 else ()) + (("dh2",) if m.dh2 else ())
        hidden = ((("dW2", "db2") if m.dW2 else ()) + (("dh1",) if m.dh1 else ())
                  + (("first_part",) if m.first and "w" in m.first else ()) + (("dx_part",) if m.first and "x" in m.first else ()))
        inp = (("dW1", "db1") if m.need_w else ()) + (("dx",) if m.need_x else ())
        return dict(head=head, hidden=hidden, pair=head + hidden, input=inp)[entry]

    def head_desc(self, o):
        from recovery_rl_amd import _lib
        m, t, q = self.m, self.t, _lib.ptr
        return _lib.rrl_head_bwd_t(self.loss_desc(o["loss"]), m.G, m.B, m.H, m.dout, q(t["h2"]), q(t["W3"]),
                                   q(o["dW3"]) if m.dW3 else None, q(o["db3"]) if m.dW3 else None, q(o["dh2"]) if m.dh2 else None)

    def hidden_desc(self, o, dh2):
        from recovery_rl_amd import _lib
        m, t, q = self.m, self.t, _lib.ptr
        first = _lib.rrl_first_layer_t()
        if m.first:
            first = _lib.rrl_first_layer_t(q(t["x"]), q(t["W1"]), t["x"].stride(0), m.din,
                                           q(o["first_part"]) if "w" in m.first else None, first_stride(m),
                                           q(o["dx_part"]) if "x" in m.first else None, 1 if o["fold"] else 0)
        return _lib.rrl_hidden_bwd_t(m.G, m.B, m.H, q(dh2), q(t["h1"]), q(t["W2"]), q(o["dW2"]) if m.dW2 else None,
                                     q(o["db2"]) if m.dW2 else None, q(o["dh1"]) if m.dh1 else None, first)

    def input_desc(self, o):
        from recovery_rl_amd import _lib
        m, t, q = self.m, self.t, _lib.ptr
        return _lib.rrl_input_bwd_t(m.G, m.B, m.H, m.din, t["x"].stride(0), q(t["dh1_in"]), q(t["x"]), q(t["W1"]),
                                    q(o["dW1"]) if m.need_w else None, q(o["db1"]) if m.need_w else None,
                                    q(o["dx"]) if m.need_x else None)

    def link_of(self, o):
        """hidden[k].dh2: heads[k].dh2, or (unlinked; the hidden entry) a tensor of its own that holds dh2."""
        return o["dh2"] if (self.m.link and self.entry == "pair") else self.t["dh2_in"]


def _array(ctype, descs):
    return (ctype * len(descs))(*descs)


def _packed_args(ctype, seeds):
    arrs = [_array(ctype, d) for d in seeds]
    n = (C.c_int * len(seeds))(*[len(d) for d in seeds])
    ptrs = (C.POINTER(ctype) * len(seeds))(*[C.cast(a, C.POINTER(ctype)) for a in arrs])
    return arrs, n, ptrs


def launch(entry, groups, outs):
    """One call of `entry` on groups of Member (one group: the solo entry; S groups: the packed one) into `outs` (the same
    nesting) -> the return code."""
    from recovery_rl_amd import _lib
    lib, st = _lib.load(), _lib.current_stream()
    if entry == "input":
        (g,), (og,) = groups, outs
        d = [mb.input_desc(o) for mb, o in zip(g, og)]
        return lib.rrl_mlp_input_backward_multi(len(d), _array(_lib.rrl_input_bwd_t, d), st)
    heads = hidden = [[]] * len(groups)
    if entry != "hidden":
        heads = [[mb.head_desc(o) for mb, o in zip(g, og)] for g, og in zip(groups, outs)]
    if entry != "head":
        hidden = [[mb.hidden_desc(o, mb.link_of(o)) for mb, o in zip(g, og)] for g, og in zip(groups, outs)]
    if len(groups) == 1:
        n = len(groups[0])
        if entry == "head":
            return lib.rrl_mlp_head_backward_multi(n, _array(_lib.rrl_head_bwd_t, heads[0]), st)
        if entry == "hidden":
            return lib.rrl_mlp_hidden_backward_multi(n, _array(_lib.rrl_hidden_bwd_t, hidden[0]), st)
        return lib.rrl_mlp_backward_pair_multi(n, _array(_lib.rrl_head_bwd_t, heads[0]), _array(_lib.rrl_hidden_bwd_t, hidden[0]), st)
    S = len(groups)
    keep_h, n, hp = _packed_args(_lib.rrl_head_bwd_t, heads)
    keep_d, nd, dp = _packed_args(_lib.rrl_hidden_bwd_t, hidden)
    assert keep_h is not None and keep_d is not None          # (alive until the call returns)
    n = nd if entry == "hidden" else n
    if entry == "head":
        return lib.rrl_mlp_head_backward_multi_packed(S, n, hp, st)
    if entry == "hidden":
        return lib.rrl_mlp_hidden_backward_multi_packed(S, n, dp, st)
    return lib.rrl_mlp_backward_pair_multi_packed(S, n, hp, dp, st)


def untouched(o, but=()):
    """The outputs (guard tails included) that hold anything but the sentinel, among those not in `but`."""
    return [k for k in OUTPUTS if k not in but and not bool((o[k + "_flat"] == SENT).all())]


def guards_written(o):
    return [k for k in OUTPUTS if not bool((guard_of(o[k + "_flat"], o[k]) == SENT).all())]


def live(mb, o, k):
    """The part of output k that the kernels write (first_part: the row tiles' partials without the floats between them)."""
    return o[k][:, :first_stride(mb.m) - 4] if k == "first_part" else o[k]


def check_member(mb, o, written, what=""):
    """Output buffers of one member against float64 by the member's class; `written`: the outputs the launch must have written,
    every other one must hold the sentinel."""
    assert not guards_written(o), (what, "written behind the end of", guards_written(o))
    left = untouched(o, but=tuple(written) + (("loss",) if mb.m.kind != "plain" else ()))     # (the scalars: test_update_pieces_gpu.py)
    assert not left, (what, "written without being asked for", left)
    for k in written:
        got = live(mb, o, k)
        ref, A = mb.ref[k], mb.A[k]
        if k == "dx_part" and o["fold"]:
            ref, A = fold4(ref), fold4(A)
        if k == "first_part":
            assert bool((o[k][:, first_stride(mb.m) - 4:] == SENT).all()), (what, "first_part between the row tiles")
        assert got.shape == ref.shape, (what, k, got.shape, ref.shape)
        if exact(mb.m):
            assert torch.equal(got, ref.float().to(got.device)), (what, k)
        else:
            tol = additions(mb.m)[k] * 2.0 ** -23 * A
            err = (got.double().cpu() - ref).abs()
            assert bool((err <= tol).all()), (what, k, float((err - tol).max()), float(A.max()))


def same_bits(a, b, what="", skip=()):
    """Two runs' outputs, guard tails and sentinels included, bit for bit; folded against unfolded dx partials through fold4."""
    for k in OUTPUTS:
        if k in skip:
            continue
        if k == "dx_part" and a["fold"] != b["fold"]:
            fa, fb = (a[k], fold4(b[k])) if a["fold"] else (fold4(a[k]), b[k])
            if bool((a[k] == SENT).all()) and bool((b[k] == SENT).all()):
                continue
            assert torch.equal(fa, fb), (what, "dx_part, folded against ((p0 + p1) + p2) + p3")
        else:
            assert torch.equal(a[k + "_flat"], b[k + "_flat"]), (what, k)
