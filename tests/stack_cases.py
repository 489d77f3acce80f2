"""Cases, float64 reference, descriptors and a restatement of the host dispatch for the three-layer stack forward
(csrc/mlp_fwd_kernels.hip), shared by test_stack_forward_cpu.py and test_stack_forward_gpu.py.

Operands are integers in [-2, 2]: every product and every partial sum of every layer is an integer below 2^24, exact in f32 in
whatever order a kernel adds it (MFMA chains, the four column-group partials, row16_sum, sum_partials_kernel), so the kernels'
results must EQUAL the float64 ones.

The library does not say which kernel it launched.  forward_path() restates the choice rrl_mlp3_forward, build_stack_group,
rrl_mlp3_forward_multi_packed and rrl_pack::seed_share make on the host, with their constants as literals;
test_stack_forward_cpu.py parses the constants out of the sources and proves that the case table below reaches every path and
every ragged condition, so a retuned constant fails there instead of moving a case onto another kernel unnoticed."""
import collections
import ctypes as C
import functools

import torch

# ---- the host dispatch's constants, as literals (test_stack_forward_cpu.py compares them with the sources) ------------------
CONSTANTS = dict(kStackRows=16, kSplit=4, kSplitSmallM=1024, kBigR=2, kPackSmallR2MinSeeds=3, RRL_FWD_LOOP_WAVES=3,
                 kLoopMinBlocks=8, kLoopMaxBlocks=32, kStackMaxH=256, plain_r2_above=256, kMaxGroup=4, kMaxSeeds=16)
ROWS, SPLIT, SMALL_M, BIG_R = 16, 4, 1024, 2
PACK_SMALL_R2_MIN_SEEDS, LOOP_WAVES, LOOP_MIN, LOOP_MAX = 3, 3, 8, 32
RESIDENT = 256 * LOOP_WAVES                  # kResidentWorkgroups
PLAIN_R2_ABOVE, MAX_GROUP, MAX_H = 256, 4, 256

Member = collections.namedtuple("Member", "G M H din dout scratch", defaults=(True,))
Path = collections.namedtuple("Path", "label path rows tiles small_r nb loop walks", defaults=(1, 1, False, ()))
LABELS = ("1", "2", "0/256", "0/gen", "3", "5", "packed0", "packed3", "packed3/small2", "packed4", "riders", "riders_keyed")
TWO_ROW_LABELS = ("2", "3", "5", "packed3", "packed3/small2", "packed4", "riders")
ONE_ROW_LABELS = ("1", "0/256", "0/gen", "packed0", "riders", "riders_keyed")


def ceil_div(a, b):
    return (a + b - 1) // b


def is_split(m):
    """rrl_mlp3_is_split and a scratch buffer: the column-split kernels."""
    return bool(m.scratch) and m.H % (16 * SPLIT) == 0 and m.H <= MAX_H


def pinned_mapping(S, always=False):
    """pack.hpp pinned_mapping -> (pinned, sp, r) with RRL_PACK_PINNED unset."""
    if S > 8:
        if 8 * ceil_div(S, 8) - S > 2:
            return False, 0, 1
        return True, 8, ceil_div(S, 8)
    sp = 1
    while sp < S:
        sp <<= 1
    if not always and sp == 8 and S <= 6:
        return False, 0, 1
    return True, sp, 1


def seed_share(S):
    pinned, sp, r = pinned_mapping(S)
    return sp * r if pinned else 1


def group_plan(members, big_r=BIG_R, small_r=1, loop_nb=1, flat=True):
    """build_stack_group -> (path, rows per block, row blocks, blocks per workgroup, workgroups) per member; ValueError where
    it returns RRL_EINVAL."""
    if not 0 < len(members) <= MAX_GROUP:
        raise ValueError("group size")
    any_big = any(is_split(m) and m.H == 256 and m.M > SMALL_M for m in members)
    all_split256 = all(is_split(m) and m.H == 256 for m in members)
    any_small = any(m.M <= SMALL_M for m in members)
    mixed = any_big and any_small and all_split256
    if mixed and not flat:
        small_r = big_r
    path, rows, tiles, nbs, wgs = -1, [], [], [], []
    for m in members:
        tiles16 = ceil_div(m.M, ROWS)
        nb = 1
        if is_split(m):
            my = 0 if (m.M <= SMALL_M or m.H != 256) else 3
            if my == 0 and small_r > 1 and m.H != 256:
                raise ValueError("two-row tiles need H = 256")
            r = (small_r if my == 0 else big_r) * ROWS
            if mixed:
                my = 5
            t = ceil_div(m.M, r)
            nb = min(loop_nb, t)
            wg = ceil_div(t, nb) * m.G * SPLIT
        elif tiles16 * m.G > PLAIN_R2_ABOVE:
            my, r = 2, 2 * ROWS
            t = ceil_div(m.M, r)
            wg = t * m.G
        else:
            my, r, t = 1, ROWS, tiles16
            wg = t * m.G
        if path >= 0 and my != path:
            raise ValueError("members on different paths")
        path = my
        rows.append(r), tiles.append(t), nbs.append(nb), wgs.append(wg)
    return path, rows, tiles, nbs, wgs


def forward_path(members, packed_S=None):
    """The path label of the dispatch table for a group of Members (rrl_mlp3_forward for one, rrl_mlp3_forward_multi and
    rrl_mlp3_forward_riders otherwise) or, with packed_S, for packed_S groups of them (rrl_mlp3_forward_multi_packed): then
    also small_r, the blocks per workgroup nb, whether the loop kernel is taken and the blocks each member's last workgroup
    walks."""
    if packed_S is None:
        path, rows, tiles, _, _ = group_plan(members)
        if path == 5:                  # the flat grid: every member on the tiles of its stand-alone launch
            rows = [BIG_R * ROWS if m.M > SMALL_M else ROWS for m in members]
        label = str(path)
        if path == 0:
            widths = {m.H == 256 for m in members}
            assert len(widths) == 1, "keep a path-0 group on one body"
            label = "0/256" if widths.pop() else "0/gen"
        return Path(label, path, tuple(rows), tuple(tiles))
    seeds = members
    assert packed_S == len(seeds) and 2 <= packed_S <= CONSTANTS["kMaxSeeds"]
    S = packed_S
    all256 = all(m.H == 256 for g in seeds for m in g)
    small_r = BIG_R if (S >= PACK_SMALL_R2_MIN_SEEDS and all256) else 1

    def build_all(loop_nb):
        path, plans = -1, []
        for g in seeds:
            my, rows, tiles, nbs, wgs = group_plan(g, BIG_R, small_r, loop_nb, flat=False)
            my = 3 if my == 5 else my
            if my not in (0, 3) or (path >= 0 and my != path):
                raise ValueError("packed: column-split members on one path only")
            path = my
            plans.append((rows, tiles, nbs, wgs))
        return path, plans
    loop_nb = 1
    path, plans = build_all(1)
    if path == 3 and all256:
        share = seed_share(S)

        def fits():
            per_seed = [sum(p[3]) for p in plans]
            if share > 1 and any(w * share > RESIDENT for w in per_seed):
                return False
            return sum(per_seed) <= RESIDENT
        while not fits() and loop_nb < LOOP_MAX:
            loop_nb += 1
            path, plans = build_all(loop_nb)
        if loop_nb < LOOP_MIN:
            loop_nb = 1
            path, plans = build_all(1)
    small_on_two = any(m.M <= SMALL_M and r == BIG_R * ROWS for g, p in zip(seeds, plans) for m, r in zip(g, p[0]))
    if path == 3 or (small_r > 1 and path == 0):
        label = "packed4" if loop_nb > 1 else ("packed3/small2" if small_on_two else "packed3")
    else:
        label = "packed0"
    rows = tuple(r for p in plans for r in p[0])
    tiles = tuple(t for p in plans for t in p[1])
    nbs = tuple(n for p in plans for n in p[2])
    walks = tuple(t - (ceil_div(t, n) - 1) * n for t, n in zip(tiles, nbs))     # blocks of each member's last workgroup
    if path == 3 or (small_r > 1 and path == 0):      # small members on multi-row tiles run the large-batch kernel; 4 = its loop form
        path = 4 if loop_nb > 1 else 3
    return Path(label, path, rows, tiles, small_r, loop_nb, loop_nb > 1, walks)


# ---- the case table ---------------------------------------------------------------------------------------------------------
# entry: positional (rrl_mlp3_forward), multi (rrl_mlp3_forward_multi), packed (rrl_mlp3_forward_multi_packed), riders and
# riders_keyed (rrl_mlp3_forward_riders).  members: Members, for packed one tuple of them per seed.
# opts: finalize (positional, split), strided (x is a column view, ldx 7), save (False: h1 and h2 null, as the target networks'
# forwards run), w2p (None / "packed" / "other": a copy made from a different W2, whose result must be that W2's), heads (per
# member None or (kind, n_part, obs_in given)).
Case = collections.namedtuple("Case", "name entry members opts")
TWIN, POLICY, ODD = (2, 4, 1), (1, 2, 4), (3, 3, 2)          # (G, din, dout): twin critic, policy, one that is neither
GAUSS, STOCH = 0, 1


def _m(gdd, M, H, scratch=True):
    return Member(gdd[0], M, H, gdd[1], gdd[2], scratch)


def _tag(gdd):
    return "g%dd%do%d" % gdd


def _positional():
    out = []
    small = (1, 15, 16, 17, 33, 200)
    for H in (16, 48, 80, 240, 256):
        for gdd in (TWIN, POLICY):
            for M in small:
                out.append(Case("pos-plain-H%d-M%d-%s" % (H, M, _tag(gdd)), "positional", (_m(gdd, M, H, False),),
                                dict(strided=(H == 48 and M == 33))))
    out.append(Case("pos-plain-H48-M33-" + _tag(ODD), "positional", (_m(ODD, 33, 48, False),), {}))
    out.append(Case("pos-plain-H80-M17-" + _tag(ODD) + "-unsaved", "positional", (_m(ODD, 17, 80, False),), dict(save=False)))
    # two row tiles per workgroup once ceil(M / 16) G > 256: 17, 5 and 21 live rows in the last block
    for gdd, M in ((POLICY, 4096 + 17), (POLICY, 4096 + 5), (TWIN, 2064 + 5)):
        out.append(Case("pos-plain-H48-M%d-%s" % (M, _tag(gdd)), "positional", (_m(gdd, M, 48, False),),
                        dict(strided=(M == 4096 + 5))))
    out.append(Case("pos-plain-H48-M4117-" + _tag(POLICY) + "-unsaved", "positional", (_m(POLICY, 4096 + 21, 48, False),),
                    dict(save=False)))
    for H in (64, 128, 192, 256):
        # H = 256 above kSplitSmallM: 1, 16, 17, 21 and 1 + 32 live rows in the last two-row block
        for M in small + ((1024, 1025, 1040, 1041, 1045, 1057) if H == 256 else ()):
            for gdd in (TWIN, POLICY):
                for fin in (0, 1):
                    out.append(Case("pos-split-H%d-M%d-%s-fin%d" % (H, M, _tag(gdd), fin), "positional", (_m(gdd, M, H),),
                                    dict(finalize=fin, strided=(fin == 1 and M in (33, 1045) and H in (128, 256)),
                                         save=not (fin == 0 and M in (17, 1041)))))
    out.append(Case("pos-split-H128-M17-" + _tag(ODD) + "-fin1", "positional", (_m(ODD, 17, 128),), dict(finalize=1)))
    return out


def _multi():
    out = []

    def add(name, members, **opts):
        w2ps = (None, "packed") if all(m.H == 256 and is_split(m) for m in members) else (None,)
        for w2p in w2ps:
            out.append(Case("multi-%s%s" % (name, "-w2p" if w2p else ""), "multi", tuple(members), dict(opts, w2p=w2p)))
    add("lone-path0-H256", [_m(TWIN, 200, 256)], strided=True)
    add("lone-path0-H128", [_m(POLICY, 17, 128)], strided=True)
    add("lone-path0-H192", [_m(TWIN, 33, 192)])
    add("lone-path1", [_m(TWIN, 33, 48, False)], strided=True)
    add("lone-path2", [_m(POLICY, 4096 + 5, 48, False)])
    add("lone-path3-M1057", [_m(TWIN, 1057, 256)], strided=True)
    add("lone-path3-M1045", [_m(POLICY, 1045, 256)])
    # kMaxGroup members of different M, G and dout on path 0: the grid is the largest member's, the others' surplus workgroups leave
    add("four-path0-H256", [_m(TWIN, 200, 256), _m(POLICY, 17, 256), _m(ODD, 33, 256), _m(POLICY, 1024, 256)])
    add("two-path0-H128", [_m(TWIN, 200, 128), _m(POLICY, 17, 128)])
    add("three-path1", [_m(TWIN, 33, 48, False), _m(POLICY, 200, 80, False), _m(ODD, 17, 16, False)])
    small = [_m(POLICY, 17, 256), _m(TWIN, 200, 256), _m(POLICY, 1024, 256)]
    add("path5-large-first", [_m(TWIN, 1057, 256)] + small, strided=True)
    add("path5-large-last", small + [_m(TWIN, 1057, 256)])
    add("path5-M1045", [_m(TWIN, 200, 256), _m(POLICY, 1045, 256)])
    # h1 and h2 null
    add("lone-path0-H256-unsaved", [_m(POLICY, 200, 256)], save=False)
    add("lone-path0-H128-unsaved", [_m(TWIN, 33, 128)], save=False)
    add("lone-path1-unsaved", [_m(POLICY, 33, 48, False)], save=False)
    add("lone-path3-unsaved", [_m(POLICY, 1057, 256)], save=False)
    add("path5-unsaved", [_m(POLICY, 1045, 256), _m(TWIN, 17, 256)], save=False)
    # a fragment-order copy made from another W2 is what is read
    out.append(Case("multi-lone-path0-H256-w2p-other", "multi", (_m(TWIN, 200, 256),), dict(w2p="other")))
    out.append(Case("multi-lone-path3-w2p-other", "multi", (_m(POLICY, 1057, 256),), dict(w2p="other")))
    return out


def _heads():
    out = []
    for M in (17, 200, 1025, 1057):
        for kind in (GAUSS, STOCH):
            for n_part in (1, 4):
                for obs in (False, True):
                    out.append(Case("head-M%d-%s-p%d-%s" % (M, "gauss" if kind == GAUSS else "stoch", n_part, "obs" if obs else "x"),
                                    "multi", (_m(TWIN, M, 256),), dict(heads=((kind, n_part, obs),), w2p="packed" if obs else None)))
    out.append(Case("head-H128-M17-gauss", "multi", (_m(TWIN, 17, 128),), dict(heads=((GAUSS, 4, True),))))
    out.append(Case("head-H128-M200-stoch", "multi", (_m(TWIN, 200, 128),), dict(heads=((STOCH, 1, False),))))
    out.append(Case("head-path5-large-first", "multi", (_m(TWIN, 1057, 256), _m(TWIN, 200, 256), _m(POLICY, 17, 256)),
                    dict(heads=((GAUSS, 4, True), (STOCH, 1, False), None))))
    out.append(Case("head-path5-large-last", "multi", (_m(TWIN, 17, 256), _m(TWIN, 1045, 256)),
                    dict(heads=((GAUSS, 1, False), (STOCH, 4, True)), w2p="packed")))
    return out


def _packed():
    out = []

    def add(name, seeds, **opts):
        w2ps = (None, "packed") if all(m.H == 256 for g in seeds for m in g) and not opts.get("once") else (None,)
        for w2p in w2ps:
            out.append(Case("packed-%s%s" % (name, "-w2p" if w2p else ""), "packed", tuple(tuple(g) for g in seeds),
                            dict(opts, w2p=opts.get("w2p", w2p))))
    for H in (128, 256):
        add("S2-path0-H%d" % H, [[_m(TWIN, 200, H), _m(POLICY, 17, H)], [_m(POLICY, 17, H), _m(TWIN, 200, H)]], strided=(H == 256))
    add("S2-path0-H128-unsaved", [[_m(POLICY, 200, 128)], [_m(TWIN, 17, 128)]], save=False)
    add("S2-path0-H256-unsaved", [[_m(POLICY, 200, 256)], [_m(TWIN, 17, 256)]], save=False)
    # from three seeds on the small members run on two-row tiles: M = 17 leaves one live row in the second tile
    add("S3-small-two-row", [[_m(TWIN, 200, 256), _m(POLICY, 17, 256)], [_m(POLICY, 17, 256)], [_m(TWIN, 200, 256)]], strided=True)
    add("S3-small-two-row-unsaved", [[_m(POLICY, 200, 256)], [_m(TWIN, 17, 256)], [_m(POLICY, 17, 256)]], save=False)
    add("S2-path3", [[_m(TWIN, 1057, 256)], [_m(POLICY, 1045, 256)]], strided=True)
    add("S2-path3-unsaved", [[_m(POLICY, 1057, 256)], [_m(TWIN, 1045, 256)]], save=False)
    add("S2-mixed", [[_m(TWIN, 1057, 256), _m(POLICY, 200, 256)], [_m(POLICY, 17, 256), _m(TWIN, 1045, 256)]])
    # the loop form: 8 pinned seeds of 86 two-row blocks each, 8 blocks per workgroup, the last one walks 6; the last block has
    # 5 (even seeds, twin critics) or 21 (odd seeds, one head: nothing behind row M but the guard) live rows
    loop = [[_m(TWIN, 2725, 256) if s % 2 == 0 else _m(POLICY, 2741, 256)] for s in range(8)]
    add("S8-loop", loop, once=True, strided=True)      # the loop form fetches the next block's x one block ahead
    add("S8-loop-unsaved", loop, once=True, w2p="packed", save=False)
    add("S8-loop-head", loop, once=True, w2p="packed",
        heads=tuple(({0: (GAUSS, 4, True), 2: (STOCH, 1, False)}.get(s % 4),) for s in range(8)))
    return out


def _riders():
    out = []
    for name, m in (("path0", _m(POLICY, 200, 256)), ("path3-M1057", _m(TWIN, 1057, 256)), ("path3-M1045", _m(POLICY, 1045, 256))):
        for w2p in (None, "packed"):
            out.append(Case("riders-noise-%s%s" % (name, "-w2p" if w2p else ""), "riders", (m,),
                            dict(w2p=w2p, strided=(name == "path0") == (w2p is None))))
    out.append(Case("riders-noise-path0-unsaved", "riders", (_m(TWIN, 200, 256),), dict(save=False)))
    out.append(Case("riders-noise-path3-unsaved", "riders", (_m(TWIN, 1045, 256),), dict(w2p="packed", save=False)))
    for w2p in (None, "packed"):      # the batch's s' over its s, B = 100: the seventh block of 16 rows has 8
        out.append(Case("riders-keyed-B100%s" % ("-w2p" if w2p else ""), "riders_keyed", (_m(POLICY, 200, 256),), dict(w2p=w2p)))
    out.append(Case("riders-keyed-B100-unsaved", "riders_keyed", (_m(POLICY, 200, 256),), dict(save=False)))
    return out


CASES = _positional() + _multi() + _heads() + _packed() + _riders()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def names(entry=None, heads=None):
    return [c.name for c in CASES if (entry is None or c.entry == entry) and (heads is None or bool(c.opts.get("heads")) == heads)]


def case_path(case):
    if case.entry == "packed":
        return forward_path(case.members, packed_S=len(case.members))
    p = forward_path(case.members)
    if case.entry in ("riders", "riders_keyed"):
        assert p.path in (0, 3) and case.members[0].H == 256
        return p._replace(label=case.entry)
    return p


def flat_members(case):
    return [m for g in case.members for m in g] if case.entry == "packed" else list(case.members)


# ---- integer problems and their float64 results -----------------------------------------------------------------------------
def bound(m):
    """Closed-form bounds on |h1|, |h2| and on |out| and every partial sum of it, for operands in [-2, 2]."""
    b1 = 2 * 2 * m.din + 2
    b2 = 2 * b1 * m.H + 2
    return b1, b2, 2 * b2 * m.H + 2


def ints(gen, *shape):
    return torch.randint(-2, 3, shape, generator=gen).double()


def reference(x, W1, b1, W2, b2, W3, b3):
    """relu(x W1' + b1), relu(h1 W2' + b2), h2 W3' + b3 in float64, and (H a multiple of 64) the four column-group partials
    of the last layer, partial 0 carrying b3."""
    h1 = torch.relu(x @ W1.transpose(1, 2) + b1.unsqueeze(1))
    h2 = torch.relu(h1 @ W2.transpose(1, 2) + b2.unsqueeze(1))
    out = h2 @ W3.transpose(1, 2) + b3.unsqueeze(1)
    ref = dict(h1=h1, h2=h2, out=out)
    H = W2.shape[1]
    if H % (16 * SPLIT) == 0:
        hs = H // SPLIT
        parts = [h2[:, :, z * hs:(z + 1) * hs] @ W3[:, :, z * hs:(z + 1) * hs].transpose(1, 2) for z in range(SPLIT)]
        parts[0] = parts[0] + b3.unsqueeze(1)
        ref["partials"] = torch.stack(parts)
    return ref


@functools.lru_cache(maxsize=None)
def problem(m, seed=0):
    """Operands of one Member (float64, on the host) and their float64 results: computed once, shared, never modified."""
    gen = torch.Generator().manual_seed(7919 * seed + 1000 * m.H + m.M + 31 * m.G + 3 * m.dout)
    G, M, H, din, dout = m[:5]
    p = dict(x=ints(gen, M, din), W1=ints(gen, G, H, din), b1=ints(gen, G, H), W2=ints(gen, G, H, H), b2=ints(gen, G, H),
             W3=ints(gen, G, dout, H), b3=ints(gen, G, dout), W2other=ints(gen, G, H, H))
    ref = reference(p["x"], p["W1"], p["b1"], p["W2"], p["b2"], p["W3"], p["b3"])
    b1, b2, b3 = bound(m)
    assert b3 < 2 ** 24
    assert float(ref["h1"].abs().max()) <= b1 and float(ref["h2"].abs().max()) <= b2
    assert max(float(v.abs().max()) for v in ref.values()) <= b3 < 2 ** 24
    return p, ref


def reference_other(m, seed=0):
    p, _ = problem(m, seed)
    return reference(p["x"], p["W1"], p["b1"], p["W2other"], p["b2"], p["W3"], p["b3"])


# ---- descriptors with guard tails (device side; used by the GPU tests only) -------------------------------------------------
SENT = -1234.5           # no integer: an output that was written cannot hold it
DEAD_ROWS = 32           # NaN rows behind the M rows of every input: a two-row block's reads past row M stay inside the buffer
GUARD_ROWS = 32          # rows of SENT behind every output: a two-row block's stores past row M would stay inside the allocation
LDX_STRIDED = 7


def guarded(dev, *shape):
    """A SENT-filled output of `shape` (rows of shape[-1] floats) with GUARD_ROWS more rows behind it -> (flat buffer, view)."""
    n = 1
    for s in shape:
        n *= s
    flat = torch.full((n + GUARD_ROWS * shape[-1],), SENT, dtype=torch.float32, device=dev)
    return flat, flat[:n].view(*shape)


def guard_of(flat, view):
    return flat[view.numel():]


def rows_then_nan(dev, live, width=None, col0=0):
    """[M + DEAD_ROWS, width] of NaN with `live` [M, w] at columns col0..; -> (buffer, view of the live part)."""
    M, w = live.shape
    buf = torch.full((M + DEAD_ROWS, width or w), float("nan"), dtype=torch.float32, device=dev)
    buf[:M, col0:col0 + w] = live.to(device=dev, dtype=torch.float32)
    return buf, buf[:M, col0:col0 + w]


def w2_pack(W2):
    from recovery_rl_amd import _lib
    w2p = torch.empty_like(W2)
    _lib.check(_lib.load().rrl_w2_pack(W2.shape[0], W2.shape[1], W2.data_ptr(), w2p.data_ptr(), _lib.current_stream()),
               "rrl_w2_pack")
    return w2p


def device_stack(m, p, dev, save=True, strided=False, w2p=None, x_live=None, ldx=None):
    """A hand-made rrl_stack_t for Member m on the operands p -> (descriptor, tensors by name).  x is the first M rows of a
    buffer whose following rows, and whose other columns (strided: ldx 7, x at column 2; or a given ldx, x at column 0), are NaN;
    h1, h2, out and scratch are SENT with a guard tail."""
    from recovery_rl_amd import _lib
    f32 = lambda t: t.to(device=dev, dtype=torch.float32).contiguous()
    t = {k: f32(p[k]) for k in ("W1", "b1", "W2", "b2", "W3", "b3")}
    live = p["x"] if x_live is None else x_live
    t["xbuf"], t["x"] = rows_then_nan(dev, live, LDX_STRIDED if strided else ldx, 2 if strided else 0)
    G, M, H, din, dout = m[:5]
    t["out_flat"], t["out"] = guarded(dev, G, M, dout)
    if save:
        t["h1_flat"], t["h1"] = guarded(dev, G, M, H)
        t["h2_flat"], t["h2"] = guarded(dev, G, M, H)
    if m.scratch:
        t["scratch_flat"], t["scratch"] = guarded(dev, SPLIT, G, M, dout)
    if w2p == "packed":
        t["W2p"] = w2_pack(t["W2"])
    elif w2p == "other":
        t["W2p"] = w2_pack(f32(p["W2other"]))
    q = _lib.ptr
    desc = _lib.rrl_stack_t(G, M, H, din, dout, t["x"].stride(0), q(t["x"]), q(t["W1"]), q(t["b1"]), q(t["W2"]), q(t["b2"]),
                            q(t["W3"]), q(t["b3"]), q(t.get("h1")), q(t.get("h2")), q(t["out"]), q(t.get("scratch")),
                            _lib.rrl_policy_head_t(), 0, q(t.get("W2p")))
    return desc, t


def guards_intact(t):
    return [k for k in ("out", "h1", "h2", "scratch")
            if k in t and not bool((guard_of(t[k + "_flat"], t[k]) == SENT).all())]


def check_exact(t, ref, split, out_written, what=""):
    """Every buffer of one stack against float64: guard tails, saved activations, the four partials and their float64 sum,
    the summed output (or its sentinel where no kernel was asked to write it)."""
    dev = t["out"].device
    want = lambda v: v.float().to(dev)
    assert not guards_intact(t), (what, "written behind the end of", guards_intact(t))
    for k in ("h1", "h2"):
        if k in t:
            assert torch.equal(t[k], want(ref[k])), (what, k)
    if split:
        assert torch.equal(t["scratch"], want(ref["partials"])), (what, "partials")
        assert torch.equal(t["scratch"].double().sum(0).float(), want(ref["out"])), (what, "sum of the partials")
    elif "scratch" in t:
        assert bool((t["scratch"] == SENT).all()), (what, "scratch written on a path without partials")
    if out_written:
        assert torch.equal(t["out"], want(ref["out"])), (what, "out")
    else:
        assert bool((t["out"] == SENT).all()), (what, "out written without finalize")


def stack_array(descs):
    from recovery_rl_amd import _lib
    return (_lib.rrl_stack_t * len(descs))(*descs)


def forward_multi(descs):
    from recovery_rl_amd import _lib
    arr = stack_array(descs)
    _lib.check(_lib.load().rrl_mlp3_forward_multi(len(descs), arr, _lib.current_stream()), "rrl_mlp3_forward_multi")


def forward_packed(seeds):
    """seeds: one list of descriptors per seed."""
    from recovery_rl_amd import _lib
    arrs = [stack_array(d) for d in seeds]
    n = (C.c_int * len(seeds))(*[len(d) for d in seeds])
    ptrs = (C.POINTER(_lib.rrl_stack_t) * len(seeds))(*[C.cast(a, C.POINTER(_lib.rrl_stack_t)) for a in arrs])
    _lib.check(_lib.load().rrl_mlp3_forward_multi_packed(len(seeds), n, ptrs, _lib.current_stream()),
               "rrl_mlp3_forward_multi_packed")


# ---- a policy head inside the stack kernel (rrl_stack_t.in_head) ------------------------------------------------------------
def head_operands(M, kind, n_part, obs, dev, seed):
    """Operands of a policy head over M rows, every per-row array with DEAD_ROWS NaN rows behind it; outputs: `xa`
    [M + DEAD_ROWS, 4] (obs_out | action, ld_action 4) and logp, SENT-filled."""
    gen = torch.Generator().manual_seed(seed)
    u = lambda *s: torch.rand(*s, generator=gen) * 2 - 1
    w = 4 if kind == GAUSS else 2
    parts = torch.full((n_part, M + DEAD_ROWS, w), float("nan"))
    parts[:, :M] = u(n_part, M, w) / n_part
    if kind == GAUSS:
        parts[:, :M, 2:] -= 0.5 / n_part
    o = dict(parts=parts.to(dev).contiguous(), scale=torch.tensor([1.5, 2.0], device=dev), bias=torch.tensor([-0.5, 1.0], device=dev),
             log_std=torch.tensor([-0.7, -16.0], device=dev), kind=kind, n_part=n_part, M=M)
    o["eps"] = rows_then_nan(dev, u(M, 2) * 2)[0] if (kind == GAUSS or n_part == 4) else None
    o["obs_in"] = rows_then_nan(dev, ints(gen, M, 2))[0] if obs else None
    return o


def head_outputs(o, dev):
    M = o["M"]
    return dict(xa=torch.full((M + DEAD_ROWS, 4), SENT, dtype=torch.float32, device=dev),
                logp=torch.full((M + DEAD_ROWS,), SENT, dtype=torch.float32, device=dev))


def head_desc(o, outs):
    from recovery_rl_amd import _lib
    import math
    q = _lib.ptr
    gauss = o["kind"] == GAUSS
    return _lib.rrl_policy_head_t(
        kind=_lib.HEAD_GAUSS if gauss else _lib.HEAD_STOCH, B=o["M"], head=q(o["parts"]), n_part=o["n_part"],
        part_stride=o["parts"][0].numel(), eps=q(o["eps"]), scale=q(o["scale"]), bias=q(o["bias"]), action=q(outs["xa"][:, 2:]),
        ld_action=4, logp=q(outs["logp"]) if gauss else None, mean_out=None, obs_in=q(o["obs_in"]),
        obs_out=q(outs["xa"]) if o["obs_in"] is not None else None, log_std=None if gauss else q(o["log_std"]),
        min_log_std=float(torch.tensor(math.log(1e-6), dtype=torch.float32)))
