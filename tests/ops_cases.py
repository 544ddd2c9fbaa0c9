"""Cases, float64 references and derived bounds of the PointNet++ and chamfer ops (csrc/fps.hip, ball_query.hip,
group_gather.hip, interpolate.hip, nn_distance.hip, nms3d.hip), shared by tests/test_ops_reference_cpu.py (references
against the C oracle, no GPU) and tests/test_ops_sweep_gpu.py (kernels against the references).

The references are written from the DEFINITION of each operation in NumPy / torch float64, not from the oracle's code
(oracle/p2r_oracle.c restates the reference kernels line by line, by the same hand as the HIP kernels): a rule misread
the same way on both sides -- tie order, the strict `<`, the fill rule, the skip ball -- does not survive a third,
independent statement.

Bounds are derived, not tuned.  gamma(k) = k u / (1 - k u), u = 2^-24, k = the number of rounded fp32 operations a term
can pass on its way into a result (tests/sa_votes_cases.py):

  * squared distance (p2r_sqdist): three differences, three squares, two sums of non-negative terms.  A term passes its
    difference (whose error the square doubles: 2), its square (1) and at most two additions (2):
    |d32 - d64| <= gamma(5) d64.
  * a comparison of two such values is DECIDABLE when their float64 gap exceeds the sum of the two bounds; against
    r2 = fl32(fl32(r) fl32(r)), which the references use exactly as the kernels form it, when the gap exceeds the one
    bound.  On a quarter-integer cloud (`lattice`, `halflattice`) every operation of the distance is exact in fp32, so
    every comparison is decidable and ties are real ties.
  * three_interpolate: a product (1) and two additions: gamma(3) sum |p_i w_i|.
  * three_interpolate_grad: a destination with cnt contributions sums cnt rounded products in cnt - 1 additions (the
    addition to the initial zero is exact): k = cnt suffices, gamma(cnt + 1) sum |go w| is the stated bound.
  * group / gather gradient, order-free forms: cnt - 1 additions: gamma(cnt) sum |go|.  The deterministic forms are held
    to the fp32 sum in ascending slot order, bit for bit (`group_grad_ordered`).
  * nn_distance: see `NND_K`.
"""
import collections
import functools

import numpy as np
import torch

from tests import cases
from tests.sa_votes_cases import U, gamma, worst  # noqa: F401  (re-exported)

G5 = gamma(5)


def fl32(x):
    return float(np.float32(x))


def radius2(radius):
    """r2 as the kernels and the reference form it: the fp32 product of the fp32 radius with itself"""
    r = np.float32(radius)
    return float(np.float32(r * r))


def exact_cloud(*clouds):
    """every coordinate a multiple of 1/4 with |x| <= 64: differences, squares and their sums are exact in fp32"""
    return all(bool(torch.all((c.double() * 4).round() == c.double() * 4)) and
               (c.numel() == 0 or float(c.abs().max()) <= 64) for c in clouds)


def sqdist64(a, b):
    """a (B,P,3), b (B,Q,3) float32 -> (B,P,Q) float64 squared distances"""
    d = a.double()[:, :, None, :] - b.double()[:, None, :, :]
    return (d * d).sum(-1)


# ---- host selection rules, restated ------------------------------------------------------------------------------------------
def _cdiv(a, b):
    return (a + b - 1) // b


def group_sort_np(S):
    """(NP, SB) of the sort form: the key count padded to a power of two from 256 (group_gather.hip:282-283)"""
    NP, SB = 256, 8
    while NP < S:
        NP, SB = NP * 2, SB + 1
    return NP, SB


def group_grad_form(b, c, n, S):
    """The kernel `group_backward` picks (p2r_group_points_grad with S = npoints * nsample, p2r_gather_points_grad
    with S = npoints): 'sort8' | 'sort4' | 'scan16' | 'scan8' | 'scan4' | 'lds_gc16' .. 'lds_gc1' | 'atomic' | 'noop'.
    A Python restatement of csrc/group_gather.hip:272-325 (the LDS budget of 152 KiB, the 256 .. 4096 slot window and the
    31-bit key of the sort form, the 2^22 pair limit of the scan form, the 64 KiB rows and 512-workgroup rule of the
    LDS scatter).  It cannot see a later change of those lines: whoever moves a threshold there moves it here."""
    if b == 0 or c == 0 or n == 0:
        return "noop"
    SP = (S + 3) & ~3
    sp = max(SP, 4)
    fit = (152 * 1024) // (sp * 4)
    if S > 0 and fit >= 5:
        NP, SB = group_sort_np(S)
        if S >= 256 and NP <= 4096 and n <= (1 << (31 - SB)):
            gfit = (152 * 1024 - NP * 4) // (sp * 4)
            if gfit >= 8 and c > 4:
                return "sort8"
            if gfit >= 4:
                return "sort4"
        if n * sp <= (1 << 22):
            if fit >= 17 and c > 8:
                return "scan16"
            if fit >= 9 and c > 4:
                return "scan8"
            return "scan4"
    row = n * 4
    gc = 16
    while gc > 1 and gc * row > 64 * 1024:
        gc >>= 1
    while gc > 1 and b * _cdiv(c, gc) < 512 and gc > 4:
        gc >>= 1
    return "lds_gc%d" % gc if gc * row <= 64 * 1024 else "atomic"


GROUP_FORMS = {"sort8", "sort4", "scan16", "scan8", "scan4", "lds_gc16", "lds_gc8", "lds_gc4", "lds_gc2", "lds_gc1",
               "atomic"}
GROUP_ORDERED = {"sort8", "sort4", "scan16", "scan8", "scan4"}


def interp_grad_form(b, c, n, m):
    """The kernel p2r_three_interpolate_grad picks: 'lds_gc16' .. 'lds_gc1' | 'atomic' | 'noop'.  A Python restatement of
    csrc/interpolate.hip:196-202 (rows of m floats, 64 KiB of LDS, at least 512 workgroups before the chunk shrinks below
    four rows); it cannot see a later change of those lines."""
    if b == 0 or c == 0 or m == 0:
        return "noop"
    row = m * 4
    gc = 16
    while gc > 1 and gc * row > 64 * 1024:
        gc >>= 1
    while gc > 4 and b * _cdiv(c, gc) < 512:
        gc >>= 1
    return "lds_gc%d" % gc if gc * row <= 64 * 1024 else "atomic"


INTERP_FORMS = {"lds_gc16", "lds_gc8", "lds_gc4", "lds_gc2", "lds_gc1", "atomic"}

MI355X_CUS = 256


def fps_form(b, n, cus=MI355X_CUS):
    """The kernel p2r_furthest_point_sampling picks on a device of `cus` compute units: 'reg<W>x<PPT>_lds' (cloud copied
    to LDS, n * 12 bytes <= 64 KiB) | 'reg<W>x<PPT>_glb' | 'coop2' .. 'coop16' (G workgroups per cloud, points per
    workgroup S = ceil(n / G)) | 'stream'.  A Python restatement of csrc/fps.hip:346-352 and :370-404; it cannot see a
    later change of those lines, takes the scratch pointer as given and 8-byte aligned, and assumes the co-operative
    launch is placed (a refused one falls back to 'stream').  There is no 'coop1': n > 16384 on G <= 16 workgroups
    leaves S >= 1025."""
    for top, w, ppt in ((64, 1, 1), (128, 1, 2), (256, 1, 4), (512, 1, 8), (1024, 2, 8), (2048, 4, 8), (4096, 8, 8),
                        (8192, 16, 8), (16384, 16, 16)):
        if n <= top:
            return "reg%dx%d_%s" % (w, ppt, "lds" if n * 12 <= 64 * 1024 else "glb")
    G = 1
    while G * 2 <= 16 and b * G * 2 <= cus:
        G *= 2
    S = _cdiv(n, G)
    if G >= 2 and S <= 16384 and b * 4 * G * 8 <= b * n * 4:
        for top, ppt in ((2048, 2), (4096, 4), (8192, 8)):
            if S <= top:
                return "coop%d" % ppt
        return "coop16"
    return "stream"


FPS_FORMS = {"reg1x1_lds", "reg1x2_lds", "reg1x4_lds", "reg1x8_lds", "reg2x8_lds", "reg4x8_lds", "reg8x8_lds",
             "reg16x8_lds", "reg16x8_glb", "reg16x16_glb", "coop2", "coop4", "coop8", "coop16", "stream"}


# ---- furthest point sampling -----------------------------------------------------------------------------------------------
FpsCase = collections.namedtuple("FpsCase", "b n m kind seed form")


_FPS_N = [(64, "reg1x1_lds"), (65, "reg1x2_lds"), (128, "reg1x2_lds"), (129, "reg1x4_lds"), (256, "reg1x4_lds"),
          (257, "reg1x8_lds"), (512, "reg1x8_lds"), (513, "reg2x8_lds"), (1024, "reg2x8_lds"), (1025, "reg4x8_lds"),
          (2048, "reg4x8_lds"), (2049, "reg8x8_lds"), (4096, "reg8x8_lds"), (4097, "reg16x8_lds"), (5461, "reg16x8_lds"),
          (5462, "reg16x8_glb"), (8192, "reg16x8_glb"), (8193, "reg16x16_glb"), (16384, "reg16x16_glb")]


def _fps_cases():
    out = []
    for i, (n, form) in enumerate(_FPS_N):
        for kind in ("uniform", "lattice"):
            out.append(FpsCase(2 if n <= 1025 else 1, n, 16 if n <= 4097 else 8, kind, 300 + i, form))
    out.append(FpsCase(1, 16385, 6, "uniform", 330, "coop2"))      # 16 workgroups of 1025 points
    out.append(FpsCase(65, 16400, 4, "uniform", 331, "coop16"))    # 2 workgroups of 8200 points
    out.append(FpsCase(129, 16385, 3, "uniform", 332, "stream"))   # more clouds than half the compute units
    return out


FPS_SWEEP = _fps_cases()


def fps_check(xyz, picks):
    """The picks (B,m) of furthest point sampling against the float64 running min-distance.  A point is live when its
    fp32 |p|^2 is not below 1e-3f.  Asserts: picks[:, 0] == 0; every pick in [0, n); in every round the pick is live
    (unless no point is) and its float64 min-distance is >= (1 - 2 gamma(5)) times the round's largest -- the fp32
    running minimum of point k lies within gamma(5) of its float64 value, and the pick's fp32 value is not below the
    float64 winner's --; in a round whose top two values are decidable the pick is the float64 arg-max.  On an exact
    cloud the pick's float64 value EQUALS the maximum (which of several equal points wins is the reference's
    block-size rule, pinned by the oracle equality).  Returns (rounds, undecidable rounds)."""
    B, n, _ = xyz.shape
    m = picks.shape[1]
    x32 = xyz.numpy()
    mag = (x32[..., 0] * x32[..., 0]) + (x32[..., 1] * x32[..., 1]) + (x32[..., 2] * x32[..., 2])
    live = torch.from_numpy(mag >= np.float32(1e-3))
    exact = exact_cloud(xyz)
    p = picks.long()
    assert bool((p[:, 0] == 0).all()), "the first pick is point 0"
    assert bool(((p >= 0) & (p < n)).all()), "a pick outside [0, n)"
    x = xyz.double()
    md = torch.full((B, n), float("inf"), dtype=torch.float64)
    rounds = undecidable = 0
    rows = torch.arange(B)
    for j in range(1, m):
        old = x[rows, p[:, j - 1]]                                    # (B,3)
        d = ((x - old[:, None, :]) ** 2).sum(-1)
        md = torch.minimum(md, d)
        cand = torch.where(live, md, torch.full_like(md, -1.0))
        top2, arg2 = torch.topk(cand, min(2, n), dim=1)
        for bi in range(B):
            if not bool(live[bi].any()):
                continue
            rounds += 1
            pk = int(p[bi, j])
            mx = float(top2[bi, 0])
            second = float(top2[bi, 1]) if n > 1 else -1.0
            assert bool(live[bi, pk]), f"round {j} cloud {bi}: pick {pk} lies in the skip ball"
            got = float(md[bi, pk])
            if exact:
                assert got == mx, f"round {j} cloud {bi}: pick {pk} at {got!r}, maximum {mx!r} (exact cloud)"
                continue
            assert got >= (1 - 2 * G5) * mx, f"round {j} cloud {bi}: pick {pk} at {got!r}, maximum {mx!r}"
            if second < 0 or mx - second > G5 * (mx + second):
                assert pk == int(arg2[bi, 0]), f"round {j} cloud {bi}: pick {pk}, float64 arg-max {int(arg2[bi, 0])}"
            else:
                undecidable += 1
    return rounds, undecidable


# ---- ball query ------------------------------------------------------------------------------------------------------------
BallCase = collections.namedtuple("BallCase", "name b n m radius nsample kind seed")
BALL_SWEEP = [
    BallCase("n2047", 1, 2047, 15, 0.4, 63, "uniform", 401),        # one LDS tile, one point short
    BallCase("n2048", 1, 2048, 16, 0.4, 64, "uniform", 402),        # exactly one tile, one full workgroup of centres
    BallCase("n2049", 2, 2049, 17, 0.4, 65, "uniform", 403),        # a second tile of one point, a second workgroup
    BallCase("n4097_m1", 1, 4097, 1, 1.0, 130, "uniform", 404),     # three tiles, > 130 hits, three fill trips
    BallCase("n4097_s1", 1, 4097, 17, 0.3, 1, "uniform", 405),      # nsample 1: stop at the first hit
    BallCase("sparse130", 1, 2049, 16, 0.3, 130, "uniform", 406),   # few hits, the fill rule over 130 slots
    BallCase("half_r050", 1, 600, 16, 0.5, 16, "halflattice", 407),  # d2 == r2 = 0.25 exactly: excluded
    BallCase("half_r075", 1, 2049, 17, 0.75, 130, "halflattice", 408),  # d2 == 0.5625 exactly
    BallCase("latt_r1", 2, 300, 15, 1.0, 65, "lattice", 409),       # d2 == 1 exactly, duplicates
    BallCase("straddle", 1, 4097, 2, 0.05, 32, "straddle", 410),    # hits 2040 .. 2055: both sides of the tile edge
    BallCase("empty", 1, 300, 3, 0.3, 16, "empty", 411),            # no hit: rows of zeros
]
BALL_BY_NAME = {c.name: c for c in BALL_SWEEP}


@functools.lru_cache(maxsize=None)
def ball_inputs(name):
    """(xyz (b,n,3), new_xyz (b,m,3)) of a ball-query case.  Cached: do not write into them."""
    c = BALL_BY_NAME[name]
    kind = c.kind if c.kind in ("uniform", "lattice", "halflattice") else "uniform"
    xyz = cases.cloud(c.b, c.n, c.seed, kind)
    new_xyz = cases.centres_from(xyz, c.m, c.seed)
    if c.kind == "straddle":
        g = torch.Generator().manual_seed(c.seed)
        centre = torch.tensor([1.25, -0.5, 0.75])
        xyz[:, 2040:2056] = centre + 0.01 * torch.randn(c.b, 16, 3, generator=g)
        new_xyz[:, 0] = centre
    if c.kind == "empty":
        new_xyz = new_xyz + 100.0
    return xyz.contiguous(), new_xyz.contiguous()


def ball_query_ref(xyz, new_xyz, radius, nsample):
    """-> (idx (b,m,nsample) int32, undecidable comparisons).  Per centre: the points with d2 < r2 in ascending order,
    the first `nsample` of them, the remaining slots filled with the first hit, zeros for a ball without a hit."""
    r2 = radius2(radius)
    d = sqdist64(new_xyz, xyz)                                        # (b,m,n)
    undec = 0 if exact_cloud(xyz, new_xyz) else int(((d - r2).abs() <= G5 * d).sum())
    hit = d < r2
    b, m, _ = d.shape
    idx = torch.zeros(b, m, nsample, dtype=torch.int32)
    for bi in range(b):
        for j in range(m):
            h = hit[bi, j].nonzero().flatten()[:nsample]
            if h.numel():
                idx[bi, j] = h[0]
                idx[bi, j, :h.numel()] = h
    return idx, undec


# ---- three_nn --------------------------------------------------------------------------------------------------------------
NnCase = collections.namedtuple("NnCase", "b n m kind seed")
THREE_NN_SWEEP = [
    NnCase(1, 255, 0, "uniform", 501), NnCase(2, 256, 1, "uniform", 502), NnCase(1, 257, 2, "uniform", 503),
    NnCase(2, 255, 3, "uniform", 504), NnCase(1, 256, 1023, "uniform", 505), NnCase(2, 257, 1024, "uniform", 506),
    NnCase(1, 255, 1025, "uniform", 507),                       # a second LDS tile of one point
    NnCase(2, 257, 300, "lattice", 508), NnCase(1, 256, 1025, "halflattice", 509), NnCase(1, 255, 2, "lattice", 510),
]


@functools.lru_cache(maxsize=None)
def three_nn_inputs(case):
    unknown = cases.cloud(case.b, case.n, case.seed, case.kind)
    known = cases.cloud(case.b, case.m, case.seed + 50, case.kind) if case.m > 0 else torch.zeros(case.b, 0, 3)
    return unknown, known


def three_nn_ref(unknown, known):
    """-> (dist2 (b,n,3) float64, idx (b,n,3) int32, undecidable comparisons): the three smallest squared distances in
    the order of a stable sort by (d2, k); with m < 3 known points the empty slots are +inf with index 0."""
    b, n, _ = unknown.shape
    m = known.shape[1]
    dist = torch.full((b, n, 3), float("inf"), dtype=torch.float64)
    idx = torch.zeros(b, n, 3, dtype=torch.int32)
    if m == 0:
        return dist, idx, 0
    d = sqdist64(unknown, known)
    sd, si = torch.sort(d, dim=2, stable=True)
    k = min(m, 3)
    dist[:, :, :k] = sd[:, :, :k]
    idx[:, :, :k] = si[:, :, :k].int()
    undec = 0
    if not exact_cloud(unknown, known):
        top = sd[:, :, :4]                                           # the order of the first three against each other and the 4th
        gap = top[:, :, 1:] - top[:, :, :-1]
        undec = int((gap <= G5 * (top[:, :, 1:] + top[:, :, :-1])).sum())
    return dist, idx, undec


# ---- three_interpolate and its gradient ------------------------------------------------------------------------------------------
InterpCase = collections.namedtuple("InterpCase", "b c n m idx_kind seed form")
INTERP_SWEEP = [
    InterpCase(1, 3, 50, 16384, "rand", 601, "lds_gc1"),       # one row fills the 64 KiB
    InterpCase(1, 3, 50, 16385, "rand", 602, "atomic"),
    InterpCase(1, 3, 50, 8192, "rand", 603, "lds_gc2"),
    InterpCase(2, 7, 300, 100, "rand", 604, "lds_gc4"),
    InterpCase(512, 1, 3, 1025, "rand", 605, "lds_gc8"),       # 512 workgroups keep the 8-row chunk
    InterpCase(600, 16, 5, 8, "rand", 606, "lds_gc16"),
    InterpCase(1, 5, 200, 40, "pair", 607, "lds_gc4"),         # i1 == i2 in every second triple
    InterpCase(1, 3, 700, 20, "one", 608, "lds_gc4"),          # all 2100 contributions on one destination
    InterpCase(1, 2, 40, 16385, "one", 609, "atomic"),
]


@functools.lru_cache(maxsize=None)
def interp_inputs(case):
    """(points (b,c,m), idx (b,n,3) int32, weight (b,n,3), grad_out (b,c,n))"""
    g = torch.Generator().manual_seed(case.seed)
    pts = torch.randn(case.b, case.c, case.m, generator=g)
    idx = torch.randint(0, case.m, (case.b, case.n, 3), generator=g, dtype=torch.int32)
    if case.idx_kind == "pair":
        idx[:, ::2, 1] = idx[:, ::2, 0]
    if case.idx_kind == "one":
        idx[:] = case.m - 3
    w = torch.rand(case.b, case.n, 3, generator=g) + 0.01
    w = (w / w.sum(-1, keepdim=True)).contiguous()
    go = torch.randn(case.b, case.c, case.n, generator=g)
    return pts, idx.contiguous(), w, go


def three_interpolate_ref(pts, idx, w):
    """-> (out (b,c,n) float64, bound): out[b,l,j] = sum_i pts[b,l,idx[b,j,i]] w[b,j,i]"""
    b, c, m = pts.shape
    n = idx.shape[1]
    ii = idx.long().reshape(b, 1, n * 3).expand(b, c, n * 3)
    terms = torch.gather(pts.double(), 2, ii).reshape(b, c, n, 3) * w.double()[:, None]
    return terms.sum(-1), gamma(3) * terms.abs().sum(-1)


def three_interpolate_grad_ref(go, idx, w, m):
    """-> (grad (b,c,m) float64, bound, cnt (b,m)): the float64 scatter of go[b,l,j] w[b,j,i] to idx[b,j,i]"""
    b, c, n = go.shape
    ii = idx.long().reshape(b, n * 3)
    terms = (go.double()[:, :, :, None] * w.double()[:, None]).reshape(b, c, n * 3)
    grad = torch.zeros(b, c, m, dtype=torch.float64).scatter_add_(2, ii[:, None].expand(b, c, n * 3), terms)
    mag = torch.zeros(b, c, m, dtype=torch.float64).scatter_add_(2, ii[:, None].expand(b, c, n * 3), terms.abs())
    cnt = torch.zeros(b, m, dtype=torch.float64).scatter_add_(1, ii, torch.ones(b, n * 3, dtype=torch.float64))
    k = cnt + 1
    return grad, (k * U / (1 - k * U))[:, None] * mag, cnt


# ---- group_points / gather_points and their gradient -------------------------------------------------------------------------
GroupCase = collections.namedtuple("GroupCase", "b c n S idx_kind op seed form")
_G = GroupCase
GROUP_SWEEP = [
    _G(1, 9, 300, 256, "rand", "group", 701, "sort8"),          # NP = 256, the first sorted length; 8 + 1 rows
    _G(1, 9, 300, 255, "rand", "group", 702, "scan16"),         # one slot short of the sort form
    _G(1, 9, 300, 257, "rand", "group", 703, "sort8"),          # NP = 512 for 257 keys, S % 4 == 1
    _G(1, 5, 300, 4096, "rand", "group", 704, "sort8"),         # NP = 4096, 5 of 8 rows
    _G(1, 5, 300, 4097, "rand", "group", 705, "scan8"),         # past the sort window
    _G(1, 5, 64, 4093, "rand", "group", 706, "sort8"),          # S % 4 != 0: three padded slots
    _G(2, 3, 512, 2045, "rand", "group", 707, "sort4"),         # S % 4 != 0, two clouds
    _G(1, 4, 50, 37, "rand", "group", 708, "scan4"),
    _G(1, 8, 50, 37, "rand", "group", 709, "scan8"),
    _G(1, 9, 50, 37, "rand", "group", 710, "scan16"),
    _G(1, 6, 1000, 5000, "rand", "group", 711, "lds_gc4"),
    _G(1, 5, 16384, 7800, "rand", "group", 712, "lds_gc1"),
    _G(1, 3, 16385, 7800, "rand", "group", 713, "atomic"),
    _G(1, 2, 42000, 100, "rand", "group", 714, "atomic"),       # short list, long rows
    _G(1, 3, 5000, 4097, "rand", "group", 715, "lds_gc2"),
    _G(512, 1, 1025, 4100, "rand", "group", 716, "lds_gc8"),    # 512 workgroups keep the 8-row chunk
    _G(512, 1, 1024, 4100, "rand", "group", 717, "lds_gc16"),   # 16 rows of 1024 floats: the whole 64 KiB
    # all S slots on one destination, per deterministic form
    _G(1, 9, 300, 256, "one", "group", 720, "sort8"),
    _G(1, 3, 64, 300, "one", "group", 721, "sort4"),
    _G(1, 4, 50, 37, "one", "group", 722, "scan4"),
    _G(1, 8, 50, 37, "one", "group", 723, "scan8"),
    _G(1, 9, 50, 37, "one", "group", 724, "scan16"),
    # most destinations never hit
    _G(1, 9, 700, 260, "sparse", "group", 725, "sort8"),
    _G(1, 6, 1000, 5000, "sparse", "group", 726, "lds_gc4"),
    # more destinations than the 512 threads of a workgroup
    _G(1, 5, 513, 300, "rand", "group", 727, "sort8"),
    _G(1, 9, 1025, 100, "rand", "group", 728, "scan16"),
    # gather_points_grad: the same dispatcher with S = npoints
    _G(1, 9, 300, 257, "rand", "gather", 730, "sort8"),
    _G(2, 3, 512, 128, "rand", "gather", 731, "scan4"),
    _G(1, 2, 42000, 100, "rand", "gather", 732, "atomic"),
    _G(1, 6, 1000, 5000, "rand", "gather", 733, "lds_gc4"),
]


def group_split(S):
    """(npoints, nsample) with npoints * nsample == S; the kernels see the product only"""
    for ns in (16, 5, 3):
        if S % ns == 0:
            return S // ns, ns
    return S, 1


@functools.lru_cache(maxsize=None)
def group_inputs(case):
    """(points (b,c,n), idx (b,S) int32, grad_out (b,c,S)); callers view idx / grad_out as (npoints, nsample)"""
    g = torch.Generator().manual_seed(case.seed)
    pts = torch.randn(case.b, case.c, case.n, generator=g)
    if case.idx_kind == "one":
        idx = torch.full((case.b, case.S), case.n - 2, dtype=torch.int32)
    elif case.idx_kind == "sparse":
        few = torch.tensor([0, case.n // 2 + 1, case.n - 1], dtype=torch.int32)
        idx = few[torch.randint(0, 3, (case.b, case.S), generator=g)]
    else:
        idx = torch.randint(0, case.n, (case.b, case.S), generator=g, dtype=torch.int32)
    go = torch.randn(case.b, case.c, case.S, generator=g)
    return pts, idx.contiguous(), go


def group_forward_ref(pts, idx):
    """points (b,c,n), idx (b,S) -> (b,c,S): out[b,l,s] = points[b,l,idx[b,s]]"""
    b, c, _ = pts.shape
    return torch.gather(pts, 2, idx.long()[:, None].expand(b, c, idx.shape[1]))


def group_grad_ref(go, idx, n):
    """-> (grad (b,c,n) float64, bound of the order-free forms, cnt (b,n))"""
    b, c, S = go.shape
    ii = idx.long()
    ie = ii[:, None].expand(b, c, S)
    grad = torch.zeros(b, c, n, dtype=torch.float64).scatter_add_(2, ie, go.double())
    mag = torch.zeros(b, c, n, dtype=torch.float64).scatter_add_(2, ie, go.double().abs())
    cnt = torch.zeros(b, n, dtype=torch.float64).scatter_add_(1, ii, torch.ones(b, S, dtype=torch.float64))
    return grad, (cnt * U / (1 - cnt * U))[:, None] * mag, cnt


def group_grad_ordered(go, idx, n):
    """The fp32 sum of every destination in ascending slot order, one rounding per addition: what the deterministic
    forms (sort, scan) return bit for bit."""
    g = go.numpy()
    ii = idx.numpy()
    b, c, S = g.shape
    out = np.zeros((b, c, n), dtype=np.float32)
    for bi in range(b):
        for s in range(S):
            k = ii[bi, s]
            out[bi, :, k] = out[bi, :, k] + g[bi, :, s]
    return torch.from_numpy(out)


# ---- nn_distance -----------------------------------------------------------------------------------------------------------
NND_MODES = {"l2": {}, "l1": {"l1": True}, "huber1": {"l1smooth": True}, "huber03": {"l1smooth": True, "delta": 0.3}}


def NND_K(mode, C):
    """Rounded operations a term of one pair's distance passes.  l2: difference (doubled by the square) 2, square 1,
    C - 1 additions: C + 2.  l1: difference 1, C - 1 additions: C.  Huber h(x) = q^2 / 2 + delta (|x| - q),
    q = min(|x|, delta): x h'(x) / h(x) <= 2, so the rounded difference costs 2; then q^2, |x| - q, the product
    with delta and the sum of the two parts, one each (halving is exact): 6, and C - 1 additions: C + 5."""
    return {"l2": C + 2, "l1": C}.get(mode, C + 5)


NndCase = collections.namedtuple("NndCase", "B N M C kind seed")
NND_SWEEP = [
    NndCase(2, 17, 9, 1, "randn", 801), NndCase(2, 9, 17, 2, "randn", 802), NndCase(3, 33, 20, 3, "randn", 803),
    NndCase(2, 20, 33, 4, "randn", 804), NndCase(2, 1, 7, 3, "randn", 805), NndCase(2, 7, 1, 4, "randn", 806),
    NndCase(1, 1, 1, 1, "randn", 807),
    NndCase(2, 40, 30, 3, "lattice", 808), NndCase(2, 30, 40, 2, "lattice", 809), NndCase(2, 50, 10, 1, "lattice", 810),
    NndCase(1, 25, 25, 4, "halflattice", 811),
    NndCase(2, 12, 10, 3, "ondelta", 812), NndCase(2, 10, 12, 2, "ondelta", 813),
]
# quarter-integer inputs are exact (and their ties real) only where delta is one of them: fl32(0.3) times a lattice value rounds
NND_COMBOS = [(c, mode) for c in NND_SWEEP for mode in NND_MODES
              if not (mode == "huber03" and c.kind in ("lattice", "halflattice"))]


def nnd_delta(mode):
    return fl32(NND_MODES[mode].get("delta", 1.0))


@functools.lru_cache(maxsize=None)
def nnd_inputs(case, mode):
    """(pc1 (B,N,C), pc2 (B,M,C), g1 (B,N), g2 (B,M)).  'ondelta': pc2 carries exact zeros in channel 0 of its first rows
    and pc1 there +-delta as fp32, so the fp32 difference IS delta; pc1 row 1 copies pc2 row 1 (diff == 0)."""
    B, N, M, C, kind, seed = case
    g = torch.Generator().manual_seed(seed)
    if kind in ("lattice", "halflattice"):
        lo, hi, sc = (-3, 4, 1.0) if kind == "lattice" else (-8, 9, 0.25)
        a = torch.randint(lo, hi, (B, N, C), generator=g).float() * sc
        q = torch.randint(lo, hi, (B, M, C), generator=g).float() * sc
    else:
        a = torch.randn(B, N, C, generator=g)
        q = torch.randn(B, M, C, generator=g)
    if kind == "ondelta":
        d = nnd_delta(mode)
        q[:, :4, 0] = 0.0
        a[:, 0, 0] = d
        a[:, 2, 0] = -d
        a[:, 1] = q[:, 1]
        q[:, 5] = a[:, 5]
    g1 = torch.randn(B, N, generator=g)
    g2 = torch.randn(B, M, generator=g)
    return a.contiguous(), q.contiguous(), g1, g2


def nnd_exact(case, mode):
    return case.kind in ("lattice", "halflattice") and mode != "huber03"


def _nnd_term(diff, mode, delta):
    if mode == "l2":
        return diff * diff
    if mode == "l1":
        return diff.abs()
    q = diff.abs().clamp(max=delta)
    return 0.5 * q * q + delta * (diff.abs() - q)


def _nnd_dterm(diff, mode, delta):
    if mode == "l2":
        return 2 * diff
    if mode == "l1":
        return torch.sign(diff)
    return torch.where(diff.abs() <= delta, diff, delta * torch.sign(diff))


def nnd_matrix(a, q, mode):
    """(B,N,M) float64: the distance of every pair, summed over the channels"""
    diff = a.double()[:, :, None, :] - q.double()[:, None, :, :]
    return _nnd_term(diff, mode, nnd_delta(mode)).sum(-1)


def nnd_ref(a, q, mode, exact=False):
    """-> (dist1 (B,N), idx1, dist2 (B,M), idx2, bound1, bound2, undecidable): the minimum over the other cloud and its
    FIRST minimal index; undecidable = rows whose two smallest values are closer than their two bounds (exact inputs:
    none, equal values are ties and the first index wins)"""
    D = nnd_matrix(a, q, mode)
    gk = gamma(NND_K(mode, a.shape[2]))
    out, undec = [], 0
    for dim in (2, 1):
        dist = D.min(dim=dim).values
        ismin = D == dist.unsqueeze(dim)
        first = ismin.int().argmax(dim=dim)                          # argmax returns the first maximal element
        if not exact and D.shape[dim] > 1:
            two = torch.topk(D, 2, dim=dim, largest=False).values
            a0, a1 = two.select(dim, 0), two.select(dim, 1)
            undec += int((a1 - a0 <= gk * (a1 + a0)).sum())
        out += [dist, first]
    return out[0], out[1], out[2], out[3], gk * out[0], gk * out[2], undec


def nnd_grad_ref(a, q, idx1, idx2, g1, g2, mode):
    """Gather form of the gradient in float64 with GIVEN arg-min indices: the cotangent of dist1[i] goes to the pair
    (i, idx1[i]), that of dist2[j] to (idx2[j], j).  -> (grad_pc1, grad_pc2, bound1, bound2); the bound of a row with cnt
    contributions is gamma(cnt + 1) sum |g dterm|: the difference (1; doubling it is exact, and where fp32 and float64
    fall on different sides of |diff| = delta the two branches differ by that same rounding), the product with g (1),
    cnt - 1 additions."""
    delta = nnd_delta(mode)
    A, Q = a.double(), q.double()
    B, N, C = A.shape
    M = Q.shape[1]
    ga = torch.zeros(B, N, C, dtype=torch.float64); ma = torch.zeros_like(ga)
    gq = torch.zeros(B, M, C, dtype=torch.float64); mq = torch.zeros_like(gq)
    ca = torch.zeros(B, N, dtype=torch.float64); cq = torch.zeros(B, M, dtype=torch.float64)
    for b in range(B):
        pairs = [(i, int(idx1[b, i]), float(g1[b, i])) for i in range(N)] + \
                [(int(idx2[b, j]), j, float(g2[b, j])) for j in range(M)]
        for i, j, g in pairs:
            t = g * _nnd_dterm(A[b, i] - Q[b, j], mode, delta)
            ga[b, i] += t; gq[b, j] -= t
            ma[b, i] += t.abs(); mq[b, j] += t.abs()
            ca[b, i] += 1; cq[b, j] += 1
    ka, kq = ca + 1, cq + 1
    return ga, gq, (ka * U / (1 - ka * U))[..., None] * ma, (kq * U / (1 - kq * U))[..., None] * mq


def nnd_autograd(a, q, g1, g2, mode):
    """The reference formula (materialised (B,N,M,C) difference, two torch.min) in float64 under torch autograd"""
    A = a.double().requires_grad_(True)
    Q = q.double().requires_grad_(True)
    D = _nnd_term(A[:, :, None, :] - Q[:, None, :, :], mode, nnd_delta(mode)).sum(-1)
    d1, i1 = torch.min(D, dim=2)
    d2, i2 = torch.min(D, dim=1)
    ((d1 * g1.double()).sum() + (d2 * g2.double()).sum()).backward()
    return i1, i2, A.grad, Q.grad


# ---- nms3d -----------------------------------------------------------------------------------------------------------------
NmsCase = collections.namedtuple("NmsCase", "name K kind thr old_type same_cls valid seed")
NMS_SWEEP = [
    NmsCase("k63_ties", 63, "ties", 0.1, False, False, None, 901),
    NmsCase("k64_ties_old", 64, "ties", 0.25, True, False, None, 902),
    NmsCase("k65_ties_cls", 65, "ties", 0.1, False, True, None, 903),
    NmsCase("k1023_ties", 1023, "ties", 0.25, False, False, None, 904),
    NmsCase("k1024_ties_old_cls", 1024, "ties", 0.1, True, True, None, 905),
    NmsCase("k64_allequal", 64, "allequal", 0.1, False, False, None, 906),
    NmsCase("k65_chain", 65, "chain", 0.25, False, False, None, 907),
    NmsCase("k64_chain_tied", 64, "chain_tied", 0.25, False, False, None, 908),
    NmsCase("k1024_chain_old", 1024, "chain_tied", 0.25, True, False, None, 909),
    NmsCase("k65_valid_some", 65, "ties", 0.1, False, False, "some", 910),
    NmsCase("k64_valid_one", 64, "ties", 0.1, False, True, "one", 911),
    NmsCase("k63_valid_none", 63, "ties", 0.25, True, False, "none", 912),
]
NMS_BY_NAME = {c.name: c for c in NMS_SWEEP}


@functools.lru_cache(maxsize=None)
def nms_inputs(name):
    """(boxes (K,8) float64 rows [x1,y1,z1,x2,y2,z2,score,cls], valid (K,) bool or None)"""
    c = NMS_BY_NAME[name]
    K = c.K
    rng = np.random.default_rng(c.seed)
    if c.kind in ("chain", "chain_tied"):
        # unit cubes half a unit apart on x: each overlaps its neighbours only (IoU 1/3, old-type 1/2), so in pick order
        # every kept box suppresses the next one
        x1 = 0.5 * np.arange(K, dtype=np.float64)
        lo = np.stack([x1, np.zeros(K), np.zeros(K)], 1)
        hi = lo + 1.0
        score = np.full(K, 0.5) if c.kind == "chain_tied" else 1.0 - np.arange(K) / (2.0 * K)
        cls = np.zeros(K)
    else:
        ctr = rng.uniform(-1.5, 1.5, (K, 3)) * (K / 64.0) ** (1 / 3)
        size = rng.uniform(0.3, 1.5, (K, 3))
        lo, hi = ctr - size / 2, ctr + size / 2
        score = np.full(K, 0.75) if c.kind == "allequal" else rng.integers(0, 4, K) / 4.0   # many exact ties
        cls = rng.integers(0, 3, K).astype(np.float64)
    boxes = np.ascontiguousarray(np.concatenate([lo, hi, score[:, None], cls[:, None]], 1))
    valid = None
    if c.valid == "some":
        valid = rng.uniform(size=K) < 0.6
    elif c.valid == "one":
        valid = np.zeros(K, bool); valid[K // 3] = True
    elif c.valid == "none":
        valid = np.zeros(K, bool)
    return boxes, valid


def nms3d_ref(boxes, thr, old_type=False, same_cls=False, valid=None):
    """Greedy non-maximum suppression in float64, from the rule: visit the (valid) boxes by descending score, equal
    scores by DESCENDING index; a visited box that is still alive is picked and removes every later box whose overlap
    with it exceeds thr (strictly).  Overlap: intersection volume over the union, or (old_type) over the LATER box's own
    volume; with same_cls only boxes of the pick's class are removed.  -> picked indices in pick order."""
    K = len(boxes)
    take = [k for k in range(K) if valid is None or valid[k]]
    order = sorted(take, key=lambda k: (-boxes[k, 6], -k))
    vol = [(boxes[k, 3] - boxes[k, 0]) * (boxes[k, 4] - boxes[k, 1]) * (boxes[k, 5] - boxes[k, 2]) for k in range(K)]
    alive = {k: True for k in order}
    picks = []
    for pos, i in enumerate(order):
        if not alive[i]:
            continue
        picks.append(i)
        for r in order[pos + 1:]:
            if not alive[r] or (same_cls and boxes[i, 7] != boxes[r, 7]):
                continue
            ext = [max(0.0, min(boxes[i, 3 + a], boxes[r, 3 + a]) - max(boxes[i, a], boxes[r, a])) for a in range(3)]
            inter = ext[0] * ext[1] * ext[2]
            o = inter / vol[r] if old_type else inter / (vol[i] + vol[r] - inter)
            if o > thr:
                alive[r] = False
    return picks


@functools.lru_cache(maxsize=None)
def nms_expected(name):
    """the picks of case `name` by `nms3d_ref`, computed once"""
    c = NMS_BY_NAME[name]
    boxes, valid = nms_inputs(name)
    return tuple(nms3d_ref(boxes, c.thr, c.old_type, c.same_cls, valid))
