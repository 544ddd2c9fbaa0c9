"""Cases, float64 references with per-element bounds, exact families, torch emulators and mutants of the split16 ST-GCN
kernels (csrc/split16.h, stgcn_gcn3h_body.h with stgcn_gcn3h_fwd.hip / stgcn_gcn3h_dx.hip, stgcn_gcn3dwh.hip,
stgcn_gcn3h_grad.hip, stgcn_tconvh.hip), shared by tests/test_split16_reference_cpu.py and tests/test_split16_sweep_gpu.py.
U, gamma, worst, check_bound, the adjacency tables, the operand families and the epilogue references are those of
tests/stgcn_cases.py (imported, not copied).

Every reference is plain float64 torch on the kernel's OWN fp32 stage input (statistics and BatchNorm-backward sums on the
device's stored result).  Next to every value comes a bound E = fp32 part + two-part part, per element:

fp32 part: gamma(k) times the same expression on absolute values, k = the largest number of rounded fp32 operations a term
can pass (stgcn_cases' convention: every product and every accumulation of an MFMA counts once, whatever the MFMA does
inside a k-step), read from the split kernels:
  * gcn3h forward / data gradient: the aggregate is one product and an fmaf chain over the list (LMAX roundings; the scale
    2^S_x rides in the coefficient table: exact), split into two parts, then every term is THREE products into ONE
    accumulator (h3_mfma12): 3 * 64 K accumulations; the bias table enters scaled by a power of two (exact), the
    accumulators leave through one (exact), the addend is one more addition: K_GCNH = LMAX + 1 + 3 * 64 K + 1.
  * gcn3dwh: V_k (fmaf chain, LMAX + 1), three products per column into one accumulator, a workgroup adds
    56 (53 joints + 3 zero slots) x 4 frames x ceil(tiles / n_blocks) columns: k = LMAX + 1 + 3 * 224 w; the rows are summed in
    float64 by the test.  The bias-table sums are stgcn_cases' colsum: (d0 + d1) + (d2 + d3), one addition per tile.
  * gcn3h_coef_grad: Y_k = W_k x is 64 terms x three products into one accumulator (d3_product): gamma(3 * 64 + 1) on
    |W_k| |x|; the reduction against dz is stgcn_gcn3_dcoef_body.h's, k_d = 13 + 4 tiles per workgroup (stgcn_cases).
  * tconvh: h = fmed3(fmaf(x, scale, shift), 0, 65504) is one rounding (x * 2^S_x without a transform: exact); per output the
    accumulator `lo` takes 2 * 192 products, `hi` 192; hi + lo, then fmaf(., 2^-S, bias): K_TCH = 2 * 192 + 3.

two-part part (split16.h; all magnitudes at the operand's SCALED range, max |x| 2^S in [2^12, 2^13)):
  * a1 = fp16(a) errs by 2^-11 |a| (half an ulp of 11 bits) while it is a normal number, the residual r = a - a1 is exact in
    fp32, a2 = fp16(r) errs by 2^-11 |r| <= 2^-22 |a| while normal: |a - a1 - a2| <= 2^-22 |a|.
  * where a part is an fp16 subnormal (below 2^-14) its error is absolute, half the subnormal grid: 2^-25.  Plain residual
    (the forward's aggregate, x of gcn3dwh and of gcn3h_coef_grad, every host-split weight): |a - a1 - a2| <= 2^-22 |a| +
    2^-25.  Scaled residual (H3_RES_SCALED, tconvh, the aggregate of gcn3dwh): a2' = fp16(2^11 r), so the floor is 2^11
    lower, 2^-36, at the same range.
  * the third weight plane 2^-11 w1 is exact while it is normal (|w1| >= 2^-3); below, it is rounded to the subnormal grid,
    2^-25, and meets b2' = 2^11 b2 with |b2| <= 2^-11 |b| + floor: one more 2^-25 |b|.
  * the dropped term: |w2| <= 2^-11 |w| + 2^-24 and |b2| <= 2^-11 |b| + 2^-25 give |w2 b2| <= 2^-22 |w| |b| + 2^-36 |w| +
    2^-35 |b| + 2^-49.
  Together, per term w b with computed parts (w1 b1 + w1' b2' + w2 b1) = (w + dw)(b + db) - w2 b2:
      |error| <= 3 * 2^-22 (1 + 2^-9) |w| |b| + F_W |b| + F_B |w| + F_W F_B
  with F_W = 2^-23 (2^-25 of the split + 2^-25 of the third plane + 2^-35, rounded up) and F_B = 2^-24 (plain: 2^-25 + 2^-36)
  or 2^-35 (scaled: 2^-36 + 2^-36), both at the scaled ranges: divided by 2^S_w / 2^S_x they are at most 2^-35 max |W| and
  2^-36 max |x| (plain) or 2^-47 max |x| (scaled) -- relative to the TENSOR's maximum for the plain residual, 2^11 lower
  with H3_RES_SCALED and in tconvh.  No constant is fitted.  The (1 + 2^-9) covers the second-order terms and the fp32
  error of the aggregate inside |b|.
  Without a range word (x_amax NULL, the forward form of tconvh) S_x = 0 and the floors are absolute.

epilogues: gcn3h's (count, mean, M2) is stgcn_gcn3.hip's on the scaled accumulators, the scale leaves by a power of two:
stgcn_cases.stats3_ref as it is.  tconvh keeps ONE pivot per channel and workgroup (the mean of the first frame's first
16 columns), a lane adds 4 column tiles x chunk frames, then four row16 additions: k_s = 1 + 4 chunk + 4, and with
D = (hi - lo) + gamma(5) M as in stgcn_cases E_mean = gamma(k_s + 1) D + u (M + D), E_M2 = gamma(3 k_s + 8) n D^2.  Its
BatchNorm-backward sums: k = 4 chunk + 5 (sum g), 4 chunk + 8 (z - mean, fmaf, the product with invstd).

EXACT families (no bound at all): under the conditions that test_split16_reference_cpu.py asserts from the float64
reference and the host split alone -- every scaled operand finite in fp16, no value-carrying part subnormal, the dropped
term identically zero, the float64 sum of absolute PART products of every output below 2^24 units -- every product and
every partial sum in every order is exactly representable and the fp32 result must EQUAL the float64 value:
  E0  operands small integers (maximum 2 in every tensor: the range word is known), weights {0, +-0.5, +-1}, coefficients
      {+-0.5, +-1, +-2} at the real entries: all residuals zero (stgcn_cases' exact family as it is).
  EW  weights P + R with 14 significant bits (P 11 bits, |R| below half a step of P: w1 = P, w2 = R != 0), operands of E0:
      pins every a2 b1 product and the w2 plane of every pair and phase.
  EX  operands +-(P + R) 2^-10 with P in [1024, 2047], R in {+-1/8, +-1/4, +-3/8}: scaled by 2^12 p = 4 P and the residual 4 R
      is alive (q' = 2^13 R, normal); weights fp16-exact with 2^-11 w1 normal; ONE non-zero coefficient per list, so the
      aggregate is c x exactly.  Pins a1' b2' and the 2^11 bookkeeping (the forward, plain residuals: a1 b2).
For the weight gradient the product is x (A operand, plain residual) times the aggregate of dz (scaled residual): EW = x
with its residual alive, EX = dz with its residual alive.

The emulators reproduce each kernel's partitioning in torch (fp16 parts via .half(), products of parts exact in fp32, plane
pairs of p2r_stgcn_gcn3h_pairs' layout, 4-frame tiles of gcn3dwh in dw_tile_order, the tconvh walk: chunks of 64 / 32 / 16
frames, frames t0 - 1 and t0 + chunk from the SAME sample at chunk boundaries and zeros at sequence ends) on NaN-filled
outputs; `mutant=` switches in one defect of MUTANTS.
"""
import struct

import torch

from tests import stgcn_cases as S
from tests.stgcn_cases import C, K, LMAX, NAN, V53, U, check, check_bound, exact_cap, gamma, tables, worst  # noqa: F401

RES = 2048.0
H16_MAX = 65504.0
H16_MIN_NORMAL = 2.0 ** -14
REL3 = 3 * 2.0 ** -22 * (1 + 2.0 ** -9)
F_W = 2.0 ** -23
F_B_PLAIN = 2.0 ** -24
F_B_SCALED = 2.0 ** -35
K_GCNH = LMAX + 1 + 3 * 64 * K + 1
K_TCH = 2 * 192 + 3
PAIRS = {0: [(0, 1), (2, -1), (3, 5), (4, 6), (7, 9), (8, 10)],          # p2r_stgcn_gcn3h_pairs(0 / 1): asserted on the GPU
         1: [(0, 1), (2, 4), (3, 5), (6, 8), (7, 9), (10, -1)]}

MUTANTS = ("drop_a2b1_plane_b", "res_unscaled", "w1s_as_w1", "single_pair_plane0", "scale_one_rescaled", "halo_relu_shift",
           "halo_neighbour_sample", "no_clamp", "mask_eq_1", "addend_before_mask", "idle_unwritten", "full_count",
           "word_not_cleared")


# ---- range words ------------------------------------------------------------------------------------------------------------------
def bits_of(v):
    return struct.unpack("<I", struct.pack("<f", float(v)))[0]


def word_scale(word):
    """p2r_split_scale on the host: word = float bits of max |x| or None -> 2^S"""
    if word is None:
        return 1.0
    eb = (int(word) >> 23) & 0xFF
    if eb == 0 or eb == 255:
        return 1.0
    return 2.0 ** min(139 - eb, 126)


def amax_word(t):
    return bits_of(t.abs().max()) if t.numel() else 0


def same_exponent_word(word):
    """a hand-built word of the same exponent and another significand"""
    return (int(word) & 0x7F800000) | 0x2AAAAA


def weight_scale(W):
    from pose2room_amd.p2rnet import math_mode
    return float(math_mode.weight_scale(W, dims=tuple(range(W.dim())))[0])


def emulate_amax_word(prev, t, mutant=None):
    """the word a producer leaves: cleared, then the maximum of the bit patterns (atomic max on unsigned)"""
    start = int(prev) if mutant == "word_not_cleared" else 0
    return max(start, amax_word(t))


# ---- operands ---------------------------------------------------------------------------------------------------------------------
def tail(shape, seed):
    """the heavy-tail profile of tests/test_split16_gpu.py (_tail_profile): runs of 8 frames at 2^0, 2^-5, ... 2^-20"""
    from tests.test_split16_gpu import _tail_profile
    N, _, T, _ = shape
    return _tail_profile(N, T, seed)[0]


class Operands(S.Operands):
    """stgcn_cases.Operands plus the keys of the split families: 'xt' / 'dzt' / 'doutt' (heavy tail), 'xr' / 'dzr' / 'doutr'
    (EX: residual alive), 'Wr' / 'W3r' (EW), 'Ws' / 'W3s' (EX: sparse fp16-exact weights), 'coef0s' / 'coef1s' (one non-zero
    coefficient per list), 'fin1' (scale 1, shift 0), 'xbig' (activations beyond fp16's range: the clamp)."""

    def __init__(self, N, T, family="bounded", seed=0, density=0.25, wdensity=0.25, rdensity=1 / 32):
        super().__init__(N, T, V53, family, "skeleton", seed, density, wdensity)
        self.rdensity = rdensity

    def _make(self, key, g):
        N, T, V = self.N, self.T, self.V
        act = (N, C, T, V)
        if key in ("xt", "dzt", "doutt"):
            return tail(act, {"xt": 31, "dzt": 32, "doutt": 33}[key] + self.seed).contiguous()
        if key in ("xr", "dzr", "doutr"):
            P = torch.randint(1024, 2048, act, generator=g).float()
            R = S._pick(g, act, (0.125, -0.125, 0.25, -0.25, 0.375, -0.375))
            sgn = S._pick(g, act, (1.0, -1.0))
            t = sgn * (P + R) / 1024 * (torch.rand(act, generator=g) < self.rdensity)
            t[0, 0, 0, 0] = (2047 + 0.375) / 1024                      # the maximum: the range word's exponent is known
            t[-1, -1, -1, -1] = -(1024 + 0.125) / 1024
            return t
        if key == "xbig":
            t = torch.randn(act, generator=g)
            t[:, :, ::5, ::7] *= 3.0e5
            return t
        if key in ("Wr", "W3r"):
            shape = (K, C, C) if key == "Wr" else (3, C, C)
            P = 2048 + 2 * torch.randint(0, 1024, shape, generator=g).float()
            R = S._pick(g, shape, (0.25, -0.25, 0.5, -0.5, 0.75, -0.75))
            sgn = S._pick(g, shape, (1.0, -1.0))
            w = sgn * (P + R) / 4096 * (torch.rand(shape, generator=g) < 1 / 16)
            w[0, 0, 0] = (4094 + 0.75) / 4096
            return w
        if key in ("Ws", "W3s"):
            shape = (K, C, C) if key == "Ws" else (3, C, C)
            w = S._pick(g, shape, (0.5, -0.5, 1.0, -1.0), 1 / 8)
            w[0, 0, 0] = 1.0
            return w
        if key in ("coef0s", "coef1s"):
            t = self.tab[int(key[4])]
            coef = torch.zeros(t["ltot"], V)
            for k in range(K):
                nreal = t["nreal"][k]
                j = (torch.rand(V, generator=g) * nreal).long().clamp_(max=max(t["Lk"][k] - 1, 0))
                val = S._pick(g, (V,), (0.5, -0.5, 1.0, -1.0, 2.0, -2.0))
                for v in range(V):
                    if int(nreal[v]) > 0:
                        coef[t["lofs"][k] + int(j[v]), v] = val[v]
            return coef
        if key == "fin1":
            fin = self["fin"].clone()
            fin[2], fin[3] = 1.0, 0.0
            return fin.contiguous()
        return super()._make(key, g)


def planes(ops, form, coef):
    return S.planes_of(ops.tab, form, coef)


# ---- bounds -----------------------------------------------------------------------------------------------------------------------
def split_bound(k, mag, magb, magw, nterms, s_w, s_x, scaled):
    """mag = sum |w| |b|, magb = sum |b|, magw = sum |w| over the nterms terms of an output element"""
    fw, fb = F_W / s_w, (F_B_SCALED if scaled else F_B_PLAIN) / s_x
    return (gamma(k) + REL3) * mag + fw * magb + fb * magw + nterms * fw * fb


def gcnh_ref(x, W, P, word, scaled, bias_cv=None, addend=None, amask=None, s_w=None):
    """graph conv in split16 arithmetic: x (N,64,T,V) fp32, W [K][64][64] (the data gradient passes the transposed planes),
    P = planes(...), word = the range word the kernel is given (None: scale 1), scaled = H3_RES_SCALED (the data gradient)
    -> (value, E, mag)"""
    value, _, mag = S.graph_conv_ref(x, W, P, bias_cv, addend, amask)
    ones = torch.ones_like(W)
    magb = S.graph_conv_ref(x, ones, P)[2]
    magw = W.double().abs().sum((0, 2))[None, :, None, None]
    s_w = weight_scale(W) if s_w is None else s_w
    E = split_bound(K_GCNH, mag, magb, magw, 64 * K, s_w, word_scale(word), scaled)
    return value, E, mag


def clamp_h(x, scale, shift):
    """the forward form's activation: relu(x scale + shift) clamped to fp16's largest finite value, in float64"""
    h = S.transform_ref(x, scale, shift)
    return h.clamp(max=H16_MAX) if scale is not None else h


def tconvh_ref(x, scale, shift, W3, word, bias=None, s_w=None):
    """out = bias + sum_p W3[p] h(t + p - 1), h = min(relu(x scale + shift), 65504) or x -> (value, E, mag)"""
    h = clamp_h(x, scale, shift)
    ha = h.abs()
    out, mag, magb = torch.zeros_like(h), torch.zeros_like(h), torch.zeros_like(h)
    ones = torch.ones(C, C, dtype=torch.float64, device=x.device)
    for p in range(3):
        out += torch.einsum("dc,nctv->ndtv", W3[p].double(), S._shifted(h, p, 3))
        sh = S._shifted(ha, p, 3)
        mag += torch.einsum("dc,nctv->ndtv", W3[p].double().abs(), sh)
        magb += torch.einsum("dc,nctv->ndtv", ones, sh)
    magw = W3.double().abs().sum((0, 2))[None, :, None, None]
    if bias is not None:
        out += bias.double()[None, :, None, None]
        mag += bias.double().abs()[None, :, None, None]
    s_w = weight_scale(W3) if s_w is None else s_w
    return out, split_bound(K_TCH, mag, magb, magw, 192, s_w, word_scale(word), True), mag


def chunk_of(T):
    return 64 if T % 64 == 0 else (32 if T % 32 == 0 else 16)


def stats_chunk_ref(z, FC):
    """(count, mean, M2) [N T / FC][64][3] of the stored z of tconvh -> (value, E)"""
    zt = S.per_tile(z.double(), FC)
    n = float(zt.shape[2])
    cnt = torch.full(zt.shape[:2], n, dtype=torch.float64, device=z.device)
    mean = zt.mean(-1)
    M2 = ((zt - mean[:, :, None]) ** 2).sum(-1)
    hi, lo = zt.amax(-1), zt.amin(-1)
    M = torch.maximum(hi.abs(), lo.abs())
    D = (hi - lo) + gamma(5) * M
    ks = 1 + 4 * FC + 4
    Emean = gamma(ks + 1) * D + U * (M + D)
    EM2 = gamma(3 * ks + 8) * n * D * D
    return torch.stack([cnt, mean, M2], -1), torch.stack([torch.zeros_like(cnt), Emean, EM2], -1)


def bwd_chunk_ref(v, u, fin, FC):
    """(sum g, sum g uhat) [N T / FC][64][2] of tconvh's data-gradient form from the stored result v -> (value, E, mag)"""
    tiles = v.shape[0] * (v.shape[2] // FC)
    val, _, mag = S.bwd_sums_ref(v, u, fin, tiles, "any", F=FC)
    return val, torch.stack([gamma(4 * FC + 5) * mag[..., 0], gamma(4 * FC + 8) * mag[..., 1]], -1), mag


def dwh_ref(x, dz, P, n_blocks, xword, dzword):
    """-> {'dw': (value [K][ci][c], E, mag), 'colsum': (value, E, mag)}: x the A operand (plain residual), the aggregate of
    dz the B operand (scaled residual)"""
    ref = S.weight_grad_ref(x, dz, P, n_blocks, F=4)
    value, _, mag = ref["dw"]
    N, _, T, V = x.shape
    w = S.wg_tiles(N * (T // 4), n_blocks)
    k = LMAX + 1 + 3 * 224 * w
    Pa = P.abs()
    magx = x.double().abs().sum((0, 2, 3))                                  # [ci]: sum |x| over the columns
    magv = torch.zeros(K, C, dtype=torch.float64, device=x.device)         # [k][c]: sum |V_k|
    for n in range(N):
        magv += torch.einsum("kvw,ctw->kc", Pa, dz[n].double().abs())
    s_x, s_g = word_scale(xword), word_scale(dzword)
    fx, fv = F_B_PLAIN / s_x, F_B_SCALED / s_g                              # x: plain two-part; 2^-11 x1: one more 2^-25 |v|
    fx = fx + 2.0 ** -25 / s_x
    E = (gamma(k) + REL3) * mag + fx * magv[:, None, :] + fv * magx[None, :, None] + N * T * V * fx * fv
    return {"dw": (value, E, mag), "colsum": ref["colsum"]}


def dcoefh_ref(x, dz, W, tab, n_blocks, xword, s_w=None):
    """dcoef [ltot][V] -> (value, E, mag): Y_k = W_k x in split arithmetic (both residuals plain), the reduction in fp32"""
    value, _, m2 = S.coef_grad_ref(x, dz, W, tab, n_blocks)
    ones = torch.ones_like(W)
    t = tab[1]
    N, _, T, V = x.shape
    nbr, real = t["nbr"].long().to(x.device), (t["gidx"] >= 0).to(x.device)
    m1 = torch.zeros_like(value)
    mx, mw = torch.zeros_like(value), torch.zeros_like(value)
    Wd, Wa = W.double(), W.double().abs()
    for n in range(N):
        xd, da = x[n].double(), dz[n].double().abs()
        xs = xd.abs().sum(0)                                                # (T, V): sum_c |x|
        for k in range(K):
            Ya = torch.einsum("dc,ctv->dtv", Wd[k], xd).abs()
            ws = Wa[k].sum(1)                                               # [d]: sum_c |W|
            for l in range(t["lofs"][k], t["lofs"][k + 1]):
                dn = da[:, :, nbr[l]]
                m1[l] += (Ya * dn).sum((0, 1))
                mx[l] += (xs[None] * dn).sum((0, 1))
                mw[l] += (ws[:, None, None] * dn).sum((0, 1))
    w = S.wg_tiles(N * (T // 16), n_blocks)
    s_w = weight_scale(W) if s_w is None else s_w
    fw, fb = F_W / s_w, F_B_PLAIN / word_scale(xword)
    m1, mx, mw = m1 * real, mx * real, mw * real
    E = gamma(13 + 4 * w) * m1 + (gamma(3 * 64 + 2) + REL3) * m2 + fw * mx + fb * mw + 64 * fw * fb * dz.double().abs().sum() * real
    return value, E, m2


# ---- conditions of the exact families (CPU test) ----------------------------------------------------------------------------------
def parts_of(t, scale, scaled):
    """fp16 parts of t * scale as the kernels form them -> (p, q) float64 with p + q the represented value"""
    v = t.float() * scale
    p = v.half()
    r = v - p.float()
    q = ((r * RES).half().double() / RES) if scaled else r.half().double()
    return p.double(), q


def exact_split(t, scale, scaled, label):
    """asserts: finite in fp16, represented exactly, no value-carrying part subnormal -> (p, q) float64 at the scaled range"""
    p, q = parts_of(t, scale, scaled)
    assert bool(torch.isfinite(p).all()) and float(p.abs().max()) <= H16_MAX, f"{label}: a scaled operand leaves fp16's range"
    assert torch.equal(p + q, t.double() * scale), f"{label}: p + q != the scaled operand"
    for name, part, f in (("p", p, 1.0), ("q", q, RES if scaled else 1.0)):
        nz = part[part != 0].abs() * f
        assert nz.numel() == 0 or float(nz.min()) >= H16_MIN_NORMAL, f"{label}: part {name} holds an fp16 subnormal"
    return p, q


def weight_parts(W, label, third_plane_cols=None):
    """the host split of W -> (w1, w2, s) float64 / float with w1 + w2 == 2^S W, 2^-11 w1 normal where w1 != 0 (only in the
    input channels third_plane_cols when given: the channels whose operand has a residual)"""
    from pose2room_amd.p2rnet import math_mode
    s = weight_scale(W)
    p, q, ps = math_mode.split_parts(W * s)
    p, q, ps = p.double(), q.double(), ps.double()
    assert torch.equal(p + q, W.double() * s), f"{label}: w1 + w2 != 2^S W"
    if third_plane_cols is not None:
        ps, p3 = ps[..., third_plane_cols], p[..., third_plane_cols]
    else:
        p3 = p
    assert torch.equal(ps * RES, p3), f"{label}: 2^-11 w1 is not exact"
    for part in (p, q, ps):
        nz = part[part != 0].abs()
        assert nz.numel() == 0 or float(nz.min()) >= H16_MIN_NORMAL, f"{label}: a weight part is an fp16 subnormal"
    return p, q, s


# ---- emulators --------------------------------------------------------------------------------------------------------------------
def _split32(v, scaled, mutant=None):
    """fp32 v -> (b1, b2) fp32 holding fp16 values; b2 the residual (scaled by 2^11 when `scaled`)"""
    p = v.half().float()
    r = v - p
    if scaled and mutant != "res_unscaled":
        r = r * RES
    return p, r.half().float()


def pair_operands(W, form):
    """the A operands of gcn3h as the kernel reads them from gcn_op.split_planes' layout
    wh[pair][ph][part][m][16 kg + r][i] = part of 2^S W_{plane (i < 4 ? a : b)}[16 m + r][16 ph + kg + 4 (i & 3)]
    -> (A [pair][slot a / b][part w1, w2, 2^-11 w1][64 rows][64 channels] fp32, 2^S); W = the forward planes"""
    from pose2room_amd.p2rnet import gcn_op
    wh, inv = gcn_op.split_planes(W, PAIRS[form], transposed=form == 1)
    P = len(PAIRS[form])
    t = wh.view(P, 4, 3, 4, 4, 16, 2, 4)                      # pair, ph, part, m, kg, r, slot, j
    A = t.permute(0, 6, 2, 3, 5, 1, 7, 4).reshape(P, 2, 3, C, C).float()      # rows (m, r), channels (ph, j, kg)
    return A, 1.0 / float(inv)


def tap_operands(W3):
    """tconvh's A operands from tconv_op.split_taps' layout wh[part][tap][ks][w][16 kg + r][i] = part of
    2^S W3[tap][16 w + r][32 ks + 8 kg + i] -> (w1, w2, 2^-11 w1 [3 taps][64][64] fp32, 2^S)"""
    from pose2room_amd.p2rnet import tconv_op
    wh, inv = tconv_op.split_taps(W3)
    A = wh.view(3, 3, 2, 4, 4, 16, 8).permute(0, 1, 3, 5, 2, 4, 6).reshape(3, 3, C, C).float()      # part, tap, (w, r), (ks, kg, i)
    return A[0], A[1], A[2], 1.0 / float(inv)


def coef_grad_operands(W):
    """gcn3h_coef_grad's A operands from gcn_op.split_planes_coef_grad's layout wd[k][ph][part][ks][16 kg + r][i] = part of
    2^S W_k[16 ph + r][32 ks + 16 (i >> 2) + 4 (i & 3) + kg] -> (w1, w2 [K][64][64] fp32, 2^S)"""
    from pose2room_amd.p2rnet import gcn_op
    wd, inv = gcn_op.split_planes_coef_grad(W)
    A = wd.view(K, 4, 2, 2, 4, 16, 2, 4).permute(0, 2, 1, 5, 3, 6, 7, 4).reshape(K, 2, C, C).float()   # k, part, (ph, r), (ks, ih, il, kg)
    return A[:, 0], A[:, 1], 1.0 / float(inv)


def emulate_gcn3h(ops, form, xkey, wkey, coefkey, word, with_bias=True, addend=False, masked=False, mutant=None):
    """z (N,64,T,V) of gcn3h_fwd_kernel (form 0) / gcn3h_dx_kernel (form 1): the coefficient table times 2^S_x, the fp32 aggregate
    chain, its two parts, pair by pair and plane by plane the three products into one accumulator, the rescale, the (masked)
    addend.  16-frame tiles on a NaN-filled output."""
    x, coef = ops[xkey], ops[coefkey]
    scaled = form == 1
    s_x = word_scale(word)
    A, s_w = pair_operands(ops[wkey], form)
    cs = coef * (1.0 if mutant == "scale_one_rescaled" else s_x)
    N, _, T, V = x.shape
    z = S._nan(N, C, T, V)
    agg = {k: S._aggregate(x, ops.tab, form, cs, k) for k in range(K)}
    parts = {k: _split32(agg[k], scaled, mutant) for k in range(K)}
    inv = 1.0 / (s_x * s_w)
    for n in range(N):
        for t0 in range(0, T, 16):
            sl = slice(t0, t0 + 16)
            acc = ((ops["bias_cv"] if with_bias else torch.zeros(C, V)) * (s_x * s_w))[:, None, :].expand(C, 16, V).clone()
            for pi, pair in enumerate(PAIRS[form]):
                for which, k in enumerate(pair):
                    a1, a2, a1s = A[pi, which]                # zeros for the missing plane of the single pair
                    if k < 0 and mutant == "single_pair_plane0":
                        k = 0
                        a1, a2, a1s = A[0, 0]
                    if k < 0:
                        assert not bool(a1.any() or a2.any() or a1s.any())
                        continue
                    b1, b2 = parts[k][0][n, :, sl], parts[k][1][n, :, sl]
                    w_res = (a1 if mutant == "w1s_as_w1" else a1s) if scaled else a1
                    acc = acc + torch.einsum("dc,ctv->dtv", w_res, b2)
                    if not (mutant == "drop_a2b1_plane_b" and which == 1):
                        acc = acc + torch.einsum("dc,ctv->dtv", a2, b1)
                    acc = acc + torch.einsum("dc,ctv->dtv", a1, b1)
            out = acc * inv
            if addend:
                a = ops["addend"][n, :, sl]
                if masked:
                    m = ops["amask"][n, :, sl]
                    on = (m == 1) if mutant == "mask_eq_1" else (m != 0)
                    out = (out + a) * on if mutant == "addend_before_mask" else out + a * on
                else:
                    out = out + a
            z[n, :, sl] = out
    return z


def emulate_tconvh(ops, xkey, wkey, word, form="plain", finkey="fin", with_bias=False, mutant=None, ukey="x"):
    """-> (out, partials or None) of tconvh_kernel.  form: 'forward' (scale / shift + ReLU at scale 1, clamp, bias,
    (count, mean, M2) partials), 'plain', 'bwd' (plain + the sums epilogue on ops[ukey] with ops[finkey]).  One workgroup
    per (sample, chunk): frames t0 - 1 .. t0 + chunk, zeros outside [0, T)."""
    x, W3 = ops[xkey], ops[wkey]
    fin = ops[finkey]
    N, _, T, V = x.shape
    FC = chunk_of(T)
    a1, a2, a1s, s_w = tap_operands(W3)
    xform = form == "forward"
    s_x = 1.0 if xform else word_scale(word)
    inv = 1.0 / (s_x * s_w)
    sc, sh = fin[2][:, None, None], fin[3][:, None, None]
    out = S._nan(N, C, T, V)
    part = S._nan(N * (T // FC), C, 3 if xform else 2) if form != "plain" else None

    def frame_values(n, t):
        """the (64, V) operand values of frame t of sample n as `put` forms them"""
        inside = 0 <= t < T
        if not inside and mutant == "halo_neighbour_sample" and 0 <= n * T + t < N * T:
            raw = x[(n * T + t) // T, :, (n * T + t) % T]
        elif inside:
            raw = x[n, :, t]
        else:
            raw = torch.zeros(C, V)
            if not (xform and mutant == "halo_relu_shift"):
                return raw
        if xform:
            v = S._fma(raw, sc[:, 0].expand_as(raw), sh[:, 0].expand_as(raw))
            v = v.clamp(min=0)
            return v if mutant == "no_clamp" else v.clamp(max=H16_MAX)
        return raw * (1.0 if mutant == "scale_one_rescaled" else s_x)

    for n in range(N):
        for ch in range(T // FC):
            t0 = ch * FC
            h = torch.stack([frame_values(n, t) for t in range(t0 - 1, t0 + FC + 1)], 1)        # (64, FC + 2, V)
            b1, b2 = _split32(h, True, mutant)
            hi, lo = torch.zeros(C, FC, V), torch.zeros(C, FC, V)
            for p in range(3):
                w_res = a1[p] if mutant == "w1s_as_w1" else a1s[p]
                lo = lo + torch.einsum("dc,ctv->dtv", w_res, b2[:, p:p + FC])
                lo = lo + torch.einsum("dc,ctv->dtv", a2[p], b1[:, p:p + FC])
                hi = hi + torch.einsum("dc,ctv->dtv", a1[p], b1[:, p:p + FC])
            bias = (ops["bias"] if with_bias else torch.zeros(C))[:, None, None].expand(C, FC, V)
            val = S._fma(hi + lo, torch.full_like(hi, inv), bias)
            out[n, :, t0:t0 + FC] = val
            b = n * (T // FC) + ch
            if form == "forward":
                piv = val[:, 0, :16].sum(1) * 0.0625
                d = val - piv[:, None, None]
                s1, s2 = d.sum((1, 2)), (d * d).sum((1, 2))
                cnt = float(FC * V)
                dd = s1 / cnt
                part[b, :, 0], part[b, :, 1], part[b, :, 2] = cnt, piv + dd, torch.clamp(s2 - s1 * dd, min=0)
            elif form == "bwd":
                u = ops[ukey][n, :, t0:t0 + FC]
                gate = S._fma(u, sc.expand_as(u), sh.expand_as(u)) > 0
                g = val * gate
                part[b, :, 0] = g.sum((1, 2))
                part[b, :, 1] = (g * (u - fin[0][:, None, None])).sum((1, 2)) * fin[1]
    return out, part


def emulate_gcn3dwh(ops, xkey, dzkey, coefkey, n_blocks, xword, dzword, mutant=None):
    """-> (dw_partial [n_blocks][K][64 ci][64 c], dbias_partial [n_blocks][64][V]) of gcn3dwh_kernel: 4-frame tiles in
    stgcn_cases.dw_tile_order, x split once per tile (plain residual, 2^-11 x1 formed from x1), the aggregate of dz with the
    scale of its range word in the coefficients, split with a scaled residual, three products per plane."""
    x, dz, coef, tab = ops[xkey], ops[dzkey], ops[coefkey], ops.tab
    N, _, T, V = x.shape
    tps = T // 4
    tiles = N * tps
    s_x, s_g = word_scale(xword), word_scale(dzword)
    cs = coef * s_g
    inv = 1.0 / (s_x * s_g)
    dw, cb = S._nan(n_blocks, K, C, C), S._nan(n_blocks, C, V)
    for b in range(n_blocks):
        mine = S.dw_tile_order(b, n_blocks, tiles)
        if not mine and mutant == "idle_unwritten":
            continue
        acc, col = torch.zeros(K, C, C), torch.zeros(C, V)
        for tile in mine:
            n, t0 = tile // tps, (tile % tps) * 4
            xt, dt = x[n, :, t0:t0 + 4] * s_x, dz[n, :, t0:t0 + 4]
            col = col + ((dt[:, 0] + dt[:, 1]) + (dt[:, 2] + dt[:, 3]))
            x1, x2 = _split32(xt, False)
            x1s = (x1 * (1 / RES)).half().float()
            x1, x2, x1s = (q.reshape(C, -1) for q in (x1, x2, x1s))
            for k in range(K):
                v1, v2 = _split32(S._aggregate(dt, tab, 1, cs, k), True, mutant)
                v1, v2 = v1.reshape(C, -1).t(), v2.reshape(C, -1).t()
                acc[k] = ((acc[k] + x1s @ v2) + x2 @ v1) + x1 @ v1
        dw[b], cb[b] = acc * inv, col
    return dw, cb


def emulate_gcn3h_dcoef(ops, xkey, wkey, n_blocks, xword, mutant=None):
    """dcoef_partial [n_blocks][ltot][V] of gcn3h_dcoef_kernel: Y_k = W_k x from two-part operands (both residuals plain), the
    fp32 reduction against dz at the row-list joints, scaled back when the table is written"""
    x, dz, W, tab = ops[xkey], ops["dz"], ops[wkey], ops.tab
    t = tab[1]
    N, _, T, V = x.shape
    tps = T // 16
    tiles = N * tps
    s_x = word_scale(xword)
    a1, a2, s_w = coef_grad_operands(W)
    inv = 1.0 / (s_x * s_w)
    real = t["gidx"] >= 0
    out = S._nan(n_blocks, t["ltot"], V)
    for b in range(n_blocks):
        mine = list(range(b, tiles, n_blocks))
        if not mine and mutant == "idle_unwritten":
            continue
        table = torch.zeros(t["ltot"], V)
        for tile in mine:
            n, t0 = tile // tps, (tile % tps) * 16
            x1, x2 = _split32(x[n, :, t0:t0 + 16] * s_x, False)
            dt = dz[n, :, t0:t0 + 16]
            for k in range(K):
                Y = torch.einsum("dc,ctv->dtv", a1[k], x2) + torch.einsum("dc,ctv->dtv", a2[k], x1)
                Y = Y + torch.einsum("dc,ctv->dtv", a1[k], x1)
                for l in range(t["lofs"][k], t["lofs"][k + 1]):
                    table[l] = table[l] + (Y * dt[:, :, t["nbr"][l].long()]).sum((0, 1)) * real[l]
        out[b] = table * inv
    return out


# ---- which operands a family uses, per stage --------------------------------------------------------------------------------------
EXACT_FAMILIES = ("E0", "EW", "EX")


def gcn_keys(form, fam):
    """(operand, weight, coefficient table) keys of the graph conv forward (form 0) / data gradient (form 1)"""
    xk = {"E0": "x", "EW": "x", "EX": "xr", "bounded": "x", "tail": "xt"}[fam]
    if form == 1:
        xk = "dz" + xk[1:]
    return xk, {"EW": "Wr", "EX": "Ws"}.get(fam, "W"), f"coef{form}" + ("s" if fam == "EX" else "")


def dwh_keys(fam):
    """(x, dz, coefficient table): the weight gradient's product is x times the aggregate of dz"""
    return ({"EW": "xr", "tail": "xt"}.get(fam, "x"), {"EX": "dzr", "tail": "dzt"}.get(fam, "dz"),
            "coef1s" if fam == "EX" else "coef1")


def dcoef_keys(fam):
    """(x, weight) of the adjacency gradient (dz stays fp32: always 'dz')"""
    return {"EX": "xr", "tail": "xt"}.get(fam, "x"), {"EW": "Wr", "EX": "Ws"}.get(fam, "W")


def tconvh_keys(form, fam):
    """(operand, weight, fin) keys of tconvh: form 'forward' reads x through scale / shift, 'plain' / 'bwd' read dout"""
    base = "x" if form == "forward" else "dout"
    xk = {"EX": base + "r", "tail": base + "t"}.get(fam, base)
    wk = {"EW": "W3r", "EX": "W3s"}.get(fam, "W3")
    if fam == "gate" and form == "forward":
        wk = "W3g"
    return xk, wk, "fin1" if (fam == "EX" and form == "forward") else "fin"


def unit_of(*tensors):
    """the largest power of two of which every element of the float64 tensors is a multiple"""
    u = 2.0 ** 30
    while not all(S.is_multiple(t, u) for t in tensors):
        u /= 2
        assert u > 2.0 ** -80
    return u


def product_conditions(w1, w2, b1, b2, contract, label, extra=None):
    """the conditions of an exact case on the parts (float64, scaled ranges): the dropped term w2 b2 identically zero and the
    sum of absolute part products of every output (+ extra, at the same scale) below 2^24 units.  contract(wa, ba) forms
    the outputs' sums from absolute parts.  -> (cap, unit)"""
    assert float(contract(w2.abs(), b2.abs()).max()) == 0.0, f"{label}: the dropped term a2 b2 is not identically zero"
    unit = unit_of(w1, w2) * unit_of(b1, b2)
    mag = contract(w1.abs() + w2.abs(), b1.abs() + b2.abs())
    if extra is not None:
        assert S.is_multiple(extra, unit), f"{label}: bias / addend off the unit grid"
        mag = mag + extra.abs()
    cap = float(mag.max()) / unit
    assert cap < S.TWO24, f"{label}: {cap:.3g} units: the case leaves the exact range"
    return cap, unit
