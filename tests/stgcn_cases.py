"""Cases, float64 references, running-error bounds and fp32 torch emulators of the exact-fp32 ST-GCN convolution kernels
(csrc/stgcn_gcn.hip, stgcn_gcn2.hip, stgcn_gcn3.hip, stgcn_gcn3_dw.hip, stgcn_gcn3_grad.hip + stgcn_gcn3_dcoef_body.h,
stgcn_tconv.hip, stgcn_tconv2.hip, stgcn_tconv3.hip, stgcn_tile.h), shared by tests/test_stgcn_reference_cpu.py and
tests/test_stgcn_sweep_gpu.py.  The split16 kernels are judged relative to these (tests/test_split16_gpu.py).

The references are plain float64 torch, one function per stage, each evaluated on the kernel's OWN fp32 stage input (the
statistics and the BatchNorm-backward sums on the device's own stored result).  Next to every value comes its
running-error bound in the convention of tests/sa_votes_cases.py / tests/pw_cases.py: u = 2^-24,
gamma(k) = k u / (1 - k u); a value that passed k rounded fp32 operations errs by at most gamma(k) times the same
expression on absolute values.  Every product and every addition counts as one rounding (an upper bound whatever the
MFMA does inside a k-step), a fused fmaf step counts once, and a count is the largest number of operations any term can
pass, so a bound holds for every summation order (the plane order rotates per wave, gcn3_dcoef adds into LDS with float
atomics).  The float64 evaluation itself errs by 2^-53 per operation: ignored.  The counts, read from the kernels:

  * graph conv, forward and data gradient (forms 0 / 1; g3_combine, agg_mfma16): the aggregate
    b_k = sum_j a_k(v_j, w) x(:, t, v_j) is one product and an fmaf chain over the list, at most LMAX = 12 roundings (the
    longest list of the skeleton, GC_MAXL).  The accumulators start from bias_cv and take K * 64 products (one rounding
    each) in K * 64 additions, then the addend is one more addition: a term passes at most
    K_GCN = LMAX + 1 + 64 K + 1 operations, E = gamma(K_GCN) (|bias_cv| + sum_k |W_k| (|a_k| |x|) + |addend|).  The masked
    addend counts where its byte is NON-ZERO (any of 1 .. 255), and nowhere else.
  * forward statistics of the first and second generation and of tconv / tconv2, (sum, sum of squares) per workgroup and
    channel of the n stored values v of the workgroup's tiles: any order, a term passes at most n - 1 additions (and one
    product in the second sum): E = gamma(n) sum |v|, gamma(n + 1) sum v^2.
  * forward statistics of gcn3 / tconv3, (count, mean, M2) per workgroup and channel.  The count is exact.  Each of the
    eight waves sums its values about a pivot c_w = the mean of 16 of them (four DPP additions, an exact product with
    1 / 16), so with lo <= v <= hi, M = max |v| every c_w lies in [lo, hi] up to gamma(5) M and
    |v - c_w| <= D = (hi - lo) + gamma(5) M.  As bn_cases derives it for bn_stats: v - c_w is one rounding, the sums pass
    at most k_s = 1 + 7 (slots) + 4 (row16) + tiles (entry updates) operations, E_s = gamma(k_s) n_w D,
    E_q = gamma(k_s + 2) n_w D^2; d = s / n_w, mean_w = c_w + d: E_mw = gamma(k_s + 1) D + u (M + D); q_w = max(q - s d, 0)
    against Q_w - S_w^2 / n_w: E_qw = gamma(3 k_s + 8) n_w D^2.  The merge mean = mean_0 + (sum_w n_w (mean_w - mean_0)) / n is a
    subtraction, eight fmaf steps, a division and an addition on terms <= D: E_mean = E_mw + gamma(11) (D + 2 E_mw) + u (M + D);
    M2 = sum_w q_w + n_w (mean_w - mean)^2 with e_b = E_mw + E_mean + u D on every (mean_w - mean) <= D, a subtraction, two
    products and eight additions: E_M2 = (gamma(3 k_s + 8) + 2 gamma(11)) n D^2 + n (2 D e_b + e_b^2).  The bound does not
    use which joints a wave owns: it holds for every partition of the values into eight pivoted sets.
  * BatchNorm-backward sums epilogues, per workgroup and channel on the device's stored result v: g' = v under the gate
    (gcn: the byte of bwd_mask is non-zero; tconv: z scale + shift > 0, formed in float64 -- the float64 product of two
    fp32 values is exact and the addition keeps the sign, so this IS the gate fmaf takes: no band, no excluded element).
      gcn3 (row-per-wave epilogue): sum g': (g0 + g1) + (g2 + g3) is two additions, four trips, six shuffles, one entry
      update per tile, the eight waves: k = 20 + tiles; sum g' uhat, uhat = (u - mean) invstd two roundings, an fmaf per
      element (16 per tile), six shuffles, the entry updates, the waves: k = 32 + tiles.
      tconv3: the sums stay in registers over the tiles: k = 6 tiles + 14 and, with (z - mean) one rounding and the
      product with invstd at the end, k = 16 tiles + 16.
      gcn2 / tconv2 (ragged tiles, two epilogue forms): any order over the n gated values of the workgroup, k = n + 3.
  * gcn3_weight_grad / gcn_weight_grad: V_k(v) = sum_j a_k(v, w_j) dz(:, t, w_j) is the fmaf chain (LMAX), the product
    with x one rounding, then a workgroup adds at most cols = 4 V ceil(tiles / n_blocks) columns and the caller's sum
    over the leading axis is taken in float64 here: E = gamma(LMAX + 1 + cols) sum |V_k| |x|.  colsum:
    (d0 + d1) + (d2 + d3), one addition per tile: gamma(2 + tiles per workgroup) sum |dz|; first generation: gamma(cols).
  * gcn3_coef_grad: Y_k = W_k x is 64 products in 64 additions: E_Y = gamma(65) |W_k| |x|; a lane multiplies four rows
    with dz (a product and three fmaf steps, one addition), seven lane-exchange additions and one LDS addition per
    phase and tile: k_d = 13 + 4 tiles per workgroup: E = gamma(k_d) sum |Y_k| |dz| + gamma(66) sum (|W_k| |x|) |dz|.  First
    generation (H_k = Wt_k^T dz against gathered x, float atomics): any order over the workgroup's 64 cols terms,
    E = gamma(64 cols + 1) sum |H_k| |x| + gamma(66) sum (|Wt_k|^T |dz|) |x|.  Padded slots are exactly zero; an entry whose
    current coefficient is zero still gets its gradient (the tables tell real from padded, not the values).
  * temporal conv (tconv, tconv2, tconv3, taps 3 / 1): h = relu(fmaf(x, scale, shift)) is one rounding, taken as float64
    x scale + shift with u |h| = one more operation on its terms; the accumulators start from the bias (tconv3_forward_add:
    from bias + add_ct, one rounding) and take 64 taps products: E = gamma(64 taps + 2 (+ 1)) (|bias| (+ |add_ct|) +
    sum |W| |h|).  The frames t = -1 and t = T of EVERY sample are zeros.
  * tconv_weight_grad (4-frame tiles): h, the product, at most cols = 4 V ceil(tiles / n_blocks) additions:
    E = gamma(2 + cols) sum |dout| |h|; dbias: two additions per tile piece, one per tile, six shuffles:
    gamma(8 + tiles per workgroup) sum |dout|.
  * tconv_weight_grad_dz: dz = k ((gq - m1) - xhat m2) exactly as bn_cases derives bn_bwd_apply:
    E = gamma(3) (|k gq| + |k m1|) + gamma(5) |k xhat m2|, the gate as above.

EXACT cases need no bound at all: x, dz, u small integers, weights from {0, +-0.5, +-1}, coefficients from
{+-0.5, +-1, +-2} at the real list entries (passed as the coefficient table directly), scale / shift / mean / invstd / bias
dyadic, sparse where the reduction is long.  Every term is then a multiple of `unit` and as long as the float64 sum of the
absolute values of an output's terms stays below 2^24 units (exact_cap, asserted from the float64 reference alone in the
CPU test) every product and every partial sum in every order is exactly representable: the fp32 result must EQUAL the
float64 reference bit for bit, in all three generations and at every n_blocks.  The statistics merges divide by counts
and stay with the bounded family.

GATE case (tconv family, p2r_bn_bwd_reduce / p2r_bn_bwd_apply with relu = 2): channels GATE_CH have scale = 1 + 2^-13,
shift = -fl(zc scale) with zc = 1 + 2^-12, whose product 1 + 2^-12 + 2^-13 + 2^-25 rounds DOWN: fl(fl(zc scale) + shift) = 0
<= 0 < fmaf(zc, scale, shift) = 2^-25.  Rounding is monotone, so this is the only way the two forms can differ for a
`> 0` gate: fl(z scale) + shift > 0 >= z scale + shift would need fl(z scale) > -shift >= z scale with -shift a float.  The
mirror image is kept as a control: channels REV_CH have scale = 1 - 2^-13, whose product rounds UP, fmaf = -2^-25 < 0 <=
fl(fl(.) + shift) = 0: closed in both forms, open only for a gate written `>= 0`.  A few hundred elements of these channels
hold zc, scattered over samples, tiles, all four channel phases and joints; the others hold zc - m 2^-12, m = 1, 2, 3
(closed in both forms), every other channel ordinary exact data.  The weights of the forward read these channels with a
factor 2^25, so an open gate is a contribution of +-0.5 or +-1 to an otherwise exact output.

The emulators reproduce each kernel's partitioning in fp32 torch (16-frame tiles, 4-frame tiles of gcn3_dw, four channel
phases of 16, k-steps of 4, the list-order fmaf chain with fmaf through float64, persistent workgroups with both tile
orders of gcn3_dw, per-workgroup partial rows, the three-tap window with its halo, first-generation tiles of 384 // V
frames) on NaN-filled outputs; `mutant=` switches in one defect of MUTANTS.
"""
import functools
import zlib

import torch

from tests import cases
from tests.bn_cases import check_bound  # noqa: F401  (re-exported)
from tests.sa_votes_cases import U, gamma, worst  # noqa: F401

NAN = float("nan")
C = 64
K = 11
V53 = 53
LMAX = 12                       # GC_MAXL: the longest neighbour list a kernel takes (the skeleton's longest is 12)
K_GCN = LMAX + 1 + 64 * K + 1
MASK_BYTES = (0, 1, 2, 255)
TWO24 = 2.0 ** 24
ZC = 1.0 + 2.0 ** -12
GATE_CH = (3, 18, 37, 60)       # one per channel phase
REV_CH = (9, 26, 45, 52)
GATE_W = 2.0 ** 25

MUTANTS = ("halo_neighbour_row", "halo_missing_interior", "drop_last_entry", "pad_as_joint0", "mask_eq_1", "unfused_gate",
           "xcd_skip_tail", "strided_double", "idle_unwritten", "full_count", "colsum_7th", "dw_untransposed",
           "addend_before_mask", "pad_below_tile_longest")


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()) & 0x7FFFFFFF)


# ---- adjacency tables -------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def tables(kind="skeleton", V=V53):
    """kind: 'skeleton' (P2RNet's 53 joints: the pattern of the static schedules), 'extra' (one more link: second
    generation), 'ring' (V joints: first generation).  -> {'A', 'V', 0: column-list tables, 1: row-list tables}, each
    {'nbr' u8 [ltot][V], 'gidx' i64 [ltot][V] (-1: padded), 'Lk', 'lofs', 'ltot', 'nreal' [K][V]}"""
    import numpy as np
    from pose2room_amd.p2rnet import gcn_tables
    if kind == "ring":
        A = cases.ring_adjacency(K, V, V)
    else:
        from pose2room_amd.p2rnet.modules.stgcn_layers import Graph
        A = np.array(Graph().A, dtype=np.float32)
        assert A.shape == (K, V53, V53) and V == V53
        if kind == "extra":
            A[3, 5, 7] = 0.5
    out = {"A": torch.from_numpy(np.ascontiguousarray(A)).float(), "V": V, "kind": kind}
    for form in (0, 1):
        nbr, gidx, Lk = gcn_tables.build(A, transpose=bool(form))
        lofs = [0]
        for n in Lk:
            lofs.append(lofs[-1] + n)
        nreal = torch.stack([(gidx[lofs[k]:lofs[k + 1]] >= 0).sum(0) for k in range(K)])
        out[form] = {"nbr": nbr, "gidx": gidx, "Lk": list(Lk), "lofs": lofs, "ltot": lofs[-1], "nreal": nreal}
    return out


def planes_of(tab, form, coef):
    """the coefficient table coef [ltot][V] of `form` as dense float64 planes P [K][column][source joint]: only REAL slots
    count (a padded slot is no link, whatever it holds)"""
    t = tab[form]
    V = tab["V"]
    gidx = t["gidx"].to(coef.device)
    flat = torch.zeros(K * V * V, dtype=torch.float64, device=coef.device)
    real = gidx >= 0
    flat[gidx[real]] = coef.double()[real]
    P = flat.view(K, V, V)
    return P.transpose(1, 2).contiguous() if form == 0 else P       # form 0: gidx = (k, source, column)


# ---- operands -------------------------------------------------------------------------------------------------------------------
def _ints(g, shape, hi, density):
    v = torch.randint(-hi, hi + 1, shape, generator=g).float()
    return v * (torch.rand(shape, generator=g) < density)


def _pick(g, shape, values, density=1.0):
    v = torch.tensor(values, dtype=torch.float32)[torch.randint(0, len(values), shape, generator=g)]
    return v * (torch.rand(shape, generator=g) < density) if density < 1.0 else v


class Operands:
    """CPU fp32 operands of one case, made on first use (`ops['x']`) from a generator of their own, so that a tensor does
    not depend on which others were asked for.  family: 'bounded' | 'exact' | 'gate' (exact data with the gate channels of
    the module docstring in x / fin / W3 / W1 / m12).  Do not write into them."""

    def __init__(self, N, T, V=V53, family="bounded", kind="skeleton", seed=0, density=0.25, wdensity=0.25):
        self.N, self.T, self.V, self.family, self.kind, self.seed = N, T, V, family, kind, seed
        self.density, self.wdensity = density, wdensity
        self.tab = tables(kind, V)
        self._c = {}

    @property
    def exact(self):
        return self.family != "bounded"

    def __getitem__(self, key):
        if key not in self._c:
            self._c[key] = self._make(key, _gen(self.N, self.T, self.V, self.family, self.kind, self.seed, key))
        return self._c[key]

    def _gate_channels(self, g):
        """x of the gate family in GATE_CH / REV_CH: zc at ~4 % of the positions, zc - m 2^-12 elsewhere"""
        shape = (self.N, len(GATE_CH) + len(REV_CH), self.T, self.V)
        m = torch.randint(1, 4, shape, generator=g).float()
        m = m * (torch.rand(shape, generator=g) >= 0.04)
        return ZC - m * 2.0 ** -12

    def _make(self, key, g):
        N, T, V, ex = self.N, self.T, self.V, self.exact
        act = (N, C, T, V)
        special = list(GATE_CH + REV_CH)
        if key in ("x", "dz", "u", "addend", "dout", "dh"):
            if not ex:
                t = torch.randn(act, generator=g)
                return torch.relu(t + 0.3) if key == "x" and self.seed % 2 else t
            t = _ints(g, act, 2, self.density)
            if key == "x" and self.family == "gate":
                t[:, special] = self._gate_channels(g)
            return t
        if key == "add_ct":
            return _ints(g, (N, C, T), 3, 1.0) if ex else torch.randn(N, C, T, generator=g)
        if key in ("amask", "bmask"):
            return torch.tensor(MASK_BYTES, dtype=torch.uint8)[torch.randint(0, 4, act, generator=g)]
        if key == "W":
            return _pick(g, (K, C, C), (0.5, -0.5, 1.0, -1.0), self.wdensity) if ex else torch.randn(K, C, C, generator=g) / 8
        if key in ("W3", "W1"):
            taps = 3 if key == "W3" else 1
            if not ex:
                return torch.randn(taps, C, C, generator=g) / 8
            return _pick(g, (taps, C, C), (0.5, -0.5, 1.0, -1.0), 0.5)
        if key in ("W3g", "W1g"):   # gate family, forward: the gate channels are read with a factor 2^25
            w = self[key[:2]].clone()
            w[:, :, special] = _pick(g, (w.shape[0], C, len(special)), (0.5, -0.5, 1.0, -1.0)) * GATE_W
            return w
        if key == "Aeff":
            A = self.tab["A"]
            if ex:
                return _pick(g, A.shape, (0.5, -0.5, 1.0, -1.0, 2.0, -2.0)) * (A != 0)
            Aeff = A * (1 + 0.1 * torch.randn(A.shape, generator=g))
            nz = (A != 0).nonzero()
            for (k, v, w) in nz[::7].tolist():          # real entries whose current coefficient is exactly zero
                Aeff[k, v, w] = 0.0
            return Aeff
        if key in ("coef0", "coef1"):
            from pose2room_amd.p2rnet import gcn_tables
            return gcn_tables.coefficients(self["Aeff"], self.tab[int(key[-1])]["gidx"]).contiguous()
        if key == "bias_cv":
            return _ints(g, (C, V), 8, 1.0) / 4 if ex else torch.randn(C, V, generator=g)
        if key == "bias":
            return _ints(g, (C,), 8, 1.0) / 4 if ex else torch.randn(C, generator=g)
        if key == "fin":            # [4][64] = mean, invstd, scale, shift
            if not ex:
                return torch.stack([torch.randn(C, generator=g) * 0.1, torch.rand(C, generator=g) + 0.5,
                                    torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.1]).contiguous()
            fin = torch.stack([_pick(g, (C,), (0.0, 0.5, -0.5, 1.0, -1.0)), _pick(g, (C,), (1.0, 2.0)),
                               _pick(g, (C,), (0.5, 1.0, 2.0)), _pick(g, (C,), (0.0, 0.5, -0.5, 1.0, -1.0, 1.5, -1.5))])
            if self.family == "gate":
                zc = torch.tensor(ZC, dtype=torch.float32)
                for chans, sc in ((GATE_CH, 1.0 + 2.0 ** -13), (REV_CH, 1.0 - 2.0 ** -13)):
                    sc = torch.tensor(sc, dtype=torch.float32)
                    for c in chans:
                        fin[0, c], fin[2, c], fin[3, c] = zc, sc, -(zc * sc)        # fp32 product: fl(zc scale)
            return fin.contiguous()
        if key == "m12":
            if not ex:
                return (torch.randn(2, C, generator=g) * 0.01).contiguous()
            m = _pick(g, (2, C), (0.0, 0.25, -0.25, 0.5, -0.5))
            if self.family == "gate":
                m[:, special] = 0.0
            return m.contiguous()
        raise KeyError(key)


def wg_tiles(tiles, n_blocks):
    """largest number of tiles a persistent workgroup walks"""
    return -(-tiles // n_blocks)


# ---- graph convolution: forward and data gradient ---------------------------------------------------------------------------------
def graph_conv_ref(x, W, P, bias_cv=None, addend=None, amask=None):
    """x (N,64,T,V) fp32, W [K][64][64] (row = output channel; the data gradient passes the transposed planes), P =
    planes_of(...) -> (z, E, mag) float64, sample by sample.  amask: bytes, the addend counts where they are non-zero."""
    N = x.shape[0]
    Wd, Wa, Pa = W.double(), W.double().abs(), P.abs()
    z = torch.empty(x.shape, dtype=torch.float64, device=x.device)
    mag = torch.empty_like(z)
    for n in range(N):
        xd = x[n].double()
        xa = xd.abs()
        zn = torch.zeros_like(xd)
        mn = torch.zeros_like(xd)
        for k in range(K):
            zn += torch.einsum("dc,ctw->dtw", Wd[k], torch.einsum("ws,cts->ctw", P[k], xd))
            mn += torch.einsum("dc,ctw->dtw", Wa[k], torch.einsum("ws,cts->ctw", Pa[k], xa))
        if bias_cv is not None:
            zn += bias_cv.double()[:, None, :]
            mn += bias_cv.double().abs()[:, None, :]
        if addend is not None:
            a = addend[n].double()
            if amask is not None:
                a = a * (amask[n] != 0)
            zn += a
            mn += a.abs()
        z[n], mag[n] = zn, mn
    return z, gamma(K_GCN) * mag, mag


def per_tile(t, F):
    """(N,64,T,V) float64 -> [N * ceil(T / F)][64][F * V] tiles of F frames in the kernels' order, a ragged last tile
    padded with NaN (use nansum / nan-aware reductions)"""
    N, Cc, T, V = t.shape
    tps = -(-T // F)
    pad = torch.full((N, Cc, tps * F, V), NAN, dtype=t.dtype, device=t.device)
    pad[:, :, :T] = t
    return pad.view(N, Cc, tps, F * V).permute(0, 2, 1, 3).reshape(N * tps, Cc, F * V)


def wg_reduce(tile_vals, n_blocks, op="sum"):
    """per-tile values [tiles][64] -> per-workgroup [n_blocks][64] with tile = b + i n_blocks"""
    tiles = tile_vals.shape[0]
    idx = torch.arange(tiles, device=tile_vals.device) % n_blocks
    if op == "sum":
        out = torch.zeros(n_blocks, tile_vals.shape[1], dtype=tile_vals.dtype, device=tile_vals.device)
        return out.index_add_(0, idx, tile_vals)
    init = float("-inf") if op == "amax" else float("inf")
    rounds = -(-tiles // n_blocks)
    pad = torch.full((rounds * n_blocks, tile_vals.shape[1]), init, dtype=tile_vals.dtype, device=tile_vals.device)
    pad[:tiles] = tile_vals
    pad = pad.view(rounds, n_blocks, -1)
    return pad.amax(0) if op == "amax" else pad.amin(0)


def stats3_ref(z, n_blocks, F=16):
    """(count, mean, M2) entries [n_blocks][64][3] of the stored z (fp32) of gcn3 / tconv3 -> (value, E)"""
    zt = per_tile(z.double(), F)                                   # whole tiles only (T % 16 == 0)
    tiles, cols = zt.shape[0], zt.shape[2]
    cnt = wg_reduce(torch.full((tiles, C), float(cols), dtype=torch.float64, device=z.device), n_blocks)
    mean = wg_reduce(zt.sum(-1), n_blocks) / cnt
    tile_wg = torch.arange(tiles, device=z.device) % n_blocks
    M2 = wg_reduce(((zt - mean[tile_wg][:, :, None]) ** 2).sum(-1), n_blocks)
    hi, lo = wg_reduce(zt.amax(-1), n_blocks, "amax"), wg_reduce(zt.amin(-1), n_blocks, "amin")
    M = torch.maximum(hi.abs(), lo.abs())
    D = (hi - lo) + gamma(5) * M
    ks = 12 + wg_tiles(tiles, n_blocks)
    Emw = gamma(ks + 1) * D + U * (M + D)
    Emean = Emw + gamma(11) * (D + 2 * Emw) + U * (M + D)
    eb = Emw + Emean + U * D
    EM2 = (gamma(3 * ks + 8) + 2 * gamma(11)) * cnt * D * D + cnt * (2 * D * eb + eb * eb)
    return torch.stack([cnt, mean, M2], -1), torch.stack([torch.zeros_like(cnt), Emean, EM2], -1)


def stats2_ref(z, n_blocks, F):
    """(sum, sum of squares) pairs [n_blocks][64][2] of the stored z: first / second generation, tiles of F frames (the
    last one ragged); n_blocks = number of tiles for the first-generation graph conv (one workgroup per tile)"""
    zt = per_tile(z.double(), F)
    tiles = zt.shape[0]
    s = wg_reduce(zt.nansum(-1), n_blocks)
    a = wg_reduce(zt.abs().nansum(-1), n_blocks)
    q = wg_reduce((zt * zt).nansum(-1), n_blocks)
    n = wg_tiles(tiles, n_blocks) * zt.shape[2]
    return torch.stack([s, q], -1), torch.stack([gamma(n) * a, gamma(n + 1) * q], -1)


def bwd_sums_ref(v, u, fin, n_blocks, kind, bmask=None, F=16):
    """(sum g', sum g' uhat) [n_blocks][64][2] from the device's stored result v (fp32).  kind: 'gcn3' | 'tconv3' |
    'any' (second generation).  gcn: gate = byte of bmask non-zero; tconv: sign of u scale + shift in float64."""
    f = fin.double()
    cv = lambda r: f[r][None, :, None, None]
    ud = u.double()
    if bmask is not None:
        gate = bmask != 0
    else:
        gate = ud * cv(2) + cv(3) > 0
    g = v.double() * gate
    t = g * ((ud - cv(0)) * cv(1))
    gt, tt = per_tile(g, F), per_tile(t, F)
    tiles = gt.shape[0]
    val = torch.stack([wg_reduce(gt.nansum(-1), n_blocks), wg_reduce(tt.nansum(-1), n_blocks)], -1)
    mag = torch.stack([wg_reduce(gt.abs().nansum(-1), n_blocks), wg_reduce(tt.abs().nansum(-1), n_blocks)], -1)
    w = wg_tiles(tiles, n_blocks)
    k1, k2 = {"gcn3": (20 + w, 32 + w), "tconv3": (6 * w + 14, 16 * w + 16)}.get(kind, (w * gt.shape[2] + 3,) * 2)
    return val, torch.stack([gamma(k1) * mag[..., 0], gamma(k2) * mag[..., 1]], -1), mag


# ---- graph convolution: weight, bias-table and adjacency gradients ---------------------------------------------------------------
def weight_grad_ref(x, dz, P, n_blocks, F=4):
    """-> {'dw': (value [K][ci][c] (dW_k transposed), E, mag), 'colsum': (value [64][V], E, mag)}; P = row-form planes"""
    N, _, T, V = x.shape
    tiles = N * (-(-T // F))
    cols = F * V * wg_tiles(tiles, n_blocks)
    dw = torch.zeros(K, C, C, dtype=torch.float64, device=x.device)
    mag = torch.zeros_like(dw)
    Pa = P.abs()
    for n in range(N):
        xd, dd = x[n].double(), dz[n].double()
        xa, da = xd.abs(), dd.abs()
        for k in range(K):
            dw[k] += torch.einsum("itv,ctv->ic", xd, torch.einsum("vw,ctw->ctv", P[k], dd))
            mag[k] += torch.einsum("itv,ctv->ic", xa, torch.einsum("vw,ctw->ctv", Pa[k], da))
    cs, ca = dz.double().sum((0, 2)), dz.double().abs().sum((0, 2))
    return {"dw": (dw, gamma(LMAX + 1 + cols) * mag, mag),
            "colsum": (cs, gamma(2 + wg_tiles(tiles, n_blocks)) * ca, ca), "cols": cols}


def coef_grad_ref(x, dz, W, tab, n_blocks, F=16, first_gen=False):
    """dcoef [ltot][V] at the row-list entries (form 1) -> (value, E, mag); padded slots: value 0, bound 0"""
    t = tab[1]
    N, _, T, V = x.shape
    nbr, real = t["nbr"].long().to(x.device), (t["gidx"] >= 0).to(x.device)
    val = torch.zeros(t["ltot"], V, dtype=torch.float64, device=x.device)
    m1, m2 = torch.zeros_like(val), torch.zeros_like(val)
    Wd, Wa = W.double(), W.double().abs()
    for n in range(N):
        xd, dd = x[n].double(), dz[n].double()
        xa, da = xd.abs(), dd.abs()
        for k in range(K):
            Y = torch.einsum("dc,ctv->dtv", Wd[k], xd)
            Ym = torch.einsum("dc,ctv->dtv", Wa[k], xa)
            for l in range(t["lofs"][k], t["lofs"][k + 1]):
                val[l] += (Y * dd[:, :, nbr[l]]).sum((0, 1))
                m1[l] += (Y.abs() * da[:, :, nbr[l]]).sum((0, 1))
                m2[l] += (Ym * da[:, :, nbr[l]]).sum((0, 1))
    tiles = N * (-(-T // F))
    w = wg_tiles(tiles, n_blocks)
    kd = 64 * F * V * w + 1 if first_gen else 13 + 4 * w
    val, m1, m2 = val * real, m1 * real, m2 * real
    return val, gamma(kd) * m1 + gamma(66) * m2, m2


# ---- temporal convolution ---------------------------------------------------------------------------------------------------------
def transform_ref(x, scale, shift):
    """h = relu(x scale + shift) in float64 (the sign is exactly fmaf's), x itself without a transform"""
    if scale is None:
        return x.double()
    return torch.relu(x.double() * scale.double()[None, :, None, None] + shift.double()[None, :, None, None])


def _shifted(h, p, taps):
    """h (N,64,T,V) -> the frames t + p - (taps - 1) / 2 with zeros outside [0, T) of every sample"""
    d = p - (taps - 1) // 2
    if d == 0:
        return h
    out = torch.zeros_like(h)
    if d < 0:
        out[:, :, -d:] = h[:, :, :d]
    else:
        out[:, :, :-d] = h[:, :, d:]
    return out


def tconv_ref(x, scale, shift, W3, bias=None, add_ct=None):
    """out = bias + add_ct + sum_p W3[p] h(t + p - (taps - 1) / 2) -> (value, E, mag)"""
    taps = W3.shape[0]
    h = transform_ref(x, scale, shift)
    ha = h.abs()
    out = torch.zeros_like(h)
    mag = torch.zeros_like(h)
    for p in range(taps):
        out += torch.einsum("dc,nctv->ndtv", W3[p].double(), _shifted(h, p, taps))
        mag += torch.einsum("dc,nctv->ndtv", W3[p].double().abs(), _shifted(ha, p, taps))
    if bias is not None:
        out += bias.double()[None, :, None, None]
        mag += bias.double().abs()[None, :, None, None]
    if add_ct is not None:
        out += add_ct.double()[..., None]
        mag += add_ct.double().abs()[..., None]
    return out, gamma(64 * taps + 2 + (add_ct is not None)) * mag, mag


def tconv_weight_grad_ref(x, scale, shift, dout, taps, n_blocks, F=4):
    """-> {'dw': (value [64 c][64 ci][taps], E, mag), 'dbias': (value [64], E, mag)}"""
    N, _, T, V = x.shape
    h = transform_ref(x, scale, shift)
    dd = dout.double()
    dw = torch.stack([torch.einsum("nctv,nitv->ci", dd, _shifted(h, p, taps)) for p in range(taps)], -1)
    mag = torch.stack([torch.einsum("nctv,nitv->ci", dd.abs(), _shifted(h.abs(), p, taps)) for p in range(taps)], -1)
    w = wg_tiles(N * (-(-T // F)), n_blocks)
    db, da = dd.sum((0, 2, 3)), dd.abs().sum((0, 2, 3))
    return {"dw": (dw, gamma(2 + F * V * w) * mag, mag), "dbias": (db, gamma(8 + w) * da, da)}


def bn_dz_ref(x, fin, dh, m12):
    """dz = scale ((x scale + shift > 0 ? dh : 0) - m1 - (x - mean) invstd m2) -> (value, E, mag)"""
    f, m = fin.double(), m12.double()
    cv = lambda r: r[None, :, None, None]
    xd = x.double()
    gq = dh.double() * (xd * cv(f[2]) + cv(f[3]) > 0)
    xh = (xd - cv(f[0])) * cv(f[1])
    k = cv(f[2])
    val = k * (gq - cv(m[0]) - xh * cv(m[1]))
    a, b = (k * gq).abs() + (k * cv(m[0])).abs(), (k * xh * cv(m[1])).abs()
    return val, gamma(3) * a + gamma(5) * b, a + b


def check(got, ref, exact, label=""):
    """got fp32 against ref = (value, E, ...) on the same device: within the bound element by element, or -- exact cases --
    EQUAL to the float64 value.  -> worst error / bound (0 for an exact case)"""
    value, E = ref[0], ref[1]
    if not exact:
        return check_bound(got, (value, E), label)
    assert got.dtype == torch.float32 and got.shape == value.shape, f"{label}: dtype / shape {got.dtype} {tuple(got.shape)}"
    assert not torch.isnan(got).any(), f"{label}: NaN (an element never written?)"
    bad = got.double() != value
    if bool(bad.any()):
        at = tuple(bad.nonzero()[0].tolist())
        raise AssertionError(f"{label}: {int(bad.sum())} element(s) differ from the exact value, first at {at}: "
                             f"{float(got[at])!r} != {float(value[at])!r}")
    return 0.0


def exact_cap(mag, unit):
    """the largest sum of absolute terms in units of the smallest term: must stay below 2^24"""
    return float(mag.max()) / unit if mag.numel() else 0.0


def is_multiple(value, unit):
    q = value / unit
    return bool((q == q.round()).all())


def gate_forms(z, scale, shift):
    """(fused, unfused) pre-activations of fp32 z (N,64,T,V): fmaf(z, scale, shift) rounded from float64 (exact here: the
    operands of the gate channels have few bits) and fl(fl(z scale) + shift) in plain fp32 torch"""
    sc, sh = scale[None, :, None, None], shift[None, :, None, None]
    return (z.double() * sc.double() + sh.double()).float(), z * sc + sh


# ---- emulators --------------------------------------------------------------------------------------------------------------------
def _fma(a, b, c):
    """fmaf through float64: the product of two fp32 values is exact there"""
    return (a.double() * b.double() + c.double()).float()


def _nan(*shape):
    return torch.full(shape, NAN, dtype=torch.float32)


def _aggregate(x, tab, form, coef, k, mutant=None):
    """b_k (.., V) of one plane in fp32: the list-order chain c0 x0, fmaf(c1, x1, .), ... over the REAL entries of each
    column's list.  x (..., V).  mutants: 'drop_last_entry' (the sixth entry of a step of six entries), 'pad_as_joint0' (padded
    slots run as links to joint 0: harmless here while the table holds zeros there)"""
    t = tab[form]
    l0, L = t["lofs"][k], t["Lk"][k]
    nreal = t["nreal"][k]
    v = torch.zeros_like(x)
    for j in range(L):
        live = nreal > j
        if mutant == "drop_last_entry" and j % 6 == 5:
            live = torch.zeros_like(live)
        if mutant == "pad_as_joint0":
            live = torch.ones_like(live)
        xj = x[..., t["nbr"][l0 + j].long()]
        cj = coef[l0 + j]
        nv = cj * xj if j == 0 else _fma(cj.expand_as(xj), xj, v)
        v = torch.where(live, nv, v)
    return v


def _tiles_of(b, n_blocks, tiles):
    return range(b, tiles, n_blocks)


def emulate_graph_conv(ops, form, gen=3, with_bias=True, addend=False, masked=False, max_blocks=256, mutant=None):
    """z (N,64,T,V) on a NaN-filled output.  gen 3 / 2: 16-frame tiles (gen 2: a ragged last one) over
    min(tiles, max_blocks) persistent workgroups (256 on the device); gen 1: one workgroup per tile of 384 // V frames.  Per tile: the accumulators start from the
    bias table, then phase by phase (16 channels), plane by plane (the order rotates with the phase), k-step by k-step
    (4 channels, added one after the other) the products with the aggregate; then the (masked) addend."""
    tab = ops.tab
    x = ops["dz"] if form == 1 else ops["x"]
    W = ops["W"].transpose(1, 2) if form == 1 else ops["W"]
    coef = ops["coef1" if form == 1 else "coef0"]
    N, _, T, V = x.shape
    F = 16 if gen > 1 else min(384 // V, T)
    tps = -(-T // F)
    tiles = N * tps
    nb = min(tiles, max_blocks) if gen > 1 else tiles
    z = _nan(N, C, T, V)
    for b in range(nb):
        for tile in _tiles_of(b, nb, tiles):
            n, t0 = tile // tps, (tile % tps) * F
            xt = x[n, :, t0:t0 + F]                                    # (64, f, V)
            acc = (ops["bias_cv"] if with_bias else torch.zeros(C, V))[:, None, :].expand(C, xt.shape[1], V).clone()
            agg = [_aggregate(xt, tab, form, coef, k, mutant) for k in range(K)]
            for ph in range(4):
                for i in range(K):
                    k = (i + ph) % K
                    for ch in range(16 * ph, 16 * ph + 16):
                        acc = acc + W[k][:, ch, None, None] * agg[k][ch][None]
            if addend:
                a = ops["addend"][n, :, t0:t0 + F]
                if masked:
                    m = ops["amask"][n, :, t0:t0 + F]
                    on = (m == 1) if mutant == "mask_eq_1" else (m != 0)
                    acc = (acc + a) * on if mutant == "addend_before_mask" else acc + a * on
                else:
                    acc = acc + a
            z[n, :, t0:t0 + F] = acc
    return z


WAVE_JOINTS = (7, 7, 7, 7, 7, 6, 6, 6)          # joints per wave of a pivoted-statistics epilogue (any split of the 53)


def emulate_stats3(z, n_blocks, mutant=None):
    """the (count, mean, M2) epilogue of gcn3 / tconv3 on the stored z (fp32, T % 16 == 0) -> [n_blocks][64][3].  Eight
    waves own consecutive joint runs; pivot = mean of the wave's first 16 values; sums about it tile by tile; the merge
    of the kernel's last lines.  mutant 'full_count': every workgroup takes ceil(tiles / n_blocks) tiles as its count."""
    N, _, T, V = z.shape
    tps = T // 16
    tiles = N * tps
    out = _nan(n_blocks, C, 3)
    j0 = [sum(WAVE_JOINTS[:w]) for w in range(9)]
    for b in range(n_blocks):
        mine = list(_tiles_of(b, n_blocks, tiles))
        ntiles = wg_tiles(tiles, n_blocks) if mutant == "full_count" else len(mine)
        s = torch.zeros(8, C)
        q = torch.zeros(8, C)
        piv = torch.zeros(8, C)
        for i, tile in enumerate(mine):
            n, t0 = tile // tps, (tile % tps) * 16
            for w in range(8):
                v = z[n, :, t0:t0 + 16, j0[w]:j0[w + 1]]               # (64, 16, joints)
                if i == 0:
                    piv[w] = v[:, :, 0].sum(1) * 0.0625
                d = v - piv[w][:, None, None]
                s[w] = s[w] + d.sum((1, 2))
                q[w] = q[w] + (d * d).sum((1, 2))
        per_joint = float(ntiles * 16)
        nw = torch.tensor([per_joint * j for j in WAVE_JOINTS])[:, None]
        d = s / nw
        mw = piv + d
        qw = torch.clamp(q - s * d, min=0)
        n = per_joint * V
        mean = mw[0] + (nw * (mw - mw[0])).sum(0) / n
        m2 = (qw + nw * (mw - mean) * (mw - mean)).sum(0)
        out[b, :, 0], out[b, :, 1], out[b, :, 2] = n, mean, m2
    return out


def emulate_bwd_sums(v, u, fin, n_blocks, bmask=None, mutant=None):
    """the BatchNorm-backward sums epilogue on the stored result v -> [n_blocks][64][2], a tile at a time"""
    N, _, T, V = v.shape
    tps = T // 16
    tiles = N * tps
    out = _nan(n_blocks, C, 2)
    cv = lambda r: fin[r][:, None, None]
    for b in range(n_blocks):
        s1, s2 = torch.zeros(C), torch.zeros(C)
        for tile in _tiles_of(b, n_blocks, tiles):
            n, t0 = tile // tps, (tile % tps) * 16
            vt, ut = v[n, :, t0:t0 + 16], u[n, :, t0:t0 + 16]
            if bmask is not None:
                m = bmask[n, :, t0:t0 + 16]
                gate = (m == 1) if mutant == "mask_eq_1" else (m != 0)
            elif mutant == "unfused_gate":
                gate = ut * cv(2) + cv(3) > 0
            else:
                gate = _fma(ut, cv(2).expand_as(ut), cv(3).expand_as(ut)) > 0
            g = vt * gate
            s1 = s1 + g.sum((1, 2))
            s2 = s2 + (g * ((ut - cv(0)) * cv(1))).sum((1, 2))
        out[b, :, 0], out[b, :, 1] = s1, s2
    return out


def dw_tile_order(b, n_blocks, tiles, mutant=None):
    """tiles of workgroup b in gcn3_dw_kernel's order: XCD-grouped (i 8 + xcd) per_xcd + slot when n_blocks % 8 == 0,
    strided b + i n_blocks otherwise.  mutants: 'xcd_skip_tail' (whole rounds only under the XCD order),
    'strided_double' (the strided order steps by n_blocks - 1)"""
    out = []
    if n_blocks % 8 == 0:
        per = n_blocks // 8
        xcd, slot = b & 7, b >> 3
        rounds = tiles // n_blocks if mutant == "xcd_skip_tail" else -(-tiles // n_blocks)
        for i in range(rounds):
            t = (i * 8 + xcd) * per + slot
            if t < tiles:
                out.append(t)
    else:
        step = max(n_blocks - 1, 1) if mutant == "strided_double" else n_blocks
        t = b
        while t < tiles:
            out.append(t)
            t += step
    return out


def emulate_gcn3_dw(ops, n_blocks, mutant=None):
    """-> (dw_partial [n_blocks][K][64 ci][64 c], colsum_partial [n_blocks][64][V]) of gcn3_dw_kernel: 4-frame tiles in
    dw_tile_order, the aggregate V_k of dz through the row lists, one fp32 product per tile and plane; 512 threads own
    seven (channel, joint) column sums each.  mutants: the tile orders', 'idle_unwritten', 'colsum_7th', 'dw_untransposed',
    'drop_last_entry'"""
    x, dz, coef, tab = ops["x"], ops["dz"], ops["coef1"], ops.tab
    N, _, T, V = x.shape
    tps = T // 4
    tiles = N * tps
    dw, cs = _nan(n_blocks, K, C, C), _nan(n_blocks, C, V)
    for b in range(n_blocks):
        mine = dw_tile_order(b, n_blocks, tiles, mutant)
        if not mine and mutant == "idle_unwritten":
            continue
        acc = torch.zeros(K, C, C)
        col = torch.zeros(C, V)
        for tile in mine:
            n, t0 = tile // tps, (tile % tps) * 4
            xt, dt = x[n, :, t0:t0 + 4], dz[n, :, t0:t0 + 4]
            col = col + ((dt[:, 0] + dt[:, 1]) + (dt[:, 2] + dt[:, 3]))
            for k in range(K):
                vk = _aggregate(dt, tab, 1, coef, k, mutant)
                acc[k] = acc[k] + xt.reshape(C, -1) @ vk.reshape(C, -1).t()
        if mutant == "colsum_7th":
            flat = col.reshape(-1).clone()
            flat[6 * 512:] = NAN                         # idx = tid + 512 i, i = 6: never written
            col = flat.view(C, V)
        dw[b] = acc.transpose(1, 2) if mutant == "dw_untransposed" else acc
        cs[b] = col
    return dw, cs


def tile_longest(tab, F):
    """[ltot][V] bool: slot j of joint v lies below the longest real list among the joints that share a 16-column n-tile
    with v in the first-generation adjacency-gradient kernel (columns joint-major: column = joint F + frame)"""
    t = tab[1]
    V = tab["V"]
    out = torch.zeros(t["ltot"], V, dtype=torch.bool)
    ntiles = -(-F * V // 16)
    for k in range(K):
        for nt in range(ntiles):
            joints = sorted({c // F for c in range(16 * nt, min(16 * nt + 16, F * V))})
            L = int(t["nreal"][k][joints].max())
            for j in range(L):
                out[t["lofs"][k] + j, joints] = True
    return out


def emulate_gcn3_dcoef(ops, n_blocks, mutant=None, F=16):
    """dcoef_partial [n_blocks][ltot][V] of gcn3_dcoef_kernel: a zeroed table per workgroup, tiles of F = 16 frames, four
    output-row phases of Y_k = W_k x, each reduced against dz at the row-list joints and added to the table (the first
    generation forms H_k = W_k^T dz against gathered x instead: the same terms).  mutants: 'pad_as_joint0' (padded slots
    run as links to joint 0), 'pad_below_tile_longest' (what gcn_dcoef_kernel did before this sweep: every slot below the
    longest list of the n-tile's joints is added, a shorter list's padding with joint 0; F = the kernel's 384 // V)"""
    x, dz, W, tab = ops["x"], ops["dz"], ops["W"], ops.tab
    t = tab[1]
    N, _, T, V = x.shape
    tps = -(-T // F)
    tiles = N * tps
    out = _nan(n_blocks, t["ltot"], V)
    real = t["gidx"] >= 0
    if mutant == "pad_below_tile_longest":
        real = real | tile_longest(tab, F)
    for b in range(n_blocks):
        table = torch.zeros(t["ltot"], V)
        for tile in _tiles_of(b, n_blocks, tiles):
            n, t0 = tile // tps, (tile % tps) * F
            xt, dt = x[n, :, t0:t0 + F], dz[n, :, t0:t0 + F]
            for ph in range(4):
                rows = slice(16 * ph, 16 * ph + 16)
                for k in range(K):
                    Y = torch.einsum("dc,ctv->dtv", W[k][rows], xt)
                    for l in range(t["lofs"][k], t["lofs"][k + 1]):
                        add = (Y * dt[rows][:, :, t["nbr"][l].long()]).sum((0, 1))
                        live = torch.ones_like(real[l]) if mutant == "pad_as_joint0" else real[l]
                        table[l] = table[l] + add * live
        out[b] = table
    return out


def _transform32(x, scale, shift, mutant=None):
    if scale is None:
        return x
    sc, sh = scale[:, None, None], shift[:, None, None]
    pre = x * sc + sh if mutant == "unfused_gate" else _fma(x, sc.expand_as(x), sh.expand_as(x))
    return torch.relu(pre)


def _window(x, n, t0, F, taps, scale, shift, mutant=None):
    """the h tile (64, F + 2 halo, V) of frames t0 - halo .. t0 + F - 1 + halo of sample n: zeros outside [0, T).
    mutants: 'halo_neighbour_row' (outside the sample the window runs on in memory: the frame in front of channel row c is
    the last frame of row c - 1), 'halo_missing_interior' (zeros at every tile edge)"""
    N, _, T, V = x.shape
    halo = (taps - 1) // 2
    f = min(F, T - t0)
    h = torch.zeros(C, f + 2 * halo, V)
    h[:, halo:halo + f] = _transform32(x[n, :, t0:t0 + f], scale, shift, mutant)
    if halo:
        flat = x.reshape(-1)
        if t0 > 0 and mutant != "halo_missing_interior":
            h[:, 0] = _transform32(x[n, :, t0 - 1:t0], scale, shift, mutant)[:, 0]
        if t0 + f < T and mutant != "halo_missing_interior":
            h[:, -1] = _transform32(x[n, :, t0 + f:t0 + f + 1], scale, shift, mutant)[:, 0]
        if mutant == "halo_neighbour_row":
            for c in range(C):
                row = (n * C + c) * T * V
                if t0 == 0 and row >= V:
                    h[c, 0] = _transform32(flat[row - V:row].view(1, 1, V), scale[c:c + 1] if scale is not None else None,
                                           shift[c:c + 1] if scale is not None else None)[0, 0]
                if t0 + f == T and row + (T + 1) * V <= flat.numel():
                    h[c, -1] = _transform32(flat[row + T * V:row + (T + 1) * V].view(1, 1, V),
                                            scale[c:c + 1] if scale is not None else None,
                                            shift[c:c + 1] if scale is not None else None)[0, 0]
    return h


def emulate_tconv(ops, taps, gen=3, xform=True, with_bias=True, add=False, data_gradient=False, gate_weights=False,
                  max_blocks=256, mutant=None):
    """out (N,64,T,V) on a NaN-filled output: tiles of 16 frames (gen 3 / 2) or 384 // V frames (gen 1) over
    min(tiles, 256) persistent workgroups; per tile the window with its halo, accumulators from bias (+ add_ct), phases
    of 16 channels, taps, k-steps of 4.  data_gradient: x = dout, flipped / transposed taps, no transform."""
    Wk = ops[("W3" if taps == 3 else "W1") + ("g" if gate_weights else "")]
    if data_gradient:
        x, Wk, xform, with_bias = ops["dout"], Wk.flip(0).transpose(1, 2), False, False
    else:
        x = ops["x"]
    scale, shift = (ops["fin"][2], ops["fin"][3]) if xform else (None, None)
    N, _, T, V = x.shape
    F = 16 if gen > 1 else min(384 // V, T)
    tps = -(-T // F)
    tiles = N * tps
    nb = min(tiles, max_blocks)
    halo = (taps - 1) // 2
    out = _nan(N, C, T, V)
    for b in range(nb):
        for tile in _tiles_of(b, nb, tiles):
            n, t0 = tile // tps, (tile % tps) * F
            h = _window(x, n, t0, F, taps, scale, shift, mutant)
            f = h.shape[1] - 2 * halo
            acc = (ops["bias"] if with_bias else torch.zeros(C))[:, None, None].expand(C, f, V).clone()
            if add:
                acc = acc + ops["add_ct"][n, :, t0:t0 + f, None]
            for ph in range(4):
                for p in range(taps):
                    for ch in range(16 * ph, 16 * ph + 16):
                        acc = acc + Wk[p][:, ch, None, None] * h[ch, p:p + f][None]
            out[n, :, t0:t0 + f] = acc
    return out


def emulate_tconv_dw(ops, taps, n_blocks, with_dz=False, xform=True, mutant=None):
    """-> (dw_partial [n_blocks][64 c][64 ci][taps], dbias_partial [n_blocks][64], dz or None) of tconv_dw_kernel: 4-frame
    tiles, strided persistent workgroups, the h window with its halo; with_dz: the BatchNorm-backward apply pass in the
    kernel's operation order"""
    x, dout, fin = ops["x"], ops["dout"], ops["fin"]
    scale, shift = (fin[2], fin[3]) if xform or with_dz else (None, None)
    N, _, T, V = x.shape
    tps = -(-T // 4)
    tiles = N * tps
    dw, db = _nan(n_blocks, C, C, taps), _nan(n_blocks, C)
    dzo = _nan(N, C, T, V) if with_dz else None
    halo = (taps - 1) // 2
    cv = lambda r: r[:, None, None]
    for b in range(n_blocks):
        acc = torch.zeros(C, C, taps)
        bs = torch.zeros(C)
        for tile in _tiles_of(b, n_blocks, tiles):
            n, t0 = tile // tps, (tile % tps) * 4
            h = _window(x, n, t0, 4, taps, scale, shift, mutant)
            f = h.shape[1] - 2 * halo
            dt = dout[n, :, t0:t0 + f]
            bs = bs + dt.sum((1, 2))
            for p in range(taps):
                acc[:, :, p] = acc[:, :, p] + dt.reshape(C, -1) @ h[:, p:p + f].reshape(C, -1).t()
            if with_dz:
                zv, dh = x[n, :, t0:t0 + f], ops["dh"][n, :, t0:t0 + f]
                pre = zv * cv(scale) + cv(shift) if mutant == "unfused_gate" else _fma(zv, cv(scale).expand_as(zv), cv(shift).expand_as(zv))
                gq = dh * (pre > 0)
                xh = (zv - cv(fin[0])) * cv(fin[1])
                dzo[n, :, t0:t0 + f] = cv(scale) * (gq - cv(ops["m12"][0]) - xh * cv(ops["m12"][1]))
        dw[b], db[b] = acc, bs
    return dw, db, dzo
