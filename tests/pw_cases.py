"""Cases, float64 references, comparison functions and torch emulators of the point-wise head kernels
(csrc/pw_layers.hip, csrc/pw_mma.h, p2rnet/pw_op.py) and of the seams of the backbone (csrc/seed_ops.hip,
p2rnet/seed_op.py), shared by tests/test_pw_reference_cpu.py and tests/test_pw_sweep_gpu.py.

The references are plain float64 torch, one function per stage, each evaluated on the kernel's OWN fp32 stage input.
Next to every value comes its running-error bound in the convention of tests/sa_votes_cases.py: u = 2^-24,
gamma(k) = k u / (1 - k u); a value that passed k rounded fp32 operations errs by at most gamma(k) times the same
expression on absolute values, an operand with an error E of its own adds E times the other operand.  The library is
built with -ffp-contract=off, so a * b + c is two roundings and plain fp32 torch in the same order reproduces it bit for
bit.  The counts are read from the kernels:

  * input transforms (pw_gemm_kernel / pw_wgrad_kernel staging): tr_mode 1 relu(x s + t), tr_mode 2 (a g + b z) + c,
    ytr relu(y sc + sh), and the gate of epilogue 1, mz sc + sh > 0: formed in fp32 torch in the kernel's order, so they
    carry no bound and the ReLU no band.  The product is then float64 on T(x).
  * product (pw_product): the accumulator starts at zero and takes kpad = 16 ceil(K / 16) products (the padded ones are
    exact zeros), then the bias: a product is rounded once and passes at most kpad + 1 additions: gamma(kpad + 2), the
    convention of sa_votes_cases.layer for the same pw_product.  Epilogue 1 writes acc under the fp32 gate, exactly 0
    where it is closed (bound 0).
  * tile statistics, on the device's own 64 output values v of a row: epilogue 0: lane sum (v0 + v1) + (v2 + v3) is two
    additions per element, p2r_row16_sum four more: E_s = gamma(6) sum |v|; mean = s / 64 is exact.  d = v - mean (one
    rounding, d enters d^2 twice), d^2 (one), four in-lane additions and four row16 steps:
    sum (v - mean_dev)^2 = M2 + 64 em^2 with |em| <= E_mean, so E_M2 = gamma(11) (M2 + 64 E_mean^2) + 64 E_mean^2.
    Epilogue 1: s1 = sum v passes four in-lane additions and four row16 steps: gamma(8) sum |v|; s2 = sum v xhat,
    xhat = (z - mean) invstd two roundings, the product one more: gamma(11) sum |v xhat|.
  * pw_wgrad: a partial over n columns: gamma(n + 1) |T(dz)| |U(y)|^T (sa_votes_cases: "one partial over cols columns").
    The bias partial: 16 in-thread additions per 64-column chunk, one addition per chunk into bsum, two shuffles:
    gamma(16 + chunks + 2) sum |T(dz)|.  A range with no chunk (split > chunks) is exactly zero.
  * pw_reduce: four interleaved accumulators take floor(P / 4) rows each, a0 the P % 4 remainder, then (a0 + a1) + (a2 + a3):
    a term passes at most floor(P / 4) + P % 4 + 2 additions.
  * pw_bn_finalize: one wave merges the entries in fp64 and rounds once; mean, invstd, scale, shift and running' exactly as
    bn_cases derives them for bn_finalize (the same last-thread arithmetic, unbiased variance over max(count - 1, 1)):
    bn_cases.finalize_ref is the reference.
  * pw_bn_bwd_finalize: embed_cases.bn_bwd_coef_ref.
  * mdn_mix: the device's expf is the one constant that cannot be read off the kernel.  With a pi output the forward writes
    1 / (1 + expf(-logit)); PI_ULP_MEASURED is max |pi - float64 sigmoid| in ulps of pi over the sweep's own logits on an
    MI355X, EXPF_ULP = max(2, ceil(2 measured)) what is allowed for expf (a finite sample: a factor of two), as a relative
    error D_EXP = EXPF_ULP 2u (measured 2.153 ulps, so EXPF_ULP = 5).  p = 1 / (1 + e): the addition and the division: relative error D_P = D_EXP + gamma(2).
    Forward: comp = eps sig + mu (sig carries D_EXP; a product, an addition), comp p (one rounding), ceil(G / 16) gated
    terms per slice, then the 16 slices in order.  Backward, per (component, column): t = sum_d dp comp, (float) t, 1 - p,
    p (1 - p), the product; dmu / dlog_sigma add ceil(cols / 256) terms per thread, then fp64 wave and block sums rounded
    once.  For f64 heads the arithmetic in T is exact to 2^-53 and the f32 parts (logit -> p, log_sigma -> sig) set the bound.
  * vote_finish: f = seed_features + net (one rounding); ss = sum f^2: f enters twice, the product, three in-lane additions
    and six shuffles: gamma(12); sqrtf and the division are correctly rounded: inv errs by gamma(12) / 2 + gamma(2)
    relative, feat = f inv by gamma(2) more.  vote_xyz = hip + net[:3] is one fp32 addition: bit for bit.  A row with
    f == 0 gives inv = 1 / 0 = inf and feat = 0 inf = NaN, what torch's division gives; no other row may change.
    vote_finish_grad: dot = sum g y: gamma(10) sum |g y| (the product, nine additions); df = inv (g - y dot): y dot one
    rounding, the subtraction, the product with inv.
  * rowsum_short: two accumulators take ceil(V / 2) elements, then a0 + a1 and the scale: gamma(ceil(V / 2) + 2).
  * gather_frames, gather_frames_grad, nearest_prefix have no tolerance: a copy; rows added in ascending seed order (a
    sequential fp32 loop is the reference, a frame nobody picked exactly 0); the first index of the fp32 minimum.

The emulators reproduce each kernel's partitioning in fp32 torch (64-column tiles, chunks of 16 k in groups of four,
split ranges, interleaved accumulators, the 64-lane stride of the merges, 16 columns x 16 component slices, ballots over
64 seeds, chunks of 8 frames) on NaN-filled outputs; `mutant=` switches in one defect of MUTANTS.
"""
import collections
import functools
import math
import zlib

import torch

from tests import bn_cases
from tests import cases
from tests.bn_cases import check_bound  # noqa: F401  (re-exported)
from tests.embed_cases import BAND_CAP, bn_bwd_coef_ref  # noqa: F401
from tests.sa_votes_cases import U, gamma, worst  # noqa: F401

NAN = float("nan")
EPS = 1e-5
PW_KMAX = 560
GF_TT, GF_MAXHIT = 8, 16

PI_ULP_MEASURED = 2.153         # max |pi - float64 sigmoid| / ulp(pi) over the sweep's logits, one run on an MI355X
EXPF_ULP = 5                   # max(2, ceil(2 * PI_ULP_MEASURED))
D_EXP = EXPF_ULP * 2 * U
D_P = D_EXP + gamma(2)

MUTANTS = ("stale_group", "kpad_rows_live", "job0_dims", "stats_row_clamped", "gate_on_acc", "drop_last_chunk",
           "empty_range_unwritten", "reduce_drop_tail", "merge_no_between", "biased_running_var", "mix_cols_16",
           "mix_slice_16", "hits_overflow", "ragged_frames", "rowsum_odd_tail", "dead_wave_unwritten")


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()) & 0x7FFFFFFF)


def ncl_cols(t):
    """(B, C, L) -> [C, B L]"""
    return t.permute(1, 0, 2).reshape(t.shape[1], -1)


def cols_ncl(m, B, L):
    """[C, B L] -> (B, C, L)"""
    return m.reshape(m.shape[0], B, L).permute(1, 0, 2).contiguous()


# ---- p2r_pw_gemm ----------------------------------------------------------------------------------------------------------------
COLUMNS = [(1, 64), (3, 64), (2, 128)]        # one tile; a tile per sample; l0 != 0
K_ROW_MAJOR = (16, 64, 80, 128, 144, 192, 208, 560)
K_TRANSPOSED = (1, 3, 15, 17, 33, 100, 259, 547)
GEMM_ROWS = (1, 15, 16, 17, 63, 64, 65, 256, 257, 259)

GemmJob = collections.namedtuple(
    "GemmJob", "name K rows w_t x_nlc out_nlc tr epi stats bias xs xc0 os oc0 ms mc0 ld", defaults=(0, 0, 0, 0, 0, 0, 0))
# xs / os / ms: channels of the tensor beyond the job's own (x_ctot = K + xs ...); xc0 / oc0 / mc0: the job's first
# channel; ld: tr_ld = K + ld, mfin_ld = rows + ld
GEMM_JOBS = [
    #        name            K   rows wt xn on tr ep st bi
    GemmJob("f16x1",         16,   1, 0, 0, 0, 0, 0, 1, 1),                       # one live wave, three dead
    GemmJob("f64x15",        64,  15, 0, 0, 0, 1, 0, 1, 1),                       # nch 4: exactly one group
    GemmJob("f80x16",        80,  16, 0, 0, 0, 0, 0, 0, 0),                       # nch 5
    GemmJob("f128x17",      128,  17, 0, 0, 0, 1, 0, 1, 1, 64, 32, 0, 0, 0, 0, 8),   # x_ctot > k, tr_ld > k
    GemmJob("f144x63",      144,  63, 0, 1, 1, 0, 0, 1, 1),                       # nch 9; NLC 16-byte in, scalar out (rows & 3)
    GemmJob("f192x64",      192,  64, 0, 1, 1, 1, 0, 1, 0, 4, 4, 4, 4),            # nch 12; float4 out inside a slice
    GemmJob("f208x65",      208,  65, 0, 0, 0, 0, 0, 1, 0, 0, 0, 7, 3),            # nch 13; out_ctot > rows (NCL)
    GemmJob("f560x256",     560, 256, 0, 0, 0, 1, 0, 1, 0),                       # nch 35 = PW_KMAX
    GemmJob("f64x257",       64, 257, 0, 0, 0, 0, 0, 1, 1),                       # mtiles 17: a second trip of one tile
    GemmJob("f16x259",       16, 259, 0, 0, 1, 0, 0, 0, 1),
    GemmJob("f64x64_octot",  64,  64, 0, 0, 1, 0, 0, 1, 1, 0, 0, 2, 0),            # out_ctot & 3
    GemmJob("f64x64_off4",   64,  64, 0, 0, 1, 0, 0, 1, 1, 0, 0, 4, 1),            # out 4 bytes past a 16-byte boundary
    GemmJob("f64x16_xodd",   64,  16, 0, 1, 0, 1, 0, 1, 0, 1, 0),                  # x_ctot & 3: scalar NLC loads
    GemmJob("f128x64_tr2",  128,  64, 0, 0, 0, 2, 0, 1, 1, 0, 0, 0, 0, 0, 0, 4),
    GemmJob("f80x259_nlc",   80, 259, 0, 1, 0, 1, 0, 1, 0),
    GemmJob("f144x1",       144,   1, 0, 0, 0, 1, 0, 1, 1),
    GemmJob("f208x15_nlc",  208,  15, 0, 0, 1, 0, 0, 0, 1, 0, 0, 5, 2),
    GemmJob("t1x16",          1,  16, 1, 0, 0, 0, 1, 1, 0),
    GemmJob("t3x64",          3,  64, 1, 1, 0, 0, 1, 1, 0),                       # K & 3: scalar NLC loads
    GemmJob("t15x17",        15,  17, 1, 0, 0, 2, 1, 1, 0),                       # kk clamped at K - 1
    GemmJob("t17x65",        17,  65, 1, 0, 0, 2, 1, 1, 0, 0, 0, 0, 0, 6, 3, 5),   # mz_ctot > rows, mfin_ld > rows
    GemmJob("t33x15",        33,  15, 1, 1, 0, 0, 1, 0, 0),
    GemmJob("t100x256",     100, 256, 1, 1, 0, 0, 1, 1, 0),                       # NLC 16-byte loads, kpad 112
    GemmJob("t259x257",     259, 257, 1, 1, 0, 0, 1, 1, 0),
    GemmJob("t547x63",      547,  63, 1, 0, 1, 2, 0, 0, 0),                       # kpad 560; no epilogue (an input gradient)
    GemmJob("t100x64_e0",   100,  64, 1, 0, 1, 2, 0, 0, 0),
    GemmJob("t17x1",         17,   1, 1, 0, 0, 0, 1, 1, 0),
    GemmJob("t259x259_nlc", 259, 259, 1, 1, 0, 2, 1, 1, 0),
    GemmJob("t33x16_slice",  33,  16, 1, 0, 0, 2, 1, 1, 0, 31, 16, 0, 0, 0, 0, 3),
    GemmJob("t3x257",         3, 257, 1, 0, 0, 0, 1, 1, 0),
    GemmJob("t15x64_bias",   15,  64, 1, 0, 0, 0, 0, 1, 1),
]
GEMM_BY_NAME = {j.name: j for j in GEMM_JOBS}
GEMM_LISTS = {      # every list runs over one (B, L); jobs differ in k, rows, layout and epilogue
    2: ((3, 64), ("f16x1", "f560x256")),
    5: ((2, 128), ("t15x17", "f144x63", "f64x257", "t100x256", "f64x64_off4")),
    8: ((1, 64), ("f80x16", "t547x63", "f192x64", "t3x64", "f128x17", "t17x65", "f16x259", "f64x16_xodd")),
}


def gemm_columns(job):
    return COLUMNS[GEMM_JOBS.index(job) % 3]


def kpad_of(K):
    return (K + 15) & ~15


@functools.lru_cache(maxsize=None)
def gemm_operands(name, B, L):
    """CPU fp32 operands of one job over B x L columns.  Channels of x / x2 / mz outside the job's slice and the columns of
    tr / mfin beyond its own are NaN: whatever reads them shows.  Cached: do not write into them."""
    j = GEMM_BY_NAME[name]
    g = _gen("gemm", name, B, L)
    randn = lambda *s: torch.randn(*s, generator=g)
    xct, mct = j.K + j.xs, j.rows + j.ms

    def act(ctot, c0, n, nlc):
        full = torch.full((B, ctot, L), NAN)
        full[:, c0:c0 + n] = randn(B, n, L)
        return full.transpose(1, 2).contiguous() if nlc else full

    def table(nrows, n, ld, make):
        t = torch.full((nrows, n + ld), NAN)
        for i in range(nrows):
            t[i, :n] = make(i)
        return t

    ops = {"x": act(xct, j.xc0, j.K, j.x_nlc)}
    if j.tr == 1:
        ops["tr"] = table(2, j.K, j.ld, lambda i: (0.5 + torch.rand(j.K, generator=g)) if i == 0 else 0.3 * randn(j.K))
    elif j.tr == 2:
        ops["x2"] = act(xct, j.xc0, j.K, j.x_nlc)
        ops["tr"] = table(3, j.K, j.ld, lambda i: randn(j.K))
    ops["w"] = (randn(j.K, j.rows) if j.w_t else randn(j.rows, j.K)) * (1.0 / j.K ** 0.5)
    if j.bias:
        ops["bias"] = randn(j.rows)
    if j.epi == 1:
        ops["mz"] = act(mct, j.mc0, j.rows, 0)
        ops["mfin"] = table(4, j.rows, j.ld, lambda i: (0.5 + torch.rand(j.rows, generator=g)) if i in (1, 2) else 0.3 * randn(j.rows))
    return ops


def _slice_cols(full, c0, n, nlc):
    """the job's channels of a full activation tensor -> [n, B L]"""
    t = full.transpose(1, 2) if nlc else full
    return ncl_cols(t[:, c0:c0 + n])


def gemm_input(j, ops):
    """T(x) [K, B L] in fp32, the kernel's operation order"""
    x = _slice_cols(ops["x"], j.xc0, j.K, j.x_nlc)
    if j.tr == 1:
        return torch.relu(x * ops["tr"][0, :j.K, None] + ops["tr"][1, :j.K, None])
    if j.tr == 2:
        z = _slice_cols(ops["x2"], j.xc0, j.K, j.x_nlc)
        tr = ops["tr"]
        return (tr[0, :j.K, None] * x + tr[1, :j.K, None] * z) + tr[2, :j.K, None]
    return x


def gemm_gate(j, ops):
    """the fp32 gate of epilogue 1 [rows, B L]"""
    mz = _slice_cols(ops["mz"], j.mc0, j.rows, 0)
    return mz * ops["mfin"][2, :j.rows, None] + ops["mfin"][3, :j.rows, None] > 0


def gemm_ref(j, ops):
    """-> {'out': (value, E) [rows, B L], 'gate': bool or None}; the product in float64 on the fp32 T(x)"""
    T = gemm_input(j, ops).double()
    W = (ops["w"].t() if j.w_t else ops["w"]).double()
    acc, mag = W @ T, W.abs() @ T.abs()
    if j.bias:
        acc, mag = acc + ops["bias"].double()[:, None], mag + ops["bias"].double().abs()[:, None]
    E = gamma(kpad_of(j.K) + 2) * mag
    gate = None
    if j.epi == 1:
        gate = gemm_gate(j, ops)
        acc, E = acc * gate, E * gate
    return {"out": (acc, E), "gate": gate}


def tile_stats_ref(j, ops, out):
    """the statistics entries of the device's own output `out` [rows, B L] fp32 -> (value, E) [tiles][rows][3 or 2]"""
    v = out.double().reshape(out.shape[0], -1, 64)                  # [rows][tiles][64]
    A = v.abs().sum(-1)
    if j.epi == 0:
        mean = v.sum(-1) / 64
        Em = gamma(6) * A / 64
        M2 = ((v - mean[..., None]) ** 2).sum(-1)
        EM2 = gamma(11) * (M2 + 64 * Em ** 2) + 64 * Em ** 2
        value = torch.stack([torch.full_like(mean, 64.0), mean, M2], -1)
        E = torch.stack([torch.zeros_like(mean), Em, EM2], -1)
    else:
        mz = _slice_cols(ops["mz"], j.mc0, j.rows, 0).double().reshape(j.rows, -1, 64)
        xhat = (mz - ops["mfin"][0, :j.rows].double()[:, None, None]) * ops["mfin"][1, :j.rows].double()[:, None, None]
        value = torch.stack([v.sum(-1), (v * xhat).sum(-1)], -1)
        E = torch.stack([gamma(8) * A, gamma(11) * (v * xhat).abs().sum(-1)], -1)
    return value.transpose(0, 1), E.transpose(0, 1)


def check_gemm(j, ops, out, stats, ref=None, label=""):
    """out [rows, B L] CPU fp32 (the job's slice), stats [tiles][rows][3 | 2] or None -> {name: worst error / bound}"""
    ref = ref or gemm_ref(j, ops)
    label = label or j.name
    ratios = {"out": check_bound(out, ref["out"], label + " out")}
    if ref["gate"] is not None:
        assert not out[~ref["gate"]].any(), f"{label}: a closed gate let a value through"
    if stats is not None:
        value, E = tile_stats_ref(j, ops, out)
        if j.epi == 0:
            assert (stats[..., 0] == 64).all(), f"{label}: count is not 64"
            assert (stats[..., 2] >= 0).all(), f"{label}: negative M2"
            ratios["mean"] = check_bound(stats[..., 1], (value[..., 1], E[..., 1]), label + " mean")
            ratios["M2"] = check_bound(stats[..., 2], (value[..., 2], E[..., 2]), label + " M2")
        else:
            ratios["s1"] = check_bound(stats[..., 0], (value[..., 0], E[..., 0]), label + " s1")
            ratios["s2"] = check_bound(stats[..., 1], (value[..., 1], E[..., 1]), label + " s2")
    return ratios


def gemm_out_shape(j, B, L):
    return (B, L, j.rows + j.os) if j.out_nlc else (B, j.rows + j.os, L)


def gemm_out_slice(j, full):
    """the job's rows of the full output tensor -> [rows, B L]"""
    return _slice_cols(full, j.oc0, j.rows, j.out_nlc)


def gemm_branches(j):
    """what the job reaches in the kernel (asserted by the CPU test)"""
    nch = kpad_of(j.K) // 16
    mtiles = (j.rows + 15) // 16
    per = (mtiles + 3) // 4
    xct, oct_ = j.K + j.xs, j.rows + j.os
    return {"nch": nch, "mtiles": mtiles, "dead_waves": sum(1 for w in range(4) if w * per >= mtiles),
            "second_trip": per > 4, "x_path": "ncl" if not j.x_nlc else ("scalar" if (j.K & 3 or xct & 3) else "vec"),
            "scalar_why": ("k" if j.K & 3 else "ctot" if xct & 3 else None) if j.x_nlc else None,
            "out_path": "ncl" if not j.out_nlc else ("vec" if not (j.rows & 3 or oct_ & 3 or j.oc0 & 3) else "scalar"),
            "out_why": None if not j.out_nlc else ("rows" if j.rows & 3 else "ctot" if oct_ & 3 else "ptr" if j.oc0 & 3 else None)}


def _row16_sum(s):
    """[..., 16] -> [...]: quad_perm [1,0,3,2], [2,3,0,1], row_half_mirror, row_mirror of p2r_row16_sum"""
    i = torch.arange(16)
    for perm in (i ^ 1, i ^ 2, (i & 8) | (7 - (i & 7)), 15 - i):
        s = s + s[..., perm]
    return s[..., 0]


def _tile_sum(t):
    """[..., 64] (column 16 n + r) -> [...]: the lane's (v0 + v1) + (v2 + v3), then the 16-lane row sum"""
    q = t.reshape(*t.shape[:-1], 4, 16)
    return _row16_sum((q[..., 0, :] + q[..., 1, :]) + (q[..., 2, :] + q[..., 3, :]))


def _lane_seq_sum(t):
    """[..., 64] -> [...]: four in-lane additions from zero in order n = 0..3, then the 16-lane row sum"""
    q = t.reshape(*t.shape[:-1], 4, 16)
    s = torch.zeros_like(q[..., 0, :])
    for n in range(4):
        s = s + q[..., n, :]
    return _row16_sum(s)


def emulate_gemm(j, ops, B, L, mutant=None, job0=None):
    """-> (out: the full NaN-filled output tensor with the job's slice written, stats [tiles][rows][3 | 2] or None).
    mutants: 'stale_group', 'kpad_rows_live', 'job0_dims' (k of `job0`, as far as it stays inside this job's tensors),
    'stats_row_clamped', 'gate_on_acc', 'dead_wave_unwritten' (the tile of a wave's second trip is not stored)"""
    K, rows = j.K, j.rows
    kpad, cols = kpad_of(K), B * L
    tile = torch.zeros(kpad, cols)
    tile[:K] = gemm_input(j, ops)
    if mutant == "kpad_rows_live" and j.w_t:
        tile[K:] = 1.0
    if mutant == "job0_dims" and job0 is not None and job0.K < K:
        tile[job0.K:] = 0.0
    A = torch.zeros(rows, kpad)
    Wm = ops["w"].t() if j.w_t else ops["w"]
    A[:, :K] = Wm
    if j.w_t and kpad > K:
        A[:, K:] = Wm[:, K - 1:K]                                    # kk clamped at K - 1: the tile rows there are zero
    nch = kpad // 16
    acc = torch.zeros(rows, cols)
    for c in range(nch):
        src = c - 8 if (mutant == "stale_group" and c >= 8 and c % 8 < 4) else c
        acc = acc + A[:, 16 * src:16 * src + 16] @ tile[16 * c:16 * c + 16]
    v = acc + (ops["bias"][:, None] if j.bias else 0.0)
    stats = None
    if j.epi == 1:
        gate = (acc > 0) if mutant == "gate_on_acc" else gemm_gate(j, ops)
        v = torch.where(gate, acc, torch.zeros(()))
    if j.stats:
        t = v.reshape(rows, -1, 64)

        def entries(t):
            if j.epi == 0:
                mean = _tile_sum(t) * (1.0 / 64.0)
                d = t - mean[..., None]
                return torch.stack([torch.full_like(mean, 64.0), mean, _lane_seq_sum(d * d)], -1)
            mz = _slice_cols(ops["mz"], j.mc0, rows, 0).reshape(rows, -1, 64)
            xhat = (mz - ops["mfin"][0, :rows, None, None]) * ops["mfin"][1, :rows, None, None]
            return torch.stack([_lane_seq_sum(t), _lane_seq_sum(t * xhat)], -1)
        stats = entries(t).transpose(0, 1).contiguous()
        if mutant == "stats_row_clamped" and rows % 16:
            # the lanes of rows >= `rows` hold row rows - 1 without its bias (epilogue 0) or zeros (epilogue 1)
            ghost = acc[rows - 1:].reshape(1, -1, 64) if j.epi == 0 else torch.zeros(1, cols // 64, 64)
            stats[:, rows - 1] = entries(ghost).transpose(0, 1)[:, 0] if j.epi == 0 else 0.0
    full = torch.full(gemm_out_shape(j, B, L), NAN)
    written = v.clone()
    if mutant == "dead_wave_unwritten" and (rows + 15) // 16 > 16:
        written[256:] = NAN
    view = (full.transpose(1, 2) if j.out_nlc else full)[:, j.oc0:j.oc0 + rows]
    view.copy_(cols_ncl(written, B, L))
    return full, stats


# ---- p2r_pw_wgrad ---------------------------------------------------------------------------------------------------------------
WGradJob = collections.namedtuple("WGradJob", "name rows K x_nlc y_nlc tr ytr db xs xc0 ys yc0 ld", defaults=(0, 0, 0, 0, 0))
WGRAD_DIMS = (1, 63, 64, 65, 129)
WGRAD_JOBS = [
    #         name          rows  K  xn yn tr yt db
    WGradJob("w1x1",          1,   1, 0, 0, 0, 0, 1),
    WGradJob("w63x64",       63,  64, 0, 0, 2, 1, 1),
    WGradJob("w64x65",       64,  65, 1, 0, 0, 1, 1),                 # NLC vector fetch of x (rows | ctot multiples of 4)
    WGradJob("w65x129",      65, 129, 1, 1, 0, 0, 1),                 # NLC scalar fetch of both
    WGradJob("w129x63",     129,  63, 0, 1, 2, 0, 0),                 # 3 x 1 tiles, no bias partial
    WGradJob("w129x129",    129, 129, 0, 0, 2, 1, 1),                 # 3 x 3 tiles
    WGradJob("w64x64_nlc",   64,  64, 1, 1, 2, 1, 1),                 # NLC vector fetch of x, x2 and y
    WGradJob("w65x1",        65,   1, 0, 0, 0, 1, 0),
    WGradJob("w63x65_slice", 63,  65, 0, 0, 2, 1, 1, 9, 4, 7, 3, 6),  # x_ctot > rows, y_ctot > k, tr_ld / ytr_ld beyond
    WGradJob("w64x64_nslice", 64, 64, 1, 1, 0, 1, 1, 4, 4, 8, 4, 0),  # NLC slices that keep the 16-byte fetch
    WGradJob("w1x129",        1, 129, 1, 0, 0, 1, 1),
]
WGRAD_BY_NAME = {j.name: j for j in WGRAD_JOBS}
WGRAD_COLUMNS = [(1, 64), (3, 64), (2, 128)]      # chunks 1, 3, 4; at (3, 64) with split 2 a range crosses a sample
WGRAD_LISTS = {3: ((3, 64), (("w1x1", 4), ("w129x129", 2), ("w64x65", 1))),
               8: ((2, 128), (("w63x64", 1), ("w64x65", 2), ("w65x129", 4), ("w129x63", 5), ("w1x1", 1), ("w64x64_nlc", 2),
                              ("w65x1", 3), ("w63x65_slice", 4)))}


def wgrad_splits(chunks):
    return sorted({1, 2, chunks, chunks + 1})


@functools.lru_cache(maxsize=None)
def wgrad_operands(name, B, L):
    j = WGRAD_BY_NAME[name]
    g = _gen("wgrad", name, B, L)
    randn = lambda *s: torch.randn(*s, generator=g)

    def act(ctot, c0, n, nlc):
        full = torch.full((B, ctot, L), NAN)
        full[:, c0:c0 + n] = randn(B, n, L)
        return full.transpose(1, 2).contiguous() if nlc else full

    ops = {"x": act(j.rows + j.xs, j.xc0, j.rows, j.x_nlc), "y": act(j.K + j.ys, j.yc0, j.K, j.y_nlc)}
    if j.tr == 2:
        ops["x2"] = act(j.rows + j.xs, j.xc0, j.rows, j.x_nlc)
        ops["tr"] = torch.full((3, j.rows + j.ld), NAN)
        ops["tr"][:, :j.rows] = randn(3, j.rows)
    if j.ytr:
        ops["ytr"] = torch.full((2, j.K + j.ld), NAN)
        ops["ytr"][0, :j.K] = 0.5 + torch.rand(j.K, generator=g)
        ops["ytr"][1, :j.K] = 0.3 * randn(j.K)
    return ops


def wgrad_inputs(j, ops):
    """(T(dz) [rows, B L], U(y) [K, B L]) in fp32, the kernel's operation order"""
    dz = _slice_cols(ops["x"], j.xc0, j.rows, j.x_nlc)
    if j.tr == 2:
        z = _slice_cols(ops["x2"], j.xc0, j.rows, j.x_nlc)
        tr = ops["tr"]
        dz = (tr[0, :j.rows, None] * dz + tr[1, :j.rows, None] * z) + tr[2, :j.rows, None]
    y = _slice_cols(ops["y"], j.yc0, j.K, j.y_nlc)
    if j.ytr:
        y = torch.relu(y * ops["ytr"][0, :j.K, None] + ops["ytr"][1, :j.K, None])
    return dz, y


def wgrad_ranges(chunks, split):
    cps = -(-chunks // split)
    return [(min(sp * cps, chunks), min(sp * cps + cps, chunks)) for sp in range(split)]


def wgrad_ref(j, ops, chunks, split):
    """-> {'dw': (value, E) [split][rows][K], 'db': (value, E) [split][rows]}"""
    dz, y = (t.double() for t in wgrad_inputs(j, ops))
    dw, Ew, db, Eb = [], [], [], []
    for lo, hi in wgrad_ranges(chunks, split):
        a, b = dz[:, 64 * lo:64 * hi], y[:, 64 * lo:64 * hi]
        n = a.shape[1]
        dw.append(a @ b.t()), Ew.append(gamma(n + 1) * (a.abs() @ b.abs().t()))
        db.append(a.sum(1)), Eb.append(gamma(16 + (hi - lo) + 2) * a.abs().sum(1))
    return {"dw": (torch.stack(dw), torch.stack(Ew)), "db": (torch.stack(db), torch.stack(Eb))}


def check_wgrad(j, dw, db, ref, chunks, split, label=""):
    label = label or f"{j.name} split {split}"
    ratios = {"dw": check_bound(dw, ref["dw"], label + " dw")}
    if db is not None:
        ratios["db"] = check_bound(db, ref["db"], label + " db")
    for sp, (lo, hi) in enumerate(wgrad_ranges(chunks, split)):
        if lo == hi:
            assert not dw[sp].any() and (db is None or not db[sp].any()), f"{label}: range {sp} has no chunk and is not zero"
    return ratios


def emulate_wgrad(j, ops, chunks, split, mutant=None):
    """mutants: 'drop_last_chunk', 'empty_range_unwritten'"""
    dz, y = wgrad_inputs(j, ops)
    dw, db = torch.full((split, j.rows, j.K), NAN), torch.full((split, j.rows), NAN)
    for sp, (lo, hi) in enumerate(wgrad_ranges(chunks, split)):
        if lo == hi and mutant == "empty_range_unwritten":
            continue
        acc, bsum = torch.zeros(j.rows, j.K), torch.zeros(j.rows, 4)
        for c in range(lo, hi - 1 if mutant == "drop_last_chunk" else hi):
            a, b = dz[:, 64 * c:64 * c + 64], y[:, 64 * c:64 * c + 64]
            for k in range(0, 64, 4):
                acc = acc + a[:, k:k + 4] @ b[:, k:k + 4].t()
            q = a.reshape(j.rows, 4, 16)
            s = torch.zeros(j.rows, 4)
            for i in range(16):
                s = s + q[:, :, i]
            bsum = bsum + s
        dw[sp] = acc
        bsum = bsum + bsum[:, [1, 0, 3, 2]]
        bsum = bsum + bsum[:, [2, 3, 0, 1]]
        db[sp] = bsum[:, 0]
    return dw, (db if j.db else None)


# ---- p2r_pw_reduce ----------------------------------------------------------------------------------------------------------------
REDUCE_P = (1, 2, 3, 4, 5, 7, 8, 9)
REDUCE_M = (1, 255, 256, 257, 513)


@functools.lru_cache(maxsize=None)
def reduce_case(P, M):
    return torch.randn(P, M, generator=_gen("reduce", P, M))


def reduce_ref(inp):
    P = inp.shape[0]
    return inp.double().sum(0), gamma(P // 4 + P % 4 + 2) * inp.double().abs().sum(0)


def emulate_reduce(inp, mutant=None):
    """mutant 'reduce_drop_tail': the P % 4 remainder is dropped"""
    P, M = inp.shape
    a = [torch.zeros(M) for _ in range(4)]
    p = 0
    while p + 4 <= P:
        for u in range(4):
            a[u] = a[u] + inp[p + u]
        p += 4
    while p < P and mutant != "reduce_drop_tail":
        a[0] = a[0] + inp[p]
        p += 1
    return (a[0] + a[1]) + (a[2] + a[3])


# ---- p2r_pw_bn_finalize / p2r_pw_bn_bwd_finalize --------------------------------------------------------------------------------
FIN_P = (1, 63, 64, 65, 130)
FIN_C = (1, 5, 96)
FIN_MOMENTUM = (0.1, 1.0, 0.0, -1.0)
FIN_KINDS = ("plain", "big", "const")


@functools.lru_cache(maxsize=None)
def finalize_case(P, C, kind="plain"):
    """bn_cases.finalize_case (unequal counts, 'big': |mean| / std = 1000).  'const': channel 0 holds one value in every
    entry (M2 = 0 exactly, invstd = 1 / sqrt(eps))."""
    case = dict(bn_cases.finalize_case(P, C, 3, kind == "big"))
    if kind == "const":
        part = case["part"].clone()
        part[:, 0, 1], part[:, 0, 2] = 0.7109375, 0.0
        case["part"] = part
    return case


def finalize_ref(case, momentum, eps=EPS):
    return bn_cases.finalize_ref(case, momentum, eps)


def check_finalize(got, ref, label=""):
    return bn_cases.check_finalize(got, ref, label)


def _wave_sum(vals):
    """[P, C] float64 -> [C]: lane l adds the entries l, l + 64, ..., then six xor-shuffle steps"""
    P, C = vals.shape
    trips = -(-P // 64)
    pad = torch.zeros(trips * 64, C, dtype=vals.dtype)
    pad[:P] = vals
    acc = torch.zeros(64, C, dtype=vals.dtype)
    for k in range(trips):
        acc = acc + pad[64 * k:64 * k + 64]
    lane = torch.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[lane ^ off]
    return acc[0]


def emulate_finalize(case, momentum, eps=EPS, mutant=None):
    """pw_bn_finalize_kernel.  mutants: 'merge_no_between', 'biased_running_var', 'fin_first_trip' (the lane loop runs once)"""
    part = case["part"].double()
    if mutant == "fin_first_trip":
        part = part[:64]
    n = _wave_sum(part[..., 0])
    mean = _wave_sum(part[..., 0] * part[..., 1]) / n
    d = part[..., 1] - mean
    m2 = _wave_sum(part[..., 2] + (0.0 if mutant == "merge_no_between" else part[..., 0] * d * d))
    return bn_cases._finalize_from(mean, m2, n, case, momentum, eps, biased=mutant == "biased_running_var", bounds=False)


@functools.lru_cache(maxsize=None)
def bwd_finalize_case(P, C):
    """partials [P][C][2], fin [4][C], the element count M"""
    g = _gen("bwdfin", P, C)
    part = torch.randn(P, C, 2, generator=g) * 3.0
    mean, invstd = torch.randn(C, generator=g), 0.5 + torch.rand(C, generator=g)
    scale = (0.5 + torch.rand(C, generator=g)) * invstd
    fin = torch.stack([mean, invstd, scale, torch.rand(C, generator=g) - 0.5 - mean * scale]).contiguous()
    return part, fin, float(64 * max(P, 4))


def bwd_finalize_ref(part, fin, M, train):
    S = part.double().sum(0)
    return bn_bwd_coef_ref(S[:, 0], S[:, 1], fin, M, train)


def check_bwd_finalize(got, ref, label=""):
    return {k: check_bound(got[k], ref[k], f"{label} {k}") for k in ("coef", "dgamma", "dbeta") if got.get(k) is not None}


def emulate_bwd_finalize(part, fin, M, train, mutant=None):
    p = part.double()[:64] if mutant == "fin_first_trip" else part.double()
    s, q = _wave_sum(p[..., 0]), _wave_sum(p[..., 1])
    mean, invstd, scale = fin[0], fin[1], fin[2]
    if train:
        m1, m2 = (s / M).float(), (q / M).float()
        coef = torch.stack([scale, -scale * invstd * m2, -scale * m1 + scale * invstd * m2 * mean])
    else:
        coef = torch.stack([scale, torch.zeros_like(scale), torch.zeros_like(scale)])
    return {"coef": coef, "dgamma": q.float(), "dbeta": s.float()}


# ---- p2r_mdn_mix_forward / p2r_mdn_mix_backward -----------------------------------------------------------------------------------
MIX_COLS = [(1, 1), (1, 15), (1, 16), (1, 17), (3, 37), (1, 257), (5, 120)]        # B L = 1, 15, 16, 17, 111, 257, 600
MIX_G = (1, 15, 16, 17, 100)
MIX_D = (1, 2, 3, 4)
MixHead = collections.namedtuple("MixHead", "D f64 eps")
MIX_LAUNCH = (MixHead(3, 0, 1), MixHead(2, 1, 1), MixHead(1, 0, 0), MixHead(4, 1, 0))     # four heads of mixed D / type
MIX_LAUNCH_SWAPPED = (MixHead(3, 1, 0), MixHead(2, 0, 0), MixHead(1, 1, 1), MixHead(4, 0, 1))   # the other type and noise of each D
MIX_LAUNCHES = (MIX_LAUNCH, MIX_LAUNCH_SWAPPED)


@functools.lru_cache(maxsize=None)
def mix_case(B, L, G, D, f64, extra=0, c0=0):
    """logit (B, G + extra, L) with the head's rows from c0 (the others NaN), mu, log_sigma [G][D], eps (B L, G, D),
    dpred (B, L, D); mu / eps / dpred in the head's type"""
    g = _gen("mix", B, L, G, D, f64, extra, c0)
    dt = torch.float64 if f64 else torch.float32
    logit = torch.full((B, G + extra, L), NAN)
    logit[:, c0:c0 + G] = 2.5 * torch.randn(B, G, L, generator=g)
    return {"logit": logit, "mu": torch.randn(G, D, generator=g, dtype=dt),
            "log_sigma": torch.rand(G, D, generator=g) * 1.5 - 1.5, "eps": torch.randn(B * L, G, D, generator=g, dtype=dt),
            "dpred": torch.randn(B, L, D, generator=g, dtype=dt), "c0": c0, "G": G}


def _mix_terms(c, with_eps):
    lg = c["logit"][:, c["c0"]:c["c0"] + c["G"]].double()                      # (B, G, L)
    B, G, L = lg.shape
    p = torch.sigmoid(lg).permute(0, 2, 1).reshape(B * L, G)                  # [col][g]
    sig = c["log_sigma"].double().exp()
    es = c["eps"].double() * sig if with_eps else torch.zeros(B * L, G, c["mu"].shape[1], dtype=torch.float64)
    return p, sig, es, c["mu"].double()


def _comp_err(es, mu, f64):
    """error of comp = eps sig + mu as formed: sig carries D_EXP; in f32 the product and the addition round"""
    E = es.abs() * D_EXP
    return E if f64 else E + gamma(2) * (es.abs() + mu.abs() + E)


def pi_ref(c):
    lg = c["logit"][:, c["c0"]:c["c0"] + c["G"]].double()
    p = torch.sigmoid(lg)
    return p, D_P * p


def pi_ulps(pi, c):
    """max |pi - float64 sigmoid| in ulps of the float64 value (what EXPF_ULP is taken from)"""
    p = pi_ref(c)[0]
    ulp = torch.exp2(torch.floor(torch.log2(p)) - 23)
    return float(((pi.double() - p).abs() / ulp).max())


def mix_forward_ref(c, with_eps):
    """-> (pred, E) (B, L, D) float64"""
    p, sig, es, mu = _mix_terms(c, with_eps)
    f64 = c["mu"].dtype == torch.float64
    G = c["G"]
    comp = es + mu
    Ec = _comp_err(es, mu, f64) if with_eps else torch.zeros_like(comp)
    term = comp * p[..., None]
    Et = Ec * p[..., None] + (comp.abs() + Ec) * p[..., None] * D_P
    if not f64:
        Et = Et + gamma(1 + -(-G // 16) + 16) * (term.abs() + Et)
    B, _, L = c["logit"].shape
    return term.sum(1).reshape(B, L, -1), Et.sum(1).reshape(B, L, -1)


def mix_backward_ref(c):
    """-> {'dlogit': (value, E) (B, G, L), 'dmu': [G][D], 'dlog_sigma': [G][D]}"""
    p, sig, es, mu = _mix_terms(c, True)
    f64 = c["mu"].dtype == torch.float64
    B, _, L = c["logit"].shape
    cols, G, D = B * L, c["G"], mu.shape[1]
    dp = c["dpred"].double().reshape(cols, 1, D)
    comp = es + mu
    Ec = _comp_err(es, mu, f64)
    t = (dp * comp).sum(-1)                                                   # [col][g]
    Et = (dp.abs() * Ec).sum(-1) + (0.0 if f64 else gamma(1 + D) * (dp.abs() * (comp.abs() + Ec)).sum(-1))
    if f64:
        Et = Et + gamma(1) * (t.abs() + Et)                                   # (float) t
    Ep = D_P * p
    q = p * (1 - p)
    Eq = Ep * (1 - p) + p * (Ep + gamma(1) * (1 - p + Ep)) + gamma(1) * (q + Ep)
    dl = t * q
    Edl = Et * (q + Eq) + t.abs() * Eq + gamma(1) * (dl.abs() + Et * (q + Eq) + t.abs() * Eq)
    to_bgl = lambda m: m.reshape(B, L, G).permute(0, 2, 1).contiguous()
    n = -(-cols // 256)
    ds = dp * p[..., None]                                                    # [col][g][d]
    Eds = ds.abs() * (D_P + (0.0 if f64 else gamma(1) * (1 + D_P)))
    dmu = ds.sum(0)
    Edmu = Eds.sum(0) + (0.0 if f64 else gamma(n + 1)) * (ds.abs() + Eds).sum(0)
    e = c["eps"].double()
    cs = (ds * e).sum(0)
    Ecs = (Eds * e.abs()).sum(0) + (0.0 if f64 else gamma(n + 1)) * ((ds.abs() + Eds) * e.abs()).sum(0)
    dls = cs * sig
    Edls = Ecs * sig * (1 + D_EXP) + cs.abs() * sig * D_EXP + gamma(2) * (cs.abs() + Ecs) * sig * (1 + D_EXP)
    return {"dlogit": (to_bgl(dl), to_bgl(Edl)), "dmu": (dmu, Edmu), "dlog_sigma": (dls, Edls)}


def check_bound_any(got, ref, label=""):
    """check_bound for f32 or f64 results"""
    assert got.shape == ref[0].shape, f"{label}: shape {tuple(got.shape)}"
    assert not torch.isnan(got).any(), f"{label}: NaN (an element never written?)"
    ratio, at = worst(got, *ref)
    assert ratio <= 1, f"{label}: error / bound {ratio:.3f} at {at}"
    return ratio


def emulate_mix_forward(c, with_eps, mutant=None):
    """-> (pred (B, L, D) in mu's type, pi (B, G, L) f32).  mutants: 'mix_cols_16', 'mix_slice_16'"""
    B, _, L = c["logit"].shape
    G, mu = c["G"], c["mu"]
    D, T = mu.shape[1], mu.dtype
    cols = B * L
    lg = c["logit"][:, c["c0"]:c["c0"] + G].permute(0, 2, 1).reshape(cols, G)
    p = 1.0 / (1.0 + torch.exp(-lg))
    comp = mu[None].expand(cols, G, D)
    if with_eps:
        comp = c["eps"] * torch.exp(c["log_sigma"]).to(T) + mu
    term = comp * p.to(T)[..., None]
    Gu = 16 * (G // 16) if mutant == "mix_slice_16" else G
    red = torch.zeros(16, cols, D, dtype=T)
    for s in range(16):
        for gi in range(s, Gu, 16):
            red[s] = red[s] + term[:, gi]
    tot = torch.zeros(cols, D, dtype=T)
    for s in range(16):
        tot = tot + red[s]
    pred = torch.full((cols, D), NAN, dtype=T)
    live = 16 * (cols // 16) if mutant == "mix_cols_16" else cols
    pred[:live] = tot[:live]
    pi = torch.full((cols, G), NAN)
    pi[:live, :Gu] = p[:live, :Gu]
    return pred.reshape(B, L, D), pi.reshape(B, L, G).permute(0, 2, 1).contiguous()


def emulate_mix_backward(c, mutant=None):
    """-> dlogit (B, G, L) f32, dmu [G][D] in mu's type, dlog_sigma [G][D] f32.  mutant 'mix_stride_once': columns >= 256 lost"""
    B, _, L = c["logit"].shape
    G, mu = c["G"], c["mu"]
    D, T = mu.shape[1], mu.dtype
    cols = B * L
    lg = c["logit"][:, c["c0"]:c["c0"] + G].permute(0, 2, 1).reshape(cols, G)
    p = 1.0 / (1.0 + torch.exp(-lg))
    sig = torch.exp(c["log_sigma"])
    e, dp = c["eps"], c["dpred"].reshape(cols, 1, D)
    comp = e * sig.to(T) + mu
    t = torch.zeros(cols, G, dtype=T)
    for d in range(D):
        t = t + dp[..., d] * comp[..., d]
    dl = t.float() * (p * (1.0 - p))
    live = min(cols, 256) if mutant == "mix_stride_once" else cols
    if live < cols:
        dl[live:] = NAN
    ds = dp * p.to(T)[..., None]
    smu, ssg = torch.zeros(256, G, D, dtype=T), torch.zeros(256, G, D, dtype=T)
    for k in range(0, live, 256):
        blk = ds[k:min(k + 256, live)]
        smu[:blk.shape[0]] = smu[:blk.shape[0]] + blk
        ssg[:blk.shape[0]] = ssg[:blk.shape[0]] + blk * e[k:k + blk.shape[0]]
    dmu = smu.double().sum(0).to(T)
    dls = ssg.double().sum(0).to(T).float() * sig
    return dl.reshape(B, L, G).permute(0, 2, 1).contiguous(), dmu, dls


# ---- p2r_vote_finish / p2r_vote_finish_grad ---------------------------------------------------------------------------------------
VOTE_COLUMNS = [(1, 64), (3, 64), (2, 128)]
VF_C = 256


@functools.lru_cache(maxsize=None)
def vote_case(B, S, zero_at=None):
    """net (B,S,259), seed_features (B,S,256), hip (B,S,3), and the backward's d_xyz (B,S,3), d_feat (B,256,S).
    zero_at = (b, s): that seed's seed_features = -net[3:], a row of zero norm"""
    g = _gen("vote", B, S, zero_at)
    net, sf = torch.randn(B, S, 3 + VF_C, generator=g), torch.randn(B, S, VF_C, generator=g)
    if zero_at is not None:
        sf[zero_at] = -net[zero_at][3:]
    return {"net": net, "sf": sf, "hip": torch.randn(B, S, 3, generator=g), "d_xyz": torch.randn(B, S, 3, generator=g),
            "d_feat": torch.randn(B, VF_C, S, generator=g)}


def vote_finish_ref(c):
    """-> {'xyz': fp32 (exact), 'feat': (value, E) (B,256,S), 'inv': (value, E) (B,S)}; a zero-norm seed: inv = inf, feat NaN"""
    f = c["sf"].double() + c["net"][..., 3:].double()
    inv = 1.0 / f.pow(2).sum(-1).sqrt()
    rel = gamma(12) / 2 * (1 + gamma(12)) + gamma(2)
    feat = f * inv[..., None]
    return {"xyz": c["hip"] + c["net"][..., :3], "feat": (feat.transpose(1, 2), (rel + gamma(2)) * feat.abs().transpose(1, 2)),
            "inv": (inv, rel * inv)}


def check_vote_finish(xyz, feat, inv, ref, zero_at=None, label=""):
    assert not torch.isnan(xyz).any() and torch.equal(xyz, ref["xyz"]), f"{label}: vote_xyz is not hip + net[:3]"
    fv, fE = (t.clone() for t in ref["feat"])
    iv, iE = (t.clone() for t in ref["inv"])
    feat, inv = feat.clone(), inv.clone()
    if zero_at is not None:
        b, s = zero_at
        assert torch.isnan(feat[b, :, s]).all() and inv[b, s] == float("inf"), f"{label}: the zero-norm seed is not 0 / 0"
        for t in (feat, fv, fE):
            t[b, :, s] = 0.0
        for t in (inv, iv, iE):
            t[b, s] = 0.0
    return {"feat": check_bound(feat, (fv, fE), label + " feat"), "inv": check_bound(inv, (iv, iE), label + " inv")}


def vote_grad_inputs(c):
    """feat (B,256,S), inv (B,S) fp32 as a correct forward leaves them (rounded from float64)"""
    ref = vote_finish_ref(c)
    return ref["feat"][0].float().contiguous(), ref["inv"][0].float()


def vote_grad_ref(c, feat, inv, with_xyz=True, with_feat=True):
    """-> {'d_xyz': fp32 exact, 'df': (value, E) (B,S,256)} on the kernel's own feat / inv"""
    y = feat.double().transpose(1, 2)
    g = c["d_feat"].double().transpose(1, 2) if with_feat else torch.zeros_like(y)
    dot = (g * y).sum(-1, keepdim=True)
    Edot = gamma(10) * (g * y).abs().sum(-1, keepdim=True)
    i = inv.double()[..., None]
    df = i * (g - y * dot)
    E = i * (y.abs() * Edot + gamma(3) * (y * dot).abs() + gamma(2) * g.abs())
    return {"d_xyz": c["d_xyz"] if with_xyz else torch.zeros_like(c["d_xyz"]), "df": (df, E)}


def check_vote_grad(d_net, d_sf, ref, zero_at=None, label=""):
    from tests import memguard
    assert memguard.same_bits(d_net[..., 3:].contiguous(), d_sf), f"{label}: d_sf is not d_net[3:]"
    assert torch.equal(d_net[..., :3], ref["d_xyz"]), f"{label}: d_net[:3] is not d_xyz"
    df, (v, E) = d_sf.clone(), (t.clone() for t in ref["df"])
    if zero_at is not None:
        assert not torch.isfinite(df[zero_at]).any(), f"{label}: the zero-norm seed has a finite gradient"
        df[zero_at], v[zero_at], E[zero_at] = 0.0, 0.0, 0.0
    return {"df": check_bound(df, (v, E), label + " df")}


def emulate_vote_finish(c):
    f = c["sf"] + c["net"][..., 3:]
    q = (f * f).reshape(*f.shape[:-1], 4, 64)                    # channel lane + 64 e
    ss = (q[..., 0, :] + q[..., 1, :]) + (q[..., 2, :] + q[..., 3, :])
    lane = torch.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        ss = ss + ss[..., lane ^ off]
    inv = 1.0 / torch.sqrt(ss[..., 0])
    return c["hip"] + c["net"][..., :3], (f * inv[..., None]).transpose(1, 2).contiguous(), inv


def emulate_vote_grad(c, feat, inv, with_xyz=True, with_feat=True):
    y = feat.transpose(1, 2)
    g = c["d_feat"].transpose(1, 2) if with_feat else torch.zeros_like(y)
    q = (g * y).reshape(*y.shape[:-1], 4, 64)
    dot = (q[..., 0, :] + q[..., 1, :]) + (q[..., 2, :] + q[..., 3, :])
    lane = torch.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        dot = dot + dot[..., lane ^ off]
    df = inv[..., None] * (g - y * dot[..., :1])
    dx = c["d_xyz"] if with_xyz else torch.zeros_like(c["d_xyz"])
    return torch.cat([dx, df], -1), df.contiguous()


# ---- p2r_rowsum_short -------------------------------------------------------------------------------------------------------------
ROWSUM_ROWS = (1, 255, 256, 257)


@functools.lru_cache(maxsize=None)
def rowsum_case(rows, V):
    return torch.randn(rows, V, generator=_gen("rowsum", rows, V))


def rowsum_ref(x, scale):
    V = x.shape[1]
    return x.double().sum(1) * scale, gamma(-(-V // 2) + 2) * x.double().abs().sum(1) * abs(scale)


def emulate_rowsum(x, scale, mutant=None):
    """mutant 'rowsum_odd_tail': the last element of an odd row is lost"""
    rows, V = x.shape
    a0, a1 = torch.zeros(rows), torch.zeros(rows)
    v = 0
    while v + 2 <= V:
        a0, a1 = a0 + x[:, v], a1 + x[:, v + 1]
        v += 2
    if v < V and mutant != "rowsum_odd_tail":
        a0 = a0 + x[:, v]
    return (a0 + a1) * torch.tensor(scale, dtype=torch.float32)


# ---- p2r_gather_frames / p2r_gather_frames_grad -----------------------------------------------------------------------------------
GATHER_CJ = [(1, 1), (5, 51), (4, 64), (1, 257)]              # C J = 1, 255, 256, 257
GRAD_T = (1, 7, 8, 9, 13)
GRAD_C = (1, 7, 8, 9)
GRAD_J = (1, 5, 53)


def designed_inds_40():
    """T = 13, S = 40: frames 0..5 are picked 17, 16, 3, 2, 1, 0 times, frame 12 (the ragged chunk) once, in a
    shuffled seed order"""
    picks = [0] * 17 + [1] * 16 + [2] * 3 + [3] * 2 + [4] + [12]
    assert len(picks) == 40
    order = torch.randperm(40, generator=_gen("inds40"))
    return torch.tensor(picks)[order].reshape(1, 40)


def designed_inds_130():
    """T = 13, S = 130: frame 3 is picked by the seeds {0, 63, 64, 65, 129} (three ballot trips), frame 9 17 times across
    the three trips, seeds 5 and 70 are out of range (-1 and T), the rest picks frames 0..12 other than 3 and 9 at most
    twice each ... or nothing (out of range)"""
    inds = torch.full((130,), -1, dtype=torch.int64)
    inds[[0, 63, 64, 65, 129]] = 3
    nine = [1, 2, 7, 20, 40, 62, 66, 67, 80, 90, 100, 127, 128, 10, 11, 12, 13]
    assert len(nine) == 17
    inds[nine] = 9
    inds[70] = 13
    for k, s in enumerate((3, 4, 30, 31, 95, 96, 110, 111, 120, 121)):
        inds[s] = (0, 0, 1, 5, 5, 6, 7, 12, 12, 11)[k]
    return inds.reshape(1, 130)


def hit_counts(inds, T):
    """(B, S) -> (B, T): seeds per frame, out-of-range indices nowhere"""
    B = inds.shape[0]
    out = torch.zeros(B, T, dtype=torch.int64)
    for b in range(B):
        ok = (inds[b] >= 0) & (inds[b] < T)
        out[b] = torch.bincount(inds[b][ok], minlength=T)
    return out


def ballot_trips(inds, t):
    """the 64-seed ballot trips (of sample 0) in which frame t has a hit"""
    return sorted({int(s) // 64 for s in (inds[0] == t).nonzero().flatten()})


def gather_ref(x, inds):
    """x (B,C,T,J), inds (B,S) -> (B,S,C J); an index outside [0, T) gives a zero row"""
    B, C, T, J = x.shape
    out = torch.zeros(B, inds.shape[1], C * J)
    for b in range(B):
        for s, t in enumerate(inds[b].tolist()):
            if 0 <= t < T:
                out[b, s] = x[b, :, t].reshape(-1)
    return out


def gather_grad_ref(dout, inds, C, T, J):
    """sequential fp32 additions in ascending seed order; a frame nobody picked is exactly 0"""
    B, S = inds.shape
    dx = torch.zeros(B, C, T, J)
    for b in range(B):
        for s, t in enumerate(inds[b].tolist()):
            if 0 <= t < T:
                dx[b, :, t] = dx[b, :, t] + dout[b, s].reshape(C, J)
    return dx


def emulate_gather_grad(dout, inds, C, T, J, mutant=None):
    """gather_frames_grad_kernel: chunks of 8 frames, per frame the hits of each 64-seed ballot trip in ascending order
    into a list of 16; counts <= 2, <= 16, > 16 (scan).  mutants: 'hits_overflow' (only the list is added),
    'ragged_frames' (the frames of a last partial chunk are not written)"""
    B, S = inds.shape
    dx = torch.full((B, C, T, J), NAN)
    for b in range(B):
        for t0 in range(0, T, GF_TT):
            if mutant == "ragged_frames" and t0 + GF_TT > T:
                continue
            for t in range(t0, min(t0 + GF_TT, T)):
                hits, cnt = [], 0
                for s0 in range(0, S, 64):
                    trip = [s for s in range(s0, min(s0 + 64, S)) if int(inds[b, s]) == t]
                    hits += trip[:max(0, GF_MAXHIT - cnt)]
                    cnt += len(trip)
                if cnt > GF_MAXHIT and mutant != "hits_overflow":
                    hits = [s for s in range(S) if int(inds[b, s]) == t]
                acc = torch.zeros(C, J)
                for s in hits:
                    acc = acc + dout[b, s].reshape(C, J)
                dx[b, :, t] = acc
    return dx


# ---- p2r_nearest_prefix -------------------------------------------------------------------------------------------------------------
PREFIX_T = (1, 2, 255, 257, 16384, 16385, 40000)
PREFIX_S = (1, 255, 256, 257)
PREFIX_MAX_T = 40000


def prefix_case(B, T, S, seed=0):
    """cumulative arc lengths with plateaus and exactly representable steps, and the model's targets (exact mid-points)"""
    g = _gen("prefix", B, T, S, seed)
    cum = cases.arc_length_case(B, T, S, g) if T > 1 else torch.zeros(B, 1)
    stride = cum[:, -1] / max(S - 1, 1)
    return cum, stride.unsqueeze(-1) * torch.arange(S, dtype=torch.float)


def nearest_prefix_ref(cum, target):
    """first index of the fp32 minimum of |cum - target|.  NaN: a NaN distance at t >= 1 never wins (the comparison d < best
    is false), a NaN distance at t = 0 is never displaced: index 0.  Without NaN this is torch.argmin."""
    d = (cum[:, :, None] - target[:, None, :]).abs()              # (B, T, S)
    nan0 = torch.isnan(d[:, 0])
    arg = torch.where(torch.isnan(d), torch.full_like(d, float("inf")), d).argmin(1)      # the first minimum
    return torch.where(nan0, torch.zeros_like(arg), arg)


assert math.isclose(D_P, D_EXP + gamma(2)) and EXPF_ULP == max(2, math.ceil(2 * PI_ULP_MEASURED))


# ---- op level: the module chains in float64 ------------------------------------------------------------------------------------------
OP_COLUMNS = COLUMNS          # 64 columns are the whole batch of a BatchNorm: the unbiased factor 64 / 63 is visible
OP_KINDS = ("vote_head", "votes_normalized", "proposal_heads")
# the max-norm tolerances of tests/test_pw_gpu.py (|got - want| <= tol max |want|), borrowed, here against float64
OP_TOL = {"vote_head": {"out": 1e-5, "dx": 2e-4, "param": 2e-4, "buffer": 1e-5},
          "votes_normalized": {"out": 1e-5, "dx": 2e-4, "dxyz": 1e-6, "param": 2e-4, "buffer": 1e-5},
          "proposal_heads": {"out": 2e-5, "dx": 2e-4, "param": 3e-4, "buffer": 1e-5}}
OP_FALLBACK_S = 96            # S % 64 != 0: `*_supported` is false


@functools.lru_cache(maxsize=None)
def _net():
    from tests.test_model_cpu import build
    return build("train", 256)[0]


def op_module(kind):
    """a fresh fp32 CPU copy of the module `kind` runs through (CenterVoteModule / ProposalNet), weights as the model tests"""
    import copy
    net = _net()
    return copy.deepcopy(net.detection if kind == "proposal_heads" else net.centervoting)


@functools.lru_cache(maxsize=None)
def op_inputs(kind, B, S, call=0):
    r = lambda shape, seed: cases.seeded_randn(shape, 100 * call + seed)
    if kind == "proposal_heads":
        G = _net().detection.gmm_center.mdn.mu.shape[0]
        return {"feats": r((B, 256, S), 1), "eps_center": r((B * S, G, 1, 3), 2), "eps_size": r((B * S, G, 1, 3), 3),
                "eps_heading": r((B * S, G, 1, 2), 4).double(), "g_center": r((B, 3, S), 5), "g_size": r((B, 3, S), 6),
                "g_heading": r((B, 2, S), 7).double(), "g_sem": r((B, 24, S), 8)}
    return {"seed_xyz": r((B, S, 53, 3), 1), "feats": r((B, S, 256), 2), "g_xyz": r((B, S, 3), 3), "g_feat": r((B, 256, S), 4),
            "g_net": r((B, 259, S), 5)}


def _instrument(module):
    """forward hooks on every conv -> BatchNorm -> ReLU layer of a float64 module: the conv input, the BatchNorm input and
    output (before the in-place ReLU) and the gradient that reaches the ReLU's output"""
    recs = []
    for name, sc in module.named_modules():
        if not (hasattr(sc, "batchnorm") and hasattr(sc, "conv") and hasattr(sc, "ReLU")):
            continue
        rec = {"name": name, "sc": sc}
        sc.conv.register_forward_hook(lambda m, i, o, rec=rec: rec.__setitem__("x", i[0].detach()))
        sc.batchnorm.register_forward_hook(lambda m, i, o, rec=rec: rec.update(z=i[0].detach(), pre=o.detach().clone()))

        def relu_hook(m, i, o, rec=rec):
            if o.requires_grad:
                o.register_hook(lambda g, rec=rec: rec.__setitem__("g", g.detach().clone()))
        sc.ReLU.register_forward_hook(relu_hook)
        recs.append(rec)
    return recs


def _bands(recs, train):
    """per layer: the gates within the layer's own bound of zero, and what each moves in the per-channel sums.
    E_pre = |scale| gamma(K + 2) |W| |x| + gamma(2) (|z scale| + |shift|): the product's bound through the affine form the
    consumer evaluates (z scale + shift, two roundings)."""
    out = {}
    for rec in recs:
        sc, x, z, pre = rec["sc"], rec["x"], rec["z"], rec["pre"]
        W = sc.conv.weight.detach()[:, :, 0]
        bn = sc.batchnorm
        mag = torch.einsum("oc,bcl->bol", W.abs(), x.abs())
        mean, var = (z.mean((0, 2)), z.var((0, 2), unbiased=False)) if train else (rec["rm"], rec["rv"])
        scale = bn.weight.detach() * (var + bn.eps).rsqrt()
        shift = bn.bias.detach() - mean * scale
        c = lambda v: v[None, :, None]
        E = c(scale.abs()) * gamma(W.shape[1] + 2) * mag + gamma(2) * ((z * c(scale)).abs() + c(shift.abs()))
        und = pre.abs() <= E
        g = rec.get("g", torch.zeros_like(pre))
        xhat = (pre - c(bn.bias.detach())) / c(bn.weight.detach())
        out[rec["name"]] = {"share": float(und.double().mean()), "count": int(und.sum()), "n": und.numel(),
                            "dbeta": (und * g.abs()).sum((0, 2)), "dgamma": (und * (g * xhat).abs()).sum((0, 2))}
    return out


def op_ref(kind, B, S, train, momentum_none=False, calls=1):
    """the module chain in float64 on the CPU -> {'out': {...}, 'grad': {...}, 'param': {name: grad}, 'buffer': {name: value},
    'bands': per-layer undecided gates} after `calls` consecutive forward / backward passes (gradients of the last)"""
    mod = op_module(kind).double().train(train)
    if momentum_none:
        for m in mod.modules():
            if isinstance(m, torch.nn.BatchNorm1d):
                m.momentum = None
    recs = _instrument(mod)
    for call in range(calls):
        mod.zero_grad()
        for rec in recs:
            rec["rm"], rec["rv"] = rec["sc"].batchnorm.running_mean.clone(), rec["sc"].batchnorm.running_var.clone()
        inp = {k: v.double() for k, v in op_inputs(kind, B, S, call).items()}
        feats = inp["feats"].clone().requires_grad_(True)
        grads = {}
        if kind == "proposal_heads":
            outs = {"center": mod.gmm_center.predict(mod.conv_center(feats), eps=inp["eps_center"]),
                    "size": mod.gmm_size.predict(mod.conv_size(feats), eps=inp["eps_size"]),
                    "heading": mod.gmm_heading.predict(mod.conv_heading(feats), eps=inp["eps_heading"]),
                    "sem": mod.conv_sem_obj(feats)}
            sum((outs[k] * inp["g_" + k]).sum() for k in outs).backward()
        elif kind == "vote_head":
            outs = {"net": mod.conv_input(feats.transpose(1, 2))}
            (outs["net"] * inp["g_net"]).sum().backward()
        else:
            xyz_in = inp["seed_xyz"].clone().requires_grad_(True)
            net = mod.conv_input(feats.transpose(1, 2)).transpose(1, 2)
            f = feats + net[..., 3:]
            outs = {"xyz": xyz_in[:, :, mod.origin_joint_id] + net[..., :3], "feat": f / f.norm(p=2, dim=2, keepdim=True)}
            ((outs["xyz"] * inp["g_xyz"]).sum() + (outs["feat"].transpose(1, 2) * inp["g_feat"]).sum()).backward()
            grads["dxyz"] = xyz_in.grad
        grads["dx"] = feats.grad
    return {"out": {k: v.detach() for k, v in outs.items()}, "grad": grads,
            "param": {n: p.grad for n, p in mod.named_parameters() if p.grad is not None},
            "buffer": {n: b.detach().clone() for n, b in mod.named_buffers()}, "bands": _bands(recs, train)}


def op_check(kind, got, ref, label=""):
    """got: the same dict layout from the device (CPU tensors).  Max-norm tolerances of OP_TOL; the BatchNorm weight / bias
    gradient of a layer gets, per channel, the terms of that layer's undecided gates on top.  Nothing is masked out.
    -> {name: error / tolerance}"""
    tol = OP_TOL[kind]
    ratios = {}

    def rel(a, b, t, slack=None, what=""):
        b = b.double()
        assert a.shape == b.shape, f"{label} {what}: shape {tuple(a.shape)} vs {tuple(b.shape)}"
        assert torch.isfinite(a).all(), f"{label} {what}: non-finite"
        err = (a.double() - b).abs()
        allowed = t * b.abs().max() + (0.0 if slack is None else slack)
        ratio = float((err / (allowed + 1e-300)).max())
        assert ratio <= 1, f"{label} {what}: error / tolerance {ratio:.3f}"
        return ratio

    for k, v in ref["out"].items():
        assert got["out"][k].dtype == (F64_OUT if (kind == "proposal_heads" and k == "heading") else torch.float32), k
        ratios["out." + k] = rel(got["out"][k], v, tol["out"], what=k)
    for k, v in ref["grad"].items():
        ratios[k] = rel(got["grad"][k], v, tol[k], what=k)
    assert set(got["param"]) == set(ref["param"]), f"{label}: gradients of {sorted(set(got['param']) ^ set(ref['param']))}"
    worst = 0.0
    for n, v in ref["param"].items():
        slack = None
        layer, _, leaf = n.rpartition(".batchnorm.")
        if leaf in ("weight", "bias") and layer in ref["bands"]:
            slack = ref["bands"][layer]["dgamma" if leaf == "weight" else "dbeta"]
        worst = max(worst, rel(got["param"][n], v, tol["param"], slack, n))
    ratios["param"] = worst
    worst = 0.0
    for n, v in ref["buffer"].items():
        if n.endswith("num_batches_tracked"):
            assert int(got["buffer"][n]) == int(v), f"{label} {n}: {int(got['buffer'][n])} steps, the chain counts {int(v)}"
        else:
            worst = max(worst, rel(got["buffer"][n], v, tol["buffer"], what=n))
    ratios["buffer"] = worst
    return ratios


F64_OUT = torch.float64
