"""Cases, float64 references, comparison functions and torch emulators of the BatchNorm and partial-sum kernels
(csrc/bn_act.hip, p2rnet/bn_op.py), shared by tests/test_bn_reference_cpu.py and tests/test_bn_sweep_gpu.py.

The references are plain float64 torch, one function per stage, each evaluated on the kernel's OWN fp32 stage inputs.
Next to every value comes its running-error bound in the convention of tests/embed_cases.py: u = 2^-24,
gamma(k) = k u / (1 - k u); a value that passed k rounded fp32 operations errs by at most gamma(k) times the same
expression on absolute values, and an operand that carries an error E of its own adds E times the other operand.  The
counts are read from the kernels (a contracted multiply-add rounds less often, never more):

  * bn_stats, one row of L elements, c = row[0]: v = x - c is one rounding; 256 threads take float4 steps (two additions
    inside a step, one per trip) or scalar steps, then six shuffle steps and the four waves: a term passes at most L + 10
    additions.  With S = sum (x - c), Q = sum (x - c)^2, A = sum |x - c| (float64):
      s:    E_s = gamma(L + 11) A                         (the subtraction, L + 10 additions)
      q:    E_q = gamma(L + 13) Q                         (v twice, the product, L + 10 additions)
      d = s / n (n = L exact):  E_d = E_s / L + gamma(1) (|S| + E_s) / L
      mean = c + d:             E = E_d + gamma(1) (|c + S / L| + E_d)
      s d against S^2 / L (a division, a product):  E_sd = (E_s (2 |S| + E_s) + gamma(2) (|S| + E_s)^2) / L
      M2 = max(q - s d, 0):     E = E_q + E_sd + gamma(1) (M2 + E_q + E_sd);  max(., 0) moves towards the true M2 >= 0.
    A constant row has A = Q = 0: every bound but the mean's is 0, M2 must be exactly 0.  The count is exact.
  * bn_apply: t = fma(x, scale, shift) is one rounding: E_t = gamma(1) |t|; with a residual pre = t + res is one more:
    E = E_t + gamma(1) (|pre| + E_t).  relu is 1-Lipschitz.  Where |pre| > E the sign of the device's value is the sign of
    pre, so the gate (y > 0, and the mask byte) must be the float64 gate; inside the band either gate is a correct
    rounding and the value is compared under the gate the device took.
  * bn_bwd_reduce, one row: g = dy or 0 (exact); xhat = (x - mean) invstd is two roundings, g xhat a third:
      sum g:       E = gamma(L + 10) sum |g|
      sum g xhat:  E = gamma(L + 13) sum |g| |xhat|
  * bn_bwd_apply: dx = k ((g - m1) - xhat m2): g and m1 pass two subtractions and the product with k; xhat m2 passes the
    two roundings of xhat, its product, the subtraction and the product with k:
      E = gamma(3) (|k g| + |k m1|) + gamma(5) |k xhat m2|;   dres = g is exact.
  * bn_finalize: the entries are merged in fp64 (2^-53 per operation over at most 600 entries: 2^-20 of u, ignored) and
    rounded: mean, invstd: gamma(1); scale = gamma_c invstd_f: gamma(2); shift = beta - mean_f scale: beta passes the
    subtraction, the product mean_f scale the roundings of mean_f (1) and scale (2), the product and the subtraction:
      E_shift = gamma(1) |beta| + gamma(5) |mean scale|.
    running' = running (1 - m) + m new, in fp32 with m = (float) momentum: (1 - m) carries the conversion of m and its
    own rounding, E_c = |running| gamma(1) (|m| + |1 - m|); then a product and the addition; `new` (mean_f, or the unbiased
    variance rounded from fp64) passes its own rounding, the conversion of m, the product and the addition:
      E = E_c + gamma(2) (|running (1 - m)| + E_c) + gamma(4) |m new|.
  * bn_bwd_finalize: fp64 sums rounded once, fp64 quotients rounded once: gamma(1) |value|.
  * colsum, f = 256 / V whole frames per sweep: a thread adds ceil(T / f) elements, then min(f, T) of the f staged values
    are not an exact zero: a term passes at most ceil(T / f) + min(f, T) additions.
  * sum_leading: rows are added one after the other into one or two accumulators per output (P < 32), or into 16 strided
    partial sums that are then added in order (P >= 32): a term passes at most P additions: E = gamma(P) sum_p |in|.

Every reduction keeps L <= 2051 per row and N L <= 2051 per channel: (N L)^2 u <= 1/4, so one lost or doubled element
moves a sum by more than its bound.  The element-wise kernels have no such limit: their shapes are the smallest that
chunk (L >= 8192 with fewer than 2048 rows).

The emulators reproduce each kernel's partitioning in fp32 torch (rows, chunks, vector body and scalar tail, threads,
shuffle steps, waves) on NaN-filled outputs; `mutant=` switches in one defect of MUTANTS.  They take the element offset
of the pointers (`align`, in elements mod 4; `mask_align` in bytes) since the kernels choose their path by alignment.
"""
import functools
import math

import torch
import torch.nn.functional as F

from tests.sa_votes_cases import U, gamma, worst  # noqa: F401  (re-exported: one definition of the bound's constants)
from tests.embed_cases import BAND_CAP  # noqa: F401

NAN = float("nan")
THREADS = 256
EPS = 1e-5
MASK_POISON = 0xA5            # what an unwritten mask byte holds (tests/memguard.py)

MUTANTS = ("drop_tail", "per_unrounded", "row_div_c", "unpivoted", "skip_remainder", "tr64_plain", "stride_256",
           "amax_not_cleared", "merge_no_between", "biased_running_var")


def _c(v):
    """per-channel vector -> broadcast over (N, C, L)"""
    return v[None, :, None]


def bn_chunks(rows, L):
    """`bn_chunks` of csrc/bn_act.hip (static there, restated here): chunks per row of the two element-wise kernels"""
    chunks = 1
    while rows * chunks < 2048 and L // (chunks * 2) >= 4096:
        chunks *= 2
    return chunks


def check_bound(got, ref, label=""):
    """got: CPU fp32; ref = (value, E).  No NaN (an element never written), every element within its bound -> worst ratio"""
    assert got.dtype == torch.float32 and got.shape == ref[0].shape, f"{label}: dtype / shape {got.dtype} {tuple(got.shape)}"
    assert not torch.isnan(got).any(), f"{label}: NaN (an element never written?)"
    ratio, at = worst(got, *ref)
    assert ratio <= 1, f"{label}: error / bound {ratio:.3f} at {at}"
    return ratio


# ---- the thread structure of the reductions --------------------------------------------------------------------------------
def _strided_acc(t, width=THREADS):
    """t [R, n]: element i goes to thread i % width, each thread adds its elements in order -> [R, width]"""
    R, n = t.shape
    acc = torch.zeros(R, width, dtype=t.dtype)
    trips = -(-n // width)
    pad = F.pad(t, (0, trips * width - n)).reshape(R, trips, width)
    for k in range(trips):
        acc = acc + pad[:, k]
    return acc


def _thread_acc(t, vec, drop_tail=False):
    """per-thread sums [R, 256] of the terms t [R, L] as bn_stats_kernel / bn_bwd_reduce_kernel form them: float4 steps
    (x + y) + (z + w) when the row is 16-byte aligned, then the scalar tail"""
    R, L = t.shape
    L4 = L // 4 if vec else 0
    acc = torch.zeros(R, THREADS, dtype=t.dtype)
    if L4:
        q = t[:, :4 * L4].reshape(R, L4, 4)
        acc = _strided_acc((q[..., 0] + q[..., 1]) + (q[..., 2] + q[..., 3]))
    if 4 * L4 < L and not drop_tail:
        tail = _strided_acc(t[:, 4 * L4:])
        acc = acc + tail
    return acc


def _block_sum(v):
    """[R, 256] -> [R]: six xor-shuffle steps inside each of the four waves, then the waves in order"""
    w = v.reshape(-1, THREADS // 64, 64)
    lane = torch.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        w = w + w[..., lane ^ off]
    a = torch.zeros(w.shape[0], dtype=v.dtype)
    for i in range(THREADS // 64):
        a = a + w[:, i, 0]
    return a


def _row_vec(rows, L, align):
    """bool [rows]: the row starts on a 16-byte boundary when the pointer sits `align` elements past one"""
    return (align + torch.arange(rows) * L) % 4 == 0


def _fma(a, b, c):
    """fp32 fused multiply-add: the product is exact in float64, the sum is rounded there (2^-53) and then to fp32"""
    return (a.double() * b.double() + c.double()).float()


# ---- p2r_bn_stats ---------------------------------------------------------------------------------------------------------------
STATS_L = (1, 3, 4, 1023, 1024, 1025, 1028, 2051)
STATS_ROWS = 5                # with L % 4 != 0 the rows start at every alignment: vector and scalar path in one case
STATS_KINDS = ("plain", "big", "const")


@functools.lru_cache(maxsize=None)
def stats_case(L, kind="plain"):
    """x [5, L] fp32.  'big': |mean| / std about 1000; 'const': every row one value.  Cached: do not write into it."""
    gen = torch.Generator().manual_seed(21000 + 7 * L + STATS_KINDS.index(kind))
    std = 0.5 + torch.rand(STATS_ROWS, 1, generator=gen)
    if kind == "const":
        return (torch.tensor([0.7, -1.3, 1000.1, 0.0, -3e-3])[:, None].expand(STATS_ROWS, L)).contiguous()
    mu = 0.5 * torch.randn(STATS_ROWS, 1, generator=gen)
    if kind == "big":
        mu = 1000.0 * std * torch.tensor([1.0, -1.0, 1.0, -1.0, 1.0])[:, None]
    return (torch.randn(STATS_ROWS, L, generator=gen) * std + mu).contiguous()


def stats_ref(x):
    """x [rows, L] fp32 -> {'count': L, 'mean': (value, E), 'M2': (value, E)} per row"""
    xd = x.double()
    L = x.shape[1]
    c = xd[:, 0]
    v = xd - c[:, None]
    S, Q, A = v.sum(1), (v * v).sum(1), v.abs().sum(1)
    mean = c + S / L
    M2 = ((xd - mean[:, None]) ** 2).sum(1)
    Es, Eq = gamma(L + 11) * A, gamma(L + 13) * Q
    Ed = Es / L + gamma(1) * (S.abs() + Es) / L
    Emean = Ed + gamma(1) * (mean.abs() + Ed)
    Esd = (Es * (2 * S.abs() + Es) + gamma(2) * (S.abs() + Es) ** 2) / L
    EM2 = Eq + Esd + gamma(1) * (M2 + Eq + Esd)
    return {"count": float(L), "mean": (mean, Emean), "M2": (M2, EM2)}


def check_stats(got, ref, label=""):
    """got [rows][3] CPU fp32 -> {name: worst error / bound}"""
    assert got.dtype == torch.float32 and not torch.isnan(got).any(), f"{label}: NaN (a row never written?)"
    assert (got[:, 0] == ref["count"]).all(), f"{label}: count is not {ref['count']}"
    assert (got[:, 2] >= 0).all(), f"{label}: negative M2"
    return {"mean": check_bound(got[:, 1], ref["mean"], label + " mean"), "M2": check_bound(got[:, 2], ref["M2"], label + " M2")}


def emulate_stats(x, align=0, mutant=None):
    """mutants: 'unpivoted' (sum x^2 - (sum x)^2 / L in fp32), 'stats_tail' (the scalar tail of a vector row lost)"""
    rows, L = x.shape
    out = torch.full((rows, 3), NAN)
    rv = _row_vec(rows, L, align)
    n = float(L)
    for vec in (True, False):
        sel = rv == vec
        if not sel.any():
            continue
        xr = x[sel]
        c = xr[:, :1]
        v = xr if mutant == "unpivoted" else xr - c
        s = _block_sum(_thread_acc(v, vec, mutant == "stats_tail"))
        q = _block_sum(_thread_acc(v * v, vec, mutant == "stats_tail"))
        d = s / n
        mean = d if mutant == "unpivoted" else c[:, 0] + d
        out[sel] = torch.stack([torch.full_like(s, n), mean, (q - s * d).clamp(min=0)], 1)
    return out


# ---- the element-wise kernels and the backward reduction: one case generator ------------------------------------------------------
CHUNK_SHAPES = [(1, 3, 8191), (1, 3, 8192), (2, 3, 8197), (1, 2, 16389), (3, 5, 35)]      # (N, C, L)
CHUNK_COUNTS = [1, 2, 2, 4, 1]
REDUCE_SHAPES = [(2, 3, L) for L in STATS_L]
MODES = (0, 1, 2, 3)


@functools.lru_cache(maxsize=None)
def ew_case(N, C, L):
    """fp32 CPU inputs of bn_apply, bn_bwd_reduce and bn_bwd_apply on one (N, C, L) tensor.  The three gate sources of the
    backward (y of mode 1, mscale / mshift of mode 2, the bytes of mode 3) are independent of each other, so a kernel
    that reads the wrong one is wrong in half the elements.  Cached: do not write into them."""
    gen = torch.Generator().manual_seed(22000 + 1009 * N + 101 * C + L)
    rand = lambda *s: torch.rand(*s, generator=gen)
    randn = lambda *s: torch.randn(*s, generator=gen)
    sign = lambda *s: torch.where(rand(*s) < 0.5, -1.0, 1.0)
    return {
        "x": (randn(N, C, L) * 2 + 0.5).contiguous(), "res": randn(N, C, L), "dy": randn(N, C, L),
        "scale": (0.5 + rand(C)) * sign(C), "shift": rand(C) - 0.5,
        "y": torch.relu(randn(N, C, L)), "mask": (rand(N, C, L) < 0.5).to(torch.uint8),
        "mean": 0.5 + 0.3 * randn(C), "invstd": 0.3 + rand(C), "kscale": (0.5 + rand(C)) * sign(C),
        "m1": 0.1 * randn(C), "m2": 0.1 * randn(C), "mscale": (0.5 + rand(C)) * sign(C), "mshift": rand(C) - 0.5,
    }


def gate_of(case, mode):
    """the ReLU gate of the backward kernels in mask mode `mode`, from the very operands the kernel reads: None (mode 0),
    y > 0, fma(x, mscale, mshift) > 0 (the fp32 fused value has the sign of the exact one, which float64 holds: the
    product of two fp32 numbers is exact there), byte != 0"""
    if mode == 0:
        return None
    if mode == 1:
        return case["y"] > 0
    if mode == 2:
        return case["x"].double() * _c(case["mscale"].double()) + _c(case["mshift"].double()) > 0
    return case["mask"] != 0


def apply_ref(x, scale, shift, res=None):
    """-> (pre, E): the float64 pre-activation x scale + shift (+ res) of (N, C, L) and its bound"""
    t = x.double() * _c(scale.double()) + _c(shift.double())
    E = gamma(1) * t.abs()
    if res is None:
        return t, E
    pre = t + res.double()
    return pre, E + gamma(1) * (pre.abs() + E)


def gate_band(ref):
    """bool: the elements whose gate fp32 rounding could turn"""
    return ref[0].abs() <= ref[1]


def check_apply(y, mask, ref, relu, label=""):
    """y (N, C, L) CPU fp32, mask uint8 or None -> worst error / bound.  relu: outside the band the device's gate is the
    float64 gate; the value is pre under the DEVICE's gate (exactly 0 where it is closed); the mask byte is y > 0."""
    pre, E = ref
    assert y.dtype == torch.float32 and not torch.isnan(y).any(), f"{label}: NaN (an element never written?)"
    if not relu:
        return check_bound(y, ref, label)
    gate = y > 0
    decided = ~gate_band(ref)
    assert torch.equal(gate[decided], (pre > 0)[decided]), f"{label}: a gate outside the rounding band differs from float64"
    if mask is not None:
        assert mask.dtype == torch.uint8 and torch.equal(mask, gate.to(torch.uint8)), f"{label}: mask byte is not y > 0"
    g = gate.double()
    return check_bound(y, (pre * g, E * g), label)


def _spans(rows, L, row_vec, mutant=None):
    """(row, chunk, lo, hi, body_lo, body_hi) of every workgroup of bn_apply_kernel / bn_bwd_apply_kernel: the float4 body
    covers [body_lo, body_hi), scalar steps [lo, body_lo) -- empty in the kernel -- and [body_hi, hi).
    mutant 'per_unrounded': per = ceil(L / chunks) is not rounded up to 4 while the body still takes its chunk start for
    16-byte aligned, so its first float4 sits at the next boundary: the elements in front of it belong to no chunk."""
    chunks = bn_chunks(rows, L)
    per = -(-L // chunks)
    if mutant != "per_unrounded":
        per = (per + 3) & ~3
    for row in range(rows):
        for chunk in range(chunks):
            lo = chunk * per
            hi = min(L, lo + per)
            if mutant == "per_unrounded" and row_vec[row]:
                b0 = (lo + 3) & ~3
                yield row, chunk, b0, hi, b0, b0 + ((hi - b0) & ~3)
            elif row_vec[row] and lo % 4 == 0:
                yield row, chunk, lo, hi, lo, lo + ((hi - lo) & ~3)
            else:
                yield row, chunk, lo, hi, lo, lo


def _scatter(outs, vals, rows, L, row_vec, mutant):
    """write the per-element values into the NaN-filled outputs over what the workgroups cover"""
    chunks = bn_chunks(rows, L)
    for row, chunk, lo, hi, b0, b1 in _spans(rows, L, row_vec, mutant):
        end = b1 if (mutant == "drop_tail" and chunk == chunks - 1 and b1 > b0) else hi
        for o, v in zip(outs, vals):
            if o is not None:
                o.view(rows, L)[row, lo:end] = v.reshape(rows, L)[row, lo:end]


def _channels(N, C, mutant):
    row = torch.arange(N * C)
    return (row // C if mutant == "row_div_c" else row % C).reshape(N, C)


def _bits_of_max(t):
    t = t[~torch.isnan(t)]
    return int(t.abs().max().view(torch.int32)) if t.numel() else 0


def emulate_apply(case, with_res, relu, with_mask=True, align=0, mask_align=0, amax_prefill=None, mutant=None):
    """-> (y, mask or None, amax word or None).  The vector path needs x, y, res at a 16-byte boundary and, with a mask,
    base % 4 == 0 and the mask pointer 4-byte aligned.  amax_prefill: what the word held before the call (the entry point
    clears it; mutant 'amax_not_cleared' does not)."""
    x = case["x"]
    N, C, L = x.shape
    ch = _channels(N, C, mutant)
    v = _fma(x, case["scale"][ch][..., None], case["shift"][ch][..., None])
    if with_res:
        v = v + case["res"]
    if relu:
        v = torch.relu(v)
    y = torch.full((N, C, L), NAN)
    mask = torch.full((N, C, L), MASK_POISON, dtype=torch.uint8) if (relu and with_mask) else None
    rv = _row_vec(N * C, L, align)
    if mask is not None:
        rv = rv & ((torch.arange(N * C) * L) % 4 == 0) & (mask_align % 4 == 0)
    _scatter([y, mask], [v, (v > 0).to(torch.uint8)], N * C, L, rv.tolist(), mutant)
    word = None
    if amax_prefill is not None:
        word = max(_bits_of_max(y), amax_prefill if mutant == "amax_not_cleared" else 0)
    return y, mask, word


def check_amax(word, out, label=""):
    """the word is the bit pattern of max |out| of what the kernel wrote (0 for an empty tensor)"""
    want = _bits_of_max(out)
    assert int(word) == want, f"{label}: amax word {int(word):#x}, max |out| has the bits {want:#x}"


# ---- p2r_bn_bwd_reduce ------------------------------------------------------------------------------------------------------------
def bwd_reduce_ref(case, mode):
    """-> (value, E) [N*C][2] = (sum g, sum g xhat) per row"""
    x = case["x"].double()
    N, C, L = x.shape
    g = case["dy"].double()
    gate = gate_of(case, mode)
    if gate is not None:
        g = g * gate
    xhat = (x - _c(case["mean"].double())) * _c(case["invstd"].double())
    value = torch.stack([g.sum(2), (g * xhat).sum(2)], -1).reshape(N * C, 2)
    E = torch.stack([gamma(L + 10) * g.abs().sum(2), gamma(L + 13) * (g * xhat).abs().sum(2)], -1).reshape(N * C, 2)
    return value, E


def _gated(case, mode):
    g = case["dy"]
    gate = gate_of(case, mode)
    return g if gate is None else torch.where(gate, g, torch.zeros(()))


def emulate_bwd_reduce(case, mode, align=0, mask_align=0, mutant=None):
    """mutants: 'row_div_c', 'reduce_tail' (the scalar tail of a vector row lost)"""
    x = case["x"]
    N, C, L = x.shape
    ch = _channels(N, C, mutant)
    g = _gated(case, mode).reshape(N * C, L)
    xh = ((x - case["mean"][ch][..., None]) * case["invstd"][ch][..., None]).reshape(N * C, L)
    rv = _row_vec(N * C, L, align)
    if mode == 3:
        rv = rv & ((torch.arange(N * C) * L) % 4 == 0) & (mask_align % 4 == 0)
    out = torch.full((N * C, 2), NAN)
    for vec in (True, False):
        sel = rv == vec
        if sel.any():
            drop = mutant == "reduce_tail"
            out[sel] = torch.stack([_block_sum(_thread_acc(g[sel], vec, drop)),
                                    _block_sum(_thread_acc(g[sel] * xh[sel], vec, drop))], 1)
    return out


# ---- p2r_bn_bwd_apply -------------------------------------------------------------------------------------------------------------
def bwd_apply_ref(case, mode):
    """-> {'dx': (value, E), 'dres': g as fp32 (exact)}"""
    x = case["x"].double()
    g = case["dy"].double()
    gate = gate_of(case, mode)
    if gate is not None:
        g = g * gate
    k, a1, a2 = (_c(case[n].double()) for n in ("kscale", "m1", "m2"))
    xhat = (x - _c(case["mean"].double())) * _c(case["invstd"].double())
    dx = k * (g - a1 - xhat * a2)
    E = gamma(3) * ((k * g).abs() + (k * a1).abs()) + gamma(5) * (k * xhat * a2).abs()
    return {"dx": (dx, E), "dres": _gated(case, mode)}


def check_bwd_apply(dx, dres, ref, label=""):
    """dx, dres (or None) CPU fp32 -> worst error / bound of dx; dres must be g exactly"""
    if dres is not None:
        assert not torch.isnan(dres).any(), f"{label} dres: NaN (an element never written?)"
        assert torch.equal(dres, ref["dres"]), f"{label}: dres is not the gated gradient"
    return check_bound(dx, ref["dx"], label + " dx")


def emulate_bwd_apply(case, mode, with_dres, align=0, mask_align=0, amax_prefill=None, mutant=None):
    """-> (dx, dres or None, amax word or None)"""
    x = case["x"]
    N, C, L = x.shape
    ch = _channels(N, C, mutant)
    pc = lambda n: case[n][ch][..., None]
    g = _gated(case, mode)
    xh = (x - pc("mean")) * pc("invstd")
    v = pc("kscale") * (g - pc("m1") - xh * pc("m2"))
    dx = torch.full((N, C, L), NAN)
    dres = torch.full((N, C, L), NAN) if with_dres else None
    rv = _row_vec(N * C, L, align)
    if mode == 3:
        rv = rv & ((torch.arange(N * C) * L) % 4 == 0) & (mask_align % 4 == 0)
    _scatter([dx, dres], [v, g], N * C, L, rv.tolist(), mutant)
    word = None
    if amax_prefill is not None:
        word = max(_bits_of_max(dx), amax_prefill if mutant == "amax_not_cleared" else 0)
    return dx, dres, word


# ---- p2r_bn_finalize / p2r_bn_bwd_finalize ----------------------------------------------------------------------------------------
FIN_P = (1, 255, 256, 257, 600)
FIN_C = (1, 3, 64)
FIN_MOMENTUM = (0.1, 1.0, 0.0, -1.0)


@functools.lru_cache(maxsize=None)
def finalize_case(P, C, width, big=False):
    """partial [P][C][width] fp32 with unequal counts per entry (2 .. 40 elements), the element count M, and the module's
    gamma, beta, running_mean, running_var.  width 3: (count, mean, M2); width 2: (sum, sum of squares) of such entries.
    big: |mean| / std about 1000.  Cached: do not write into them."""
    gen = torch.Generator().manual_seed(23000 + 97 * P + 7 * C + width + (1 if big else 0))
    rand = lambda *s: torch.rand(*s, generator=gen, dtype=torch.float64)
    randn = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64)
    n = torch.randint(2, 41, (P, 1), generator=gen).double().expand(P, C)
    std = 0.5 + rand(C)
    mu = 1000.0 * std * torch.where(rand(C) < 0.5, -1.0, 1.0) if big else 0.5 * randn(C)
    mean_p = mu + std * randn(P, C) / n.sqrt()
    m2_p = n * std ** 2 * (0.5 + rand(P, C))
    if width == 3:
        part = torch.stack([n, mean_p, m2_p], -1)
    else:
        part = torch.stack([n * mean_p, m2_p + n * mean_p ** 2], -1)
    f = lambda t: t.float().contiguous()
    return {"part": f(part), "M": float(n[:, 0].sum()), "gamma": f(0.5 + rand(C)), "beta": f(rand(C) - 0.5),
            "running_mean": f(0.2 * randn(C)), "running_var": f(0.5 + 1.5 * rand(C))}


def _merge(part, M, between=True):
    """float64 (mean, M2, M) per channel of entries [P][C][width]; width 3 uses the entries' own counts"""
    part = part.double()
    if part.shape[-1] == 3:
        n = part[..., 0]
        tot = n.sum(0)
        mean = (n * part[..., 1]).sum(0) / tot
        m2 = part[..., 2] + (n * (part[..., 1] - mean) ** 2 if between else 0.0)
        return mean, m2.sum(0), tot
    s, q = part[..., 0].sum(0), part[..., 1].sum(0)
    mean = s / M
    return mean, q - mean * mean * M, torch.full_like(s, M)


def _finalize_from(mean, m2, Mc, case, momentum, eps, biased=False, bounds=True):
    """the constants and running statistics from the merged (mean, M2, M): float64 values with their bounds, or (bounds =
    False) the fp32 arithmetic of the kernel's last thread"""
    gam, bet = case["gamma"], case["beta"]
    rm, rv = case["running_mean"], case["running_var"]
    var = (m2 / Mc).clamp(min=0.0)
    invstd = (var + eps).rsqrt()
    new_var = var if biased else var * (Mc / (Mc - 1.0).clamp(min=1.0))
    if not bounds:
        mean_f, invstd_f = mean.float(), invstd.float()
        scale = gam * invstd_f
        out = {"out": torch.stack([mean_f, invstd_f, scale, bet - mean_f * scale])}
        if momentum >= 0:
            mom = torch.tensor(momentum, dtype=torch.float32)
            out["running_mean"] = rm * (1.0 - mom) + mom * mean_f
            out["running_var"] = rv * (1.0 - mom) + mom * new_var.float()
        else:
            out["running_mean"], out["running_var"] = rm.clone(), rv.clone()
        return out
    scale = gam.double() * invstd
    value = torch.stack([mean, invstd, scale, bet.double() - mean * scale])
    E = torch.stack([gamma(1) * mean.abs(), gamma(1) * invstd, gamma(2) * scale.abs(),
                     gamma(1) * bet.double().abs() + gamma(5) * (mean * scale).abs()])
    ref = {"out": (value, E)}
    for name, run, new in (("running_mean", rm.double(), mean), ("running_var", rv.double(), new_var)):
        if momentum < 0:
            ref[name] = (run, torch.zeros_like(run))
            continue
        Ec = run.abs() * gamma(1) * (abs(momentum) + abs(1 - momentum))
        keep = run * (1 - momentum)
        ref[name] = (keep + momentum * new, Ec + gamma(2) * (keep.abs() + Ec) + gamma(4) * (momentum * new).abs())
    return ref


def finalize_ref(case, momentum, eps=EPS):
    """-> {'out': (value, E) [4][C] = mean, invstd, scale, shift; 'running_mean', 'running_var': (value, E)}; a negative
    momentum leaves the running statistics as they are (bound 0)"""
    return _finalize_from(*_merge(case["part"], case["M"]), case, momentum, eps)


def check_finalize(got, ref, label=""):
    """got: 'out' [4][C], 'running_mean', 'running_var' [C] CPU fp32 -> {name: worst error / bound}"""
    return {k: check_bound(got[k], ref[k], f"{label} {k}") for k in ("out", "running_mean", "running_var")}


def _fin_block_sum(vals):
    """[P, C] float64 -> [C]: thread t adds the entries p = t, t + 256, ..., then the block sum"""
    return _block_sum(_strided_acc(vals.t().contiguous()))


def emulate_finalize(case, momentum, eps=EPS, mutant=None):
    """bn_finalize_kernel: fp64 stride loops and block sums, then thread 0's fp32 arithmetic.  mutants:
    'merge_no_between', 'biased_running_var', 'fin_first_trip' (the stride loop runs once: entries beyond 256 lost)"""
    part = case["part"].double()
    if mutant == "fin_first_trip":
        part = part[:THREADS]
    if part.shape[-1] == 3:
        n = _fin_block_sum(part[..., 0])
        mean = _fin_block_sum(part[..., 0] * part[..., 1]) / n
        d = part[..., 1] - mean
        m2 = _fin_block_sum(part[..., 2] + (0.0 if mutant == "merge_no_between" else part[..., 0] * d * d))
        Mc = n
        mean = (mean * n) / Mc
    else:
        s, q = _fin_block_sum(part[..., 0]), _fin_block_sum(part[..., 1])
        Mc = torch.full_like(s, case["M"])
        mean = s / Mc
        m2 = q - mean * mean * Mc
    return _finalize_from(mean, m2, Mc, case, momentum, eps, biased=mutant == "biased_running_var", bounds=False)


@functools.lru_cache(maxsize=None)
def bwd_finalize_case(P, C):
    gen = torch.Generator().manual_seed(24000 + 97 * P + C)
    return (torch.randn(P, C, 2, generator=gen) * 3.0).contiguous(), float(37 * P + 5)


def bwd_finalize_ref(part, M):
    """-> (value, E) [4][C] = sum g, sum g xhat, (sum g) / M, (sum g xhat) / M"""
    S = part.double().sum(0)
    value = torch.stack([S[:, 0], S[:, 1], S[:, 0] / M, S[:, 1] / M])
    return value, gamma(1) * value.abs()


def emulate_bwd_finalize(part, M, mutant=None):
    p = part.double()[:THREADS] if mutant == "fin_first_trip" else part.double()
    s, q = _fin_block_sum(p[..., 0]), _fin_block_sum(p[..., 1])
    return torch.stack([s.float(), q.float(), (s / M).float(), (q / M).float()])


# ---- p2r_colsum -------------------------------------------------------------------------------------------------------------------
COLSUM_V = (1, 53, 128, 129, 255, 256)      # lanes_used = (256 / V) V: 256, 212, 256, 129, 255, 256
COLSUM_T = (1, 5, 39)
COLSUM_ROWS = 3


@functools.lru_cache(maxsize=None)
def colsum_case(T, V):
    gen = torch.Generator().manual_seed(25000 + 300 * T + V)
    return torch.randn(COLSUM_ROWS, T, V, generator=gen).contiguous()


def colsum_ref(x):
    """x [rows][T][V] -> (value, E) [rows][V]"""
    _, T, V = x.shape
    f = THREADS // V
    k = -(-T // f) + min(f, T)
    return x.double().sum(1), gamma(k) * x.double().abs().sum(1)


def emulate_colsum(x, mutant=None):
    """mutant 'stride_256': the threads stride by the workgroup size, not by lanes_used, and so change their joint"""
    rows, T, V = x.shape
    lanes = (THREADS // V) * V
    stride = THREADS if mutant == "stride_256" else lanes
    n = T * V
    trips = -(-n // stride)
    pad = F.pad(x.reshape(rows, n), (0, trips * stride - n)).reshape(rows, trips, stride)[:, :, :lanes]
    acc = torch.zeros(rows, lanes)
    for k in range(trips):
        acc = acc + pad[:, k]
    staged = acc.reshape(rows, lanes // V, V)
    out = torch.zeros(rows, V)
    for j in range(lanes // V):
        out = out + staged[:, j]
    return out


# ---- p2r_sum_leading --------------------------------------------------------------------------------------------------------------
SUM_P = (1, 7, 8, 9, 31, 32, 33, 127, 128, 129, 256, 300)     # the row kernel from 32 on; 8 and 8 x 16 rows per unrolled trip
SUM_M = (4, 60, 64, 68, 1028)                                 # the row kernel's workgroup owns 64 outputs, the other 1024
SUM_M_TR64 = (4096, 8192)


@functools.lru_cache(maxsize=4)
def sum_case(P, M):
    gen = torch.Generator().manual_seed(26000 + 10007 * P + M)
    return torch.randn(P, M, generator=gen)


def _tr64(t):
    return t.reshape(-1, 64, 64).transpose(1, 2).reshape(-1)


def sum_leading_ref(inp, tr64=False):
    """inp [P][M] -> (value, E) [M]; tr64: out[blk][b][a] = sum_p in[p][blk][a][b]"""
    value, E = inp.double().sum(0), gamma(inp.shape[0]) * inp.double().abs().sum(0)
    return (_tr64(value), _tr64(E)) if tr64 else (value, E)


def emulate_sum_leading(inp, tr64=False, mutant=None):
    """sum_leading_kernel (P < 32) and sum_leading_rows_kernel.  mutants: 'skip_remainder' (the rows after the unrolled loop
    lost), 'tr64_plain' (the blocks not transposed)"""
    P, M = inp.shape
    if P >= 32:
        acc = torch.zeros(16, M)
        for ty in range(16):
            p = ty
            while p + 7 * 16 < P:
                for u in range(8):
                    acc[ty] = acc[ty] + inp[p + 16 * u]
                p += 8 * 16
            while p < P and mutant != "skip_remainder":
                acc[ty] = acc[ty] + inp[p]
                p += 16
        out = acc[0]
        for r in range(1, 16):
            out = out + acc[r]
    else:
        acc, acc2 = torch.zeros(M), torch.zeros(M)
        p = 0
        while p + 8 <= P:
            for u in range(0, 8, 2):
                acc, acc2 = acc + inp[p + u], acc2 + inp[p + u + 1]
            p += 8
        while p < P and mutant != "skip_remainder":
            acc = acc + inp[p]
            p += 1
        out = acc + acc2
    return _tr64(out) if (tr64 and mutant != "tr64_plain") else out


# ---- the op: BatchNorm (+ residual) (+ ReLU) under float64 autograd -------------------------------------------------------------
OP_SHAPES = [(3, 8, 7, 5), (2, 64, 16, 53), (1, 4, 155, 53), (2, 6, 35)]
Y_TOL = (1e-5, 1e-5)          # (rtol, atol): the project's tolerances of tests/test_bn_gpu.py, here against float64
STAT_TOL = (1e-5, 1e-6)
DX_TOL = (1e-4, 1e-5)
PARAM_TOL = 1e-4              # of max |ref|


@functools.lru_cache(maxsize=None)
def op_case(shape):
    """x, res, go of `shape` and the module's gamma, beta, running_mean, running_var away from their defaults"""
    gen = torch.Generator().manual_seed(27000 + sum((i + 1) * s for i, s in enumerate(shape)))
    C = shape[1]
    rand = lambda *s: torch.rand(*s, generator=gen)
    return {"x": torch.randn(shape, generator=gen) * 2 + 0.5, "res": torch.randn(shape, generator=gen),
            "go": torch.randn(shape, generator=gen), "gamma": 0.5 + rand(C), "beta": rand(C) - 0.5,
            "running_mean": 0.4 * rand(C) - 0.2, "running_var": 0.5 + 1.5 * rand(C)}


def op_ref(case, with_res, relu, train, gate=None, momentum=0.1, eps=EPS):
    """relu?(bn(x) + res) in float64 under autograd.  The ReLU is pre * gate with gate = (pre > 0) when `gate` is None, else
    the given boolean tensor as a constant.  -> dict: 'pre', 'y', 'dx', 'dres' (or None), 'dgamma', 'dbeta', 'running_mean',
    'running_var' (updated in training mode)"""
    x = case["x"].double().requires_grad_(True)
    gam, bet = (case[k].double().requires_grad_(True) for k in ("gamma", "beta"))
    res = case["res"].double().requires_grad_(True) if with_res else None
    rm, rv = case["running_mean"].double(), case["running_var"].double()
    dims = [d for d in range(x.dim()) if d != 1]
    bc = lambda v: v.view(1, -1, *([1] * (x.dim() - 2)))
    if train:
        n = x.numel() // x.shape[1]
        mean, var = x.mean(dims), x.var(dims, unbiased=False)
        rm = ((1 - momentum) * rm + momentum * mean).detach()
        rv = ((1 - momentum) * rv + momentum * var * (n / max(n - 1, 1))).detach()
    else:
        mean, var = rm, rv
    pre = (x - bc(mean)) * bc((var + eps).rsqrt() * gam) + bc(bet)
    if res is not None:
        pre = pre + res
    y = pre
    if relu:
        y = pre * ((pre > 0) if gate is None else gate).detach().double()
    y.backward(case["go"].double())
    return {"pre": pre.detach(), "y": y.detach(), "dx": x.grad, "dres": res.grad if res is not None else None,
            "dgamma": gam.grad, "dbeta": bet.grad, "running_mean": rm, "running_var": rv}


def close_ratio(got, want, rtol, atol):
    """largest |got - want| / (atol + rtol |want|): at most 1 is what torch.testing.assert_close(rtol, atol) accepts"""
    want = want.double()
    return float(((got.detach().double() - want).abs() / (atol + rtol * want.abs())).max())


def rel_ratio(got, want, tol):
    """max |got - want| / (tol max |want|)"""
    want = want.double()
    return float((got.detach().double() - want).abs().max() / (tol * want.abs().max() + 1e-300))


def width2_partials(x):
    """(sum, sum of squares) per (sample, channel) of x (N, C, ...) -> [N][C][2] fp32, from float64 sums"""
    xd = x.double().flatten(2)
    return torch.stack([xd.sum(2), (xd * xd).sum(2)], -1).float()


assert math.isclose(gamma(1), U / (1 - U))
