"""Cases, float64 references and comparison functions of the embedding MLPs (csrc/embed.hip, csrc/embed_bwd.hip, the
single-tap temporal-conv kernels, p2rnet/embed_op.py), shared by tests/test_embed_reference_cpu.py and
tests/test_embed_sweep_gpu.py.

The references are plain float64 torch, one function per stage, each evaluated on the kernel's OWN fp32 stage inputs, so
the error of a stage is not mixed with the error of the stage before.  Next to every value comes its running-error bound
with u = 2^-24 and gamma(k) = k u / (1 - k u): a value that passed k rounded fp32 operations errs by at most gamma(k)
times the same expression on absolute values; an operand that carries an error E of its own adds E times the other
operand.  The bounds are derived from the kernels' operation counts, not measured, and hold for every summation order
with one round-to-nearest per operation (a fused multiply-add rounds less often, never more):

  * dz = a g + b z + c (the BatchNorm-backward form, formed while a tile is staged): two rounded products, two additions;
    the product a g passes three roundings: E_dz = gamma(3) (|a g| + |b z| + |c|).  dz = g (coef == NULL) is exact.
  * A = relu(zp scale + shift): a rounded product and an addition, relu is 1-Lipschitz: E_A = gamma(2) (|zp scale| + |shift|)
    where the gate is open, 0 where it is closed (the cases hold no element whose gate fp32 rounding could turn).
  * g_prev = (W^T dz) gated: a rounded product, then 64 additions into an accumulator that starts at zero:
    E_g = |W|^T E_dz + gamma(65) |W|^T (|dz| + E_dz); exactly 0 where the gate is closed.
    For E_dz = gamma(3) |dz|_abs this is below gamma(68) |W|^T |dz|_abs: three roundings, a product, 64 additions.
  * sums over the N L columns, left as P partial rows that are then added: a term passes at most N L + P additions.
      S1 = sum g_prev:                E = sum E_g + gamma(N L + P) sum (|g_prev| + E_g)
      S2 = sum g_prev xhat, xhat = (zp - mean) invstd (a subtraction and two products, each relative to its own result):
                                      E = sum E_g |xhat| + gamma(N L + P + 3) sum (|g_prev| + E_g) |xhat|
      dW = dz A^T (a rounded product): E = E_dz |A|^T + (|dz| + E_dz) E_A^T + gamma(N L + P + 1) (|dz| + E_dz) (|A| + E_A)^T
      db = row sums of dz:            E = sum E_dz + gamma(N L + P) sum (|dz| + E_dz)
  * BatchNorm-backward constants (pw_bn_bwd_finalize_kernel): the partials are added in fp64 (exact next to u), then
    dbeta = fl(S1), dgamma = fl(S2): gamma(1); m = fl(S / M): one rounding; a = scale: exact;
    b = -scale invstd m2: m2's rounding and two products: gamma(3) |b|;
    c = -scale m1 + scale invstd m2 mean: gamma(3) |scale m1| + gamma(5) |scale invstd m2 mean|.
  * the 3 -> 64 layer: out = b + ((w0 x0 + w1 x1) + w2 x2): a product and three additions: gamma(4) (|W| |x| + |b|).
  * its weight gradient, one row of L columns per workgroup: 256 threads take float4 steps (two additions inside a step,
    one per trip) or scalar steps, then six shuffle steps and the four waves: a term passes at most L + 10 additions,
    after the product with x (the dout column has none) and the three roundings of the lazy dz:
      E = sum E_dz |x| + gamma(L + 11) sum (|dz| + E_dz) |x|,   dout column: sum E_dz + gamma(L + 10) sum (|dz| + E_dz).

Every stage-level case keeps N L <= 2048 columns (L <= 2048 per row of the 3 -> 64 weight gradient): (N L)^2 u <= 1/4, so
one lost or doubled column moves a sum by more than its bound.  The float64 evaluation itself errs by 2^-53 per
operation, 2^-29 of the bound: ignored.
"""
import copy
import functools

import torch

from tests.sa_votes_cases import U, gamma, worst  # noqa: F401  (re-exported: one definition of the bound's constants)

C = 64
COLS = 64                 # columns per tile of embed_bwd_kernel
FWD_TOL = 5e-5            # the project's forward tolerance of this MLP against fp64 ("out vs fp64")
STAT_TOL = 2e-5           # running statistics against fp64
GRAD_TOL = 1e-4           # parameter gradients against fp64 (test_bn_relu_pointwise)


def _c(v):
    """per-channel vector -> broadcast over (N, 64, L)"""
    return v[None, :, None]


# ---- p2r_embed_layer_backward ---------------------------------------------------------------------------------------------
LAYER_SHAPES = [(1, 64), (5, 64), (2, 192), (3, 128), (1, 2048), (2, 1024)]     # (5, 64): every tile is another sample
BIG_MEAN_SHAPE = (5, 64)                                                         # |mean| / std about 100


def n_blocks_of(N, L):
    """the workgroup counts of the sweep: one workgroup walking all tiles, unequal tile counts, exactly one tile each,
    the clamp with zeroed rows"""
    tiles = N * L // COLS
    return sorted({n for n in (1, 2, 3, tiles - 1, tiles, tiles + 1, 512) if n >= 1})


@functools.lru_cache(maxsize=None)
def layer_case(N, L, big_mean=False):
    """fp32 CPU tensors g, z, zp (N,64,L), coef [3][64], fin [4][64], W [64][64].  Cached: do not write into them.
    fin is the BatchNorm of zp's own statistics with gamma in [0.5, 1.5], beta in [-0.5, 0.5]; g is a masked gradient
    (about half zeros).  An element whose gate lies within twice the rounding band (`gate_band`) is moved out of it."""
    gen = torch.Generator().manual_seed(11000 + 131 * N + L + (7 if big_mean else 0))
    rand = lambda *s: torch.rand(*s, generator=gen)
    randn = lambda *s: torch.randn(*s, generator=gen)
    std = 0.5 + rand(C)
    mu = (100.0 * std * torch.where(rand(C) < 0.5, -1.0, 1.0)) if big_mean else 0.5 * randn(C)
    zp = (randn(N, C, L) * _c(std) + _c(mu)).contiguous()
    gam, bet = 0.5 + rand(C), rand(C) - 0.5
    z = randn(N, C, L)
    g = (randn(N, C, L) * (rand(N, C, L) < 0.5)).contiguous()
    coef = torch.stack([0.5 + rand(C), 0.1 * randn(C), 0.1 * randn(C)]).contiguous()
    W = ((rand(C, C) * 2 - 1) * (2.4 / C ** 0.5)).contiguous()
    for _ in range(4):
        mean = zp.double().mean((0, 2))
        invstd = (zp.double().var((0, 2), unbiased=False) + 1e-5).rsqrt().float()
        mean = mean.float()
        scale = gam * invstd
        fin = torch.stack([mean, invstd, scale, bet - mean * scale]).contiguous()
        near = gate_band(zp, fin, width=8)
        if not near.any():
            break
        zp = torch.where(near, zp + 1e-3 * _c(std), zp).contiguous()
    return {"g": g, "z": z, "coef": coef, "zp": zp, "fin": fin, "W": W}


def gate_band(zp, fin, width=4):
    """bool (N,64,L): the elements whose gate zp scale + shift > 0 fp32 rounding could turn -- a product rounded before
    the addition against a fused multiply-add: |scale zp + shift| <= width u (|scale zp| + |shift|)"""
    zp, s, t = zp.double(), _c(fin[2].double()), _c(fin[3].double())
    return (zp * s + t).abs() <= width * U * ((zp * s).abs() + t.abs())


def layer_backward_ref(g, z, coef, zp, fin, W):
    """float64 reference of one p2r_embed_layer_backward call on its fp32 inputs (coef None: dz = g, z unused).
    -> dict: 'gate' (N,64,L) bool; 'g_prev' = (value, E); 'S1', 'S2', 'dW', 'db' = (value, fixed, mag, k): the bound of a
    sum left in P partial rows over N L columns is fixed + gamma(N L + P + k) mag (`summed_bound`)."""
    g, zp, W = g.double(), zp.double(), W.double()
    mean, invstd, scale, shift = (_c(fin[i].double()) for i in range(4))
    if coef is None:
        dz, Edz = g, torch.zeros_like(g)
    else:
        a, b, c = (_c(coef[i].double()) for i in range(3))
        z = z.double()
        dz = a * g + b * z + c
        Edz = gamma(3) * ((a * g).abs() + (b * z).abs() + c.abs())
    y = zp * scale + shift
    gate = y > 0
    A = y * gate
    EA = gamma(2) * ((zp * scale).abs() + shift.abs()) * gate
    dza = dz.abs() + Edz
    lin = lambda w, v: torch.einsum("oi,nol->nil", w, v)
    g_prev = lin(W, dz) * gate
    Eg = (lin(W.abs(), Edz) + gamma(65) * lin(W.abs(), dza)) * gate
    ga = g_prev.abs() + Eg
    xhat = ((zp - mean) * invstd).abs()
    outer = lambda p, q: torch.einsum("nol,nil->oi", p, q)
    return {
        "gate": gate, "dz": (dz, Edz), "g_prev": (g_prev, Eg),
        "S1": (g_prev.sum((0, 2)), Eg.sum((0, 2)), ga.sum((0, 2)), 0),
        "S2": ((g_prev * (zp - mean) * invstd).sum((0, 2)), (Eg * xhat).sum((0, 2)), (ga * xhat).sum((0, 2)), 3),
        "dW": (outer(dz, A), outer(Edz, A.abs()) + outer(dza, EA), outer(dza, A.abs() + EA), 1),
        "db": (dz.sum((0, 2)), Edz.sum((0, 2)), dza.sum((0, 2)), 0),
    }


def summed_bound(entry, cols, parts):
    _, fixed, mag, k = entry
    return fixed + gamma(cols + parts + k) * mag


def check_layer_backward(got, ref, label=""):
    """got: the buffers of one call as CPU fp32 tensors -- 'g_prev' (N,64,L), 'sums' [P][64][2], 'dw_part' [P][64][64],
    'db_part' [P][64] or None.  Asserts: no NaN anywhere; the partial rows at and beyond min(P, tiles) exactly zero;
    g_prev elementwise within its bound, exactly 0 where the gate is closed; the sums over the partial rows of S1, S2, dW
    and db within theirs.  -> {name: worst error / bound}"""
    gp = got["g_prev"]
    N, _, L = gp.shape
    cols, P = N * L, got["sums"].shape[0]
    live = min(P, cols // COLS)
    parts = {"sums": got["sums"], "dw_part": got["dw_part"]}
    if got.get("db_part") is not None:
        parts["db_part"] = got["db_part"]
    for k, t in list(parts.items()) + [("g_prev", gp)]:
        assert t.dtype == torch.float32 and not torch.isnan(t).any(), f"{label} {k}: NaN (an element never written?)"
    for k, t in parts.items():
        assert t.shape[0] == P and not t[live:].any(), f"{label} {k}: a partial row beyond the {live} workgroups is not zero"
    value, E = ref["g_prev"]
    assert not gp[~ref["gate"]].any(), f"{label} g_prev: not 0 where the gate is closed"
    ratios = {"g_prev": worst(gp, value, E)}
    summed = {"S1": parts["sums"][..., 0], "S2": parts["sums"][..., 1], "dW": parts["dw_part"]}
    if "db_part" in parts:
        summed["db"] = parts["db_part"]
    for k, t in summed.items():
        ratios[k] = worst(t.double().sum(0), ref[k][0], summed_bound(ref[k], cols, live))
    for k, (ratio, at) in ratios.items():
        assert ratio <= 1, f"{label} {k}: error / bound {ratio:.3f} at {at}"
    return {k: r for k, (r, _) in ratios.items()}


def emulate_layer_backward(case, n_blocks, lazy=True, with_db=True, mutant=None):
    """fp32 torch emulation of embed_bwd_kernel's work split: tiles of 64 columns dealt to n_blocks workgroups (tile t to
    workgroup t mod n_blocks), per-workgroup partials in rows -> the `got` of check_layer_backward.  mutant: one of MUTANTS,
    a defect of the kind the persistent loop could have."""
    g, z, zp, fin, W = case["g"], case["z"], case["zp"], case["fin"], case["W"]
    coef = case["coef"] if lazy else None
    N, _, L = g.shape
    tiles = N * L // COLS
    blocks = min(n_blocks, tiles)
    mean, invstd, scale, shift = (fin[i][:, None] for i in range(4))
    gp = torch.full((N, C, L), float("nan"))
    sums, dwp, dbp = torch.zeros(n_blocks, C, 2), torch.zeros(n_blocks, C, C), torch.zeros(n_blocks, C)

    def tile_of(x, t):
        n, c0 = divmod(t * COLS, L)
        return x[n, :, c0:c0 + COLS]

    for b in range(blocks):
        mine = list(range(b, tiles, n_blocks))
        for i, t in enumerate(mine):
            n, c0 = divmod(t * COLS, L)
            dz = tile_of(g, t)
            if lazy:
                dz = coef[0][:, None] * dz + coef[1][:, None] * tile_of(z, t) + coef[2][:, None]
            zt = tile_of(zp, t)
            A = torch.relu(zt * scale + shift)
            zm = zt
            if mutant == "stale_zp" and i > 0:
                zm = tile_of(zp, mine[i - 1])
            if mutant == "gate_z":
                zm = tile_of(z, t)
            v = (W.t() @ dz) * (zm * scale + shift > 0)
            gp[n, :, c0:c0 + COLS] = v
            if mutant == "drop_last_tile" and b == 0 and i == len(mine) - 1:
                continue
            xhat = zt if mutant == "s2_raw" else (zt - mean) * invstd
            sums[b, :, 0] += v.sum(1)
            sums[b, :, 1] += (v * xhat).sum(1)
            dwp[b] += dz @ A.t()
            dbp[b] += (dz[:, 16:] if mutant == "db_quarter" and t == 0 else dz).sum(1)
    if mutant == "skip_partial":
        for t in (sums, dwp, dbp):
            t[blocks - 1] = 0
    return {"g_prev": gp, "sums": sums, "dw_part": dwp, "db_part": dbp if with_db else None}


MUTANTS = ("drop_last_tile", "stale_zp", "skip_partial", "gate_z", "s2_raw", "db_quarter")


# ---- p2r_pw_bn_bwd_finalize ------------------------------------------------------------------------------------------------
def bn_bwd_coef_ref(S1, S2, fin, M, train):
    """S1, S2 [64] float64 (the partial rows added in float64), fin [4][64] fp32 -> 'coef' [3][64], 'dgamma', 'dbeta' as
    (value, E), as pw_bn_bwd_finalize_kernel defines them; evaluation mode: coef = (scale, 0, 0)"""
    mean, invstd, scale, _ = (fin[i].double() for i in range(4))
    zero = torch.zeros_like(scale)
    if train:
        m1, m2 = S1 / M, S2 / M
        b = -scale * invstd * m2
        c1, c2 = -scale * m1, scale * invstd * m2 * mean
        coef = torch.stack([scale, b, c1 + c2])
        E = torch.stack([zero, gamma(3) * b.abs(), gamma(3) * c1.abs() + gamma(5) * c2.abs()])
    else:
        coef, E = torch.stack([scale, zero, zero]), torch.zeros(3, scale.numel(), dtype=torch.float64)
    return {"coef": (coef, E), "dgamma": (S2, gamma(1) * S2.abs()), "dbeta": (S1, gamma(1) * S1.abs())}


def check_bn_bwd_coef(got, ref, label=""):
    """got: 'coef' [3][64], 'dgamma', 'dbeta' [64] CPU fp32 -> {name: worst error / bound}"""
    ratios = {}
    for k in ("coef", "dgamma", "dbeta"):
        assert not torch.isnan(got[k]).any(), f"{label} {k}: NaN"
        ratio, at = worst(got[k], *ref[k])
        assert ratio <= 1, f"{label} {k}: error / bound {ratio:.3f} at {at}"
        ratios[k] = ratio
    return ratios


@functools.lru_cache(maxsize=None)
def finalize_case(P):
    """partials [P][64][2] of an embedding-shaped job, its fin [4][64] and the element count M"""
    gen = torch.Generator().manual_seed(12000 + P)
    part = torch.randn(P, C, 2, generator=gen) * 3.0
    mean, invstd = torch.randn(C, generator=gen), 0.5 + torch.rand(C, generator=gen)
    scale = (0.5 + torch.rand(C, generator=gen)) * invstd
    fin = torch.stack([mean, invstd, scale, torch.rand(C, generator=gen) - 0.5 - mean * scale]).contiguous()
    return part, fin, 64 * max(P, 4)


# ---- the 3 -> 64 layer: weight gradient and statistics -----------------------------------------------------------------------
WGRAD_N = (1, 3)
WGRAD_L = (7, 64, 1028, 1030, 2048)     # scalar tail only; the vector path; a second trip of the stride loop; L % 4 != 0


@functools.lru_cache(maxsize=None)
def wgrad_case(N, L):
    gen = torch.Generator().manual_seed(13000 + 17 * N + L)
    x = torch.randn(N, 3, L, generator=gen) * torch.tensor([1.0, 0.4, 2.0])[None, :, None]
    g = torch.randn(N, C, L, generator=gen) * (torch.rand(N, C, L, generator=gen) < 0.5)
    z = torch.randn(N, C, L, generator=gen)
    coef = torch.stack([0.5 + torch.rand(C, generator=gen), 0.1 * torch.randn(C, generator=gen),
                        0.1 * torch.randn(C, generator=gen)])
    return {"x": x.contiguous(), "g": g.contiguous(), "z": z, "coef": coef.contiguous()}


def embed3_wgrad_ref(x, g, z=None, coef=None):
    """-> (value, E) [N*64][4]: the sums over L of dout x0, dout x1, dout x2, dout with dout = coef[0] g + coef[1] z + coef[2]
    (coef None: dout = g)"""
    x, g = x.double(), g.double()
    N, _, L = g.shape
    if coef is None:
        dz, Edz = g, torch.zeros_like(g)
    else:
        a, b, c = (_c(coef[i].double()) for i in range(3))
        dz = a * g + b * z.double() + c
        Edz = gamma(3) * ((a * g).abs() + (b * z.double()).abs() + c.abs())
    dza = dz.abs() + Edz
    row = lambda p, q: torch.einsum("ncl,ndl->ncd", p, q)
    value = torch.cat([row(dz, x), dz.sum(2, keepdim=True)], 2)
    E = torch.cat([row(Edz, x.abs()) + gamma(L + 11) * row(dza, x.abs()),
                   Edz.sum(2, keepdim=True) + gamma(L + 10) * dza.sum(2, keepdim=True)], 2)
    return value.reshape(N * C, 4), E.reshape(N * C, 4)


def check_embed3_wgrad(got, ref, label=""):
    """got [N*64][4] CPU fp32 -> worst error / bound"""
    assert got.dtype == torch.float32 and not torch.isnan(got).any(), f"{label}: NaN (a row never written?)"
    ratio, at = worst(got, *ref)
    assert ratio <= 1, f"{label}: error / bound {ratio:.3f} at {at}"
    return ratio


def emulate_embed3_wgrad(case, lazy=True, mutant=None):
    """fp32 torch emulation of embed3_wgrad_kernel: the float4 body when L % 4 == 0, scalar steps otherwise.
    mutant 'drop_tail': the float4 body over L // 4 steps whatever L, the remaining columns lost; 'drop_c': coef[2] lost"""
    x, g = case["x"], case["g"]
    N, _, L = g.shape
    dz = g
    if lazy:
        a, b, c = (_c(case["coef"][i]) for i in range(3))
        dz = a * g + b * case["z"] if mutant == "drop_c" else a * g + b * case["z"] + c
    n = (L // 4) * 4 if mutant == "drop_tail" else L
    out = torch.cat([torch.einsum("ncl,ndl->ncd", dz[..., :n], x[..., :n]), dz[..., :n].sum(2, keepdim=True)], 2)
    return out.reshape(N * C, 4)


STATS_L = (1, 1023, 1024, 1025, 2049)   # one workgroup holds 1024 points: at 1025 and 2049 the last one holds one


@functools.lru_cache(maxsize=None)
def stats_case(B, L, offset, constant=False):
    gen = torch.Generator().manual_seed(14000 + 7 * B + L + int(offset))
    x = torch.randn(B, 3, L, generator=gen) * torch.tensor([1.0, 0.3, 2.0])[None, :, None] + offset
    if constant:
        x = torch.tensor([0.7, -1.3, offset + 2.1])[None, :, None].expand(B, 3, L)
    W = (torch.rand(C, 3, generator=gen) * 2 - 1) * 3 ** -0.5
    b = (torch.rand(C, generator=gen) * 2 - 1) * 3 ** -0.5
    return x.contiguous(), W.contiguous(), b


def embed3_stats_ref(x, W, b):
    """-> (out, E) (N,64,L) float64 with E = gamma(4) (|W| |x| + |b|), and the per-channel mean and biased variance of
    the float64 output"""
    x, W, b = x.double(), W.double(), b.double()
    out = torch.einsum("cd,ndl->ncl", W, x) + _c(b)
    E = gamma(4) * (torch.einsum("cd,ndl->ncl", W.abs(), x.abs()) + _c(b.abs()))
    return (out, E), out.mean((0, 2)), out.var((0, 2), unbiased=False)


# ---- the whole MLP ---------------------------------------------------------------------------------------------------------
MLP_CASES = [(1, 16, 20, False), (2, 16, 20, True), (2, 64, 53, True), (3, 1, 64, False), (5, 1, 64, True),
             (2, 16, 4, False)]      # (B, rows, inner, add)
PARAMS = ("0.conv.weight", "0.batchnorm.weight", "0.batchnorm.bias", "1.conv.weight", "1.batchnorm.weight",
          "1.batchnorm.bias", "2.conv.weight", "2.conv.bias")
BUFFERS = ("0.batchnorm.running_mean", "0.batchnorm.running_var", "1.batchnorm.running_mean", "1.batchnorm.running_var")
BAND_CAP = 1e-3


@functools.lru_cache(maxsize=None)
def mlp_case(B, rows, inner, add):
    """-> (seq, x (B,3,L), pe (B,64,rows) or None, dout (B,64,L)): a `_point_mlp(3, 64, 64)` on the CPU in training mode
    with BatchNorm parameters and running statistics away from their defaults.  Cached: deep-copy the module."""
    from pose2room_amd.p2rnet.modules.stgcn import _point_mlp
    L = rows * inner
    saved = torch.random.get_rng_state()
    try:
        torch.manual_seed(15000 + B * 100 + rows + inner)
        seq = _point_mlp(3, 64, 64)
        with torch.no_grad():
            for m in seq.modules():
                if isinstance(m, torch.nn.BatchNorm1d):
                    m.weight.uniform_(0.5, 1.5), m.bias.uniform_(-0.5, 0.5)
                    m.running_mean.uniform_(-0.2, 0.2), m.running_var.uniform_(0.5, 2.0)
        x = torch.randn(B, 3, L) * torch.tensor([1.0, 0.4, 2.0])[None, :, None]
        pe = torch.randn(B, 64, rows) if add else None
        dout = torch.randn(B, 64, L)
    finally:
        torch.random.set_rng_state(saved)
    return seq, x, pe, dout


def mlp_inputs(seq):
    """(params, bn_buffers) of a `_point_mlp` stack as dicts of detached tensors, keyed like its state_dict"""
    sd = {k: v.detach().clone() for k, v in seq.state_dict().items()}
    return {k: sd[k] for k in PARAMS}, {k: sd[k] for k in BUFFERS}


def mlp_ref(x, params, bn_buffers, train, inner, add, dout, gates=None, momentum=0.1, eps=1e-5):
    """The cbr, cbr, c chain in float64 under autograd.  Each ReLU is y * gate with gate = (y > 0) when `gates` is None,
    else the given pair of boolean tensors (B,64,L) as constants.  add (B,64,L/inner) or None is added to the output,
    broadcast over `inner`.  -> dict: 'out', 'grads' {name: gradient}, 'd_add', 'running' {name: updated statistic},
    'y1', 'y2' (the two pre-activations)"""
    p = {k: v.detach().double().requires_grad_(True) for k, v in params.items()}
    pe = add.detach().double().requires_grad_(True) if add is not None else None
    x = x.double()
    B, _, L = x.shape
    running = {}

    def conv(v, w, bias=None):
        y = torch.einsum("oi,nil->nol", w.reshape(w.shape[0], w.shape[1]), v)
        return y if bias is None else y + _c(bias)

    def bn(v, i):
        pre = f"{i}.batchnorm."
        rm, rv = bn_buffers[pre + "running_mean"].double(), bn_buffers[pre + "running_var"].double()
        if train:
            mean, var = v.mean((0, 2)), v.var((0, 2), unbiased=False)
            n = v.shape[0] * v.shape[2]
            running[pre + "running_mean"] = ((1 - momentum) * rm + momentum * mean).detach()
            running[pre + "running_var"] = ((1 - momentum) * rv + momentum * var * (n / max(n - 1, 1))).detach()
        else:
            mean, var = rm, rv
            running[pre + "running_mean"], running[pre + "running_var"] = rm, rv
        return (v - _c(mean)) * _c((var + eps).rsqrt() * p[pre + "weight"]) + _c(p[pre + "bias"])

    ys = []
    v = x
    for i in (0, 1):
        y = bn(conv(v, p[f"{i}.conv.weight"], p.get(f"{i}.conv.bias")), i)
        gate = (y > 0) if gates is None else gates[i]
        ys.append(y.detach())
        v = y * gate.detach().double()
    out = conv(v, p["2.conv.weight"], p.get("2.conv.bias"))
    if pe is not None:
        out = (out.view(B, C, L // inner, inner) + pe.unsqueeze(-1)).view(B, C, L)
    out.backward(dout.double())
    return {"out": out.detach(), "grads": {k: v.grad for k, v in p.items()}, "d_add": pe.grad if pe is not None else None,
            "running": running, "y1": ys[0], "y2": ys[1]}


def module_chain_ref(seq, x, pe, inner, dout, train):
    """the same quantities from a float64 deep copy of the module under autograd"""
    ref = copy.deepcopy(seq).double().train(train)
    add = pe.detach().double().requires_grad_(True) if pe is not None else None
    B, _, L = x.shape
    out = ref(x.double())
    if add is not None:
        out = (out.view(B, C, L // inner, inner) + add.unsqueeze(-1)).view(B, C, L)
    out.backward(dout.double())
    sd = ref.state_dict()
    return {"out": out.detach(), "grads": {k: v.grad for k, v in ref.named_parameters()},
            "d_add": add.grad if add is not None else None, "running": {k: sd[k] for k in BUFFERS}}


def band_share(y, width=FWD_TOL):
    """share of the elements of a pre-activation within `width` max|y| of zero: the gates a forward error of the
    project's tolerance could turn"""
    return (y.abs() <= width * y.abs().max()).double().mean().item()


def saved_stage_tensors(out):
    """(z1, z2, fin1, fin2) that embed_op._EmbedMLP saved for its backward: the conv outputs (B,64,L) of the first two
    layers and the (mean, invstd, scale, shift) [4][64] of their BatchNorms.  The one place that knows the op's layout."""
    _, z1, z2, fin1, fin2 = out.grad_fn.saved_tensors[:5]
    return z1, z2, fin1, fin2


def rel_err(got, want):
    """max |got - want| / max |want|, the measure of the project's tolerances for this MLP"""
    want = want.double()
    return ((got.detach().double() - want).abs().max() / (want.abs().max() + 1e-12)).item()
