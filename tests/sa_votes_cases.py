"""Scenes and the float64 reference of the fused vote aggregation (csrc/sa_votes.hip, pointnet2_ops/fused.py), shared by
tests/test_sa_votes_reference_cpu.py and tests/test_sa_votes_sweep_gpu.py.

The reference is plain float64 torch, one function per stage, so a stage of the kernel can be compared on the kernel's
OWN stage input and its error is not mixed with the error of the stage before.  Next to every value comes its
running-error bound: the same expression on absolute values times gamma(k) = k u / (1 - k u), u = 2^-24, k = the
number of rounded fp32 operations an operand can pass on its way into one output element.  The bound is derived, not
measured, and holds for every summation order with one round-to-nearest per operation (a fused multiply-add rounds
less often, never more):

  * a layer z = W x + b: an accumulator starting at zero takes 256 products, then the bias.  The first product is
    rounded once and passes 256 + 1 additions: k = 258.
  * a transposed layer (no bias): k = 257.
  * a weight gradient over nb * L columns in `split` ranges whose partials are then added: k = nb * L + split; one
    partial over `cols` columns: k = cols + 1.
  * a bias gradient, the sum of nb * L values: k = nb * L.
  * the scatter of dG back to a point that fills `slots` slots: k = slots + 1.

The float64 evaluation itself errs by 2^-53 per operation, 2^-29 of the bound: ignored.
"""
import collections
import functools

import torch

from tests import cases

U = 2.0 ** -24
C = 256
S = 16
K_LAYER = 258
K_LAYER_T = 257

Scene = collections.namedtuple("Scene", "name B N M kind radius seed offset")
SCENES = [
    # full balls, early exit of the query loop before N, a last workgroup with one live wave, four query trips
    Scene("walk", 2, 200, 9, "walk", 0.3, 1, 0.0),
    # counts 6..17: padded and full balls in one workgroup, N % 64 != 0
    Scene("partial", 1, 130, 13, "uniform", 1.2, 2, 0.0),
    # squared distances exactly r^2 (strict <), duplicate points
    Scene("edge", 1, 600, 6, "halflattice", 0.5, 3, 0.0),
    # one-point balls: 16 identical columns, N == 64 exactly
    Scene("dup", 3, 64, 6, "lattice", 0.3, 4, 0.0),
    # three dead waves
    Scene("m1", 1, 33, 1, "uniform", 0.3, 5, 0.0),
    # N < 16 < 64: every ball holds all points, then pads; M < 4 in every cloud
    Scene("m3b", 5, 5, 3, "uniform", 5.0, 6, 0.0),
    # empty balls: idx all 0, feature column 0 everywhere
    Scene("empty", 1, 40, 5, "uniform", 0.3, 7, 100.0),
]
BY_NAME = {s.name: s for s in SCENES}
NAMES = [s.name for s in SCENES]
INPUTS = ("xyz", "new_xyz", "features", "w1", "b1", "w2", "b2", "dout")


@functools.lru_cache(maxsize=None)
def scene(name):
    """dict of CPU float32 tensors xyz (B,N,3), new_xyz (B,M,3), features (B,256,N), w1, w2 (256,256), b1, b2 (256),
    dout (B,256,M), and `radius`.  Cached: callers must not write into the tensors."""
    s = BY_NAME[name]
    g = torch.Generator().manual_seed(7000 + s.seed)
    xyz = cases.cloud(s.B, s.N, s.seed, s.kind)
    new_xyz = (cases.centres_from(xyz, s.M, s.seed) + s.offset).contiguous()
    weight = lambda: ((torch.rand(C, C, generator=g) * 2 - 1) * (2.4 / C ** 0.5)).contiguous()
    features = torch.randn(s.B, C, s.N, generator=g)
    w1, b1 = weight(), 0.1 * torch.randn(C, generator=g)
    w2, b2 = weight(), 0.1 * torch.randn(C, generator=g)
    b2[::4] -= 6.0                      # these channels pool to exactly 0: the `out > 0` gate and the all-tie rule
    dout = torch.randn(s.B, C, s.M, generator=g)
    return {"xyz": xyz, "new_xyz": new_xyz, "features": features, "w1": w1, "b1": b1, "w2": w2, "b2": b2,
            "dout": dout, "radius": s.radius}


def gamma(k):
    return k * U / (1.0 - k * U)


# ---- ball membership in plain torch (the reference of the indices is the oracle; this one gives the hit counts) ----------
def ball_hits(xyz, new_xyz, radius):
    """(B,M,N) bool: fp32 squared distance, summed x, y, z in this order, strictly below fp32 radius^2"""
    d = new_xyz[:, :, None, :] - xyz[:, None, :, :]
    d2 = d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]
    r = torch.tensor(radius, dtype=torch.float32)
    return d2 < r * r


def ball_query(xyz, new_xyz, radius, nsample=S):
    """-> idx (B,M,nsample) int32: the first `nsample` hits in ascending order, the rest filled with the first hit,
    zeros for an empty ball; and the hit counts (B,M), not capped"""
    hit = ball_hits(xyz, new_xyz, radius)
    n = xyz.shape[1]
    cnt = hit.sum(-1)
    order = torch.where(hit, torch.arange(n).expand_as(hit), torch.full_like(hit, n, dtype=torch.int64))
    order = torch.sort(order, dim=-1).values[..., :nsample]
    if order.shape[-1] < nsample:
        order = torch.cat([order, order.new_full(order.shape[:-1] + (nsample - order.shape[-1],), n)], -1)
    first = torch.where(cnt > 0, order[..., 0], torch.zeros_like(cnt))
    idx = torch.where(order < n, order, first[..., None].expand_as(order))
    return idx.to(torch.int32), cnt


def first_slot(idx):
    """(B,M,S) -> (B,M,S) int64: the lowest slot of the ball that holds the same point"""
    same = idx[..., :, None] == idx[..., None, :]
    return same.to(torch.uint8).argmax(-1)


# ---- forward stages ---------------------------------------------------------------------------------------------------------
def gather(features, idx):
    """features (B,C,N), idx (B,M,S) -> (B,C,M,S) in the dtype of `features`: a copy, exact"""
    B, Cn, _ = features.shape
    _, M, Sn = idx.shape
    flat = idx.long().reshape(B, 1, M * Sn).expand(B, Cn, M * Sn)
    return torch.gather(features, 2, flat).reshape(B, Cn, M, Sn)


def layer(W, b, X):
    """pre-activation W X + b of a 1x1 convolution, X (B,256,M,S) -> (z, E) in float64, E = gamma(258) (|W| |X| + |b|)"""
    W, b, X = W.double(), b.double(), X.double()
    z = torch.einsum("oc,bcms->boms", W, X) + b[None, :, None, None]
    mag = torch.einsum("oc,bcms->boms", W.abs(), X.abs()) + b.abs()[None, :, None, None]
    return z, gamma(K_LAYER) * mag


def pool(z2, idx=None):
    """max over the samples of relu(z2) and its arg-max, first index on ties.  With `idx`, a slot that repeats the point
    of a lower slot does not take part: its column is the same column, so the lower slot wins whatever the last bits."""
    v = torch.relu(z2)
    if idx is not None:
        repeat = first_slot(idx) != torch.arange(idx.shape[-1])
        v = v.masked_fill(repeat[:, None], -1.0)
    val, arg = v.max(-1)
    return val, arg


def margins(z1, E1, z2, E2, idx):
    """Which decisions of a scene fp32 rounding could turn: bool tensors, True = undecided (margin below twice the bound).
      h:   |z1| < 2 E1                                            (B,C,M,S)
      out: |largest pre-activation of the ball| < 2 max E2         (B,C,M): covers 0 < out < 2 E2 and the mirror image
      arg: out > 0 and the two largest pre-activations of DISTINCT points closer than 2 max E2   (B,C,M)"""
    repeat = first_slot(idx) != torch.arange(idx.shape[-1])
    z = z2.masked_fill(repeat[:, None], float("-inf"))
    top = torch.topk(z, 2, dim=-1).values
    e = E2.max(-1).values
    return {"h": z1.abs() < 2 * E1, "out": top[..., 0].abs() < 2 * e,
            "arg": (top[..., 0] > 0) & (top[..., 0] - top[..., 1] < 2 * e)}


# ---- backward stages --------------------------------------------------------------------------------------------------------
def dz2_stage(dout, amax, positive):
    """dZ2 (B,C,M,S): dout at the arg-max sample where the pooled output is positive, else 0.  Exact, in dout's dtype."""
    hot = torch.arange(S)[None, None, None, :] == amax.long()[..., None]
    return torch.where(hot & positive[..., None], dout[..., None].expand(hot.shape), torch.zeros((), dtype=dout.dtype))


def layer_t(W, dZ):
    """W^T dZ for W [out][in], dZ (B,256,M,S) -> (value, E), E = gamma(257) |W|^T |dZ|"""
    W, dZ = W.double(), dZ.double()
    return (torch.einsum("oc,boms->bcms", W, dZ), gamma(K_LAYER_T) * torch.einsum("oc,boms->bcms", W.abs(), dZ.abs()))


def dz1_stage(W2, dZ2, active):
    """(W2^T dZ2) where the hidden unit is active, exactly 0 elsewhere -> (value, E)"""
    v, e = layer_t(W2, dZ2)
    zero = torch.zeros((), dtype=torch.float64)
    return torch.where(active, v, zero), torch.where(active, e, zero)


def dg_stage(W1, dZ1):
    return layer_t(W1, dZ1)


def _scatter(x, idx, n):
    B, Cn, M, Sn = x.shape
    flat = idx.long().reshape(B, 1, M * Sn).expand(B, Cn, M * Sn)
    return torch.zeros(B, Cn, n, dtype=x.dtype).scatter_add_(2, flat, x.reshape(B, Cn, M * Sn))


def dfeat_stage(dG, idx, n):
    """gradient of the gather: every point sums the slots that hold it -> (value, E), E = gamma(slots + 1) sum |dG|"""
    dG = dG.double()
    slots = _scatter(torch.ones(idx.shape[0], 1, *idx.shape[1:], dtype=torch.float64), idx, n)
    return _scatter(dG, idx, n), gamma(slots + 1) * _scatter(dG.abs(), idx, n)


def dw_stage(dZ, X, split):
    """sum over samples and positions of dZ X^T, dZ, X (B,256,M,S) -> (value (256,256), E)"""
    dZ, X = dZ.double(), X.double()
    k = dZ.shape[0] * dZ.shape[2] * dZ.shape[3] + split
    return (torch.einsum("boms,bcms->oc", dZ, X), gamma(k) * torch.einsum("boms,bcms->oc", dZ.abs(), X.abs()))


def db_stage(dZ):
    dZ = dZ.double()
    k = dZ.shape[0] * dZ.shape[2] * dZ.shape[3]
    return dZ.sum((0, 2, 3)), gamma(k) * dZ.abs().sum((0, 2, 3))


# ---- end to end -------------------------------------------------------------------------------------------------------------
def forward(sc, idx, active=None):
    """The whole forward in float64 on the indices `idx`.  `active` (B,C,M,S) bool: the implementation's H > 0, taken in
    place of the reference's own; E2 is then the one-stage bound on the reference's H, the cascade is in `backward`."""
    G = gather(sc["features"], idx)
    z1, E1 = layer(sc["w1"], sc["b1"], G)
    if active is None:
        active = z1 > 0
    H = torch.where(active, z1, torch.zeros((), dtype=torch.float64))
    z2, E2 = layer(sc["w2"], sc["b2"], H)
    out, amax = pool(z2, idx)
    return {"idx": idx, "G": G, "z1": z1, "E1": E1, "active": active, "H": H, "z2": z2, "E2": E2, "out": out, "amax": amax}


def backward(sc, fwd, amax=None, positive=None, split=1):
    """Gradients of sum(out * dout) in float64 and their CASCADED bounds for an fp32 implementation that took the
    decisions `fwd['active']` (H > 0), `amax` and `positive` (out > 0): name -> (value, E) for dfeat, dw1, db1, dw2,
    db2, and the intermediates dZ2, dZ1, dG.

    Cascade: x~ the implementation's value of x, |x~ - x| <= Ex.  A product fl(A~ B~) errs from A B by at most
    EA |B| + (|A| + EA) EB + gamma(k) (|A| + EA)(|B| + EB); operands that are inputs have E = 0.
      H:   relu is 1-Lipschitz and the mask is the implementation's own: EH = E1 where active, 0 elsewhere.
      dZ2: a copy of dout: exact.        dZ1: E = gamma(257) |W2|^T |dZ2| where active.
      dG:  |W1|^T EdZ1 + gamma(257) |W1|^T (|dZ1| + EdZ1).
      dfeat: scatter(EdG) + gamma(slots + 1) scatter(|dG| + EdG).
      dw1: EdZ1 |G|^T + gamma(k) (|dZ1| + EdZ1) |G|^T.      dw2: |dZ2| EH^T + gamma(k) |dZ2| (|H| + EH)^T.
      db1: sum EdZ1 + gamma(nb L) sum (|dZ1| + EdZ1).      db2: gamma(nb L) sum |dZ2|."""
    idx, G, H, active = fwd["idx"], fwd["G"].double(), fwd["H"], fwd["active"]
    amax = fwd["amax"] if amax is None else amax
    positive = fwd["out"] > 0 if positive is None else positive
    n = sc["features"].shape[2]
    w1a, dout = sc["w1"].double().abs(), sc["dout"].double()
    zero = torch.zeros((), dtype=torch.float64)
    EH = torch.where(active, fwd["E1"], zero)
    dZ2 = dz2_stage(dout, amax, positive)
    dZ1, EdZ1 = dz1_stage(sc["w2"], dZ2, active)
    dG, _ = dg_stage(sc["w1"], dZ1)
    EdG = torch.einsum("oc,boms->bcms", w1a, EdZ1) + gamma(K_LAYER_T) * torch.einsum("oc,boms->bcms", w1a, dZ1.abs() + EdZ1)
    dfeat, _ = dfeat_stage(dG, idx, n)
    slots = _scatter(torch.ones(idx.shape[0], 1, *idx.shape[1:], dtype=torch.float64), idx, n)
    Edfeat = _scatter(EdG, idx, n) + gamma(slots + 1) * _scatter(dG.abs() + EdG, idx, n)
    nbl = dZ2.shape[0] * dZ2.shape[2] * dZ2.shape[3]
    prod = lambda a, b: torch.einsum("boms,bcms->oc", a, b)
    dw1 = prod(dZ1, G)
    Edw1 = prod(EdZ1, G.abs()) + gamma(nbl + split) * prod(dZ1.abs() + EdZ1, G.abs())
    dw2 = prod(dZ2, H)
    Edw2 = prod(dZ2.abs(), EH) + gamma(nbl + split) * prod(dZ2.abs(), H.abs() + EH)
    db1 = dZ1.sum((0, 2, 3))
    Edb1 = EdZ1.sum((0, 2, 3)) + gamma(nbl) * (dZ1.abs() + EdZ1).sum((0, 2, 3))
    db2, Edb2 = db_stage(dZ2)
    return {"dZ2": (dZ2, torch.zeros_like(dZ2)), "dZ1": (dZ1, EdZ1), "dG": (dG, EdG), "dfeat": (dfeat, Edfeat),
            "dw1": (dw1, Edw1), "db1": (db1, Edb1), "dw2": (dw2, Edw2), "db2": (db2, Edb2)}


def worst(got, want, bound):
    """(largest |got - want| / bound, its index) over the elements; an element with bound 0 must be exact (ratio 0 or inf)"""
    err = (got.detach().double() - want).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound)
    if ratio.numel() == 0:
        return 0.0, ()
    flat = int(ratio.reshape(-1).argmax())
    at = []
    for d in reversed(ratio.shape):
        at.append(flat % d)
        flat //= d
    return float(ratio.reshape(-1).max()), tuple(reversed(at))


# ---- p2r_gemm_nt_256 ----------------------------------------------------------------------------------------------------------
GEMM_CASES = [  # (nb, L, split)
    (1, 16, 1),        # L < one chunk
    (1, 64, 1),        # one fast-path chunk
    (4, 64, 3),        # fast path, a part spanning samples
    (3, 48, 4),        # scalar path, chunks that cross samples
    (1, 592, 64),      # M = 37
    (2, 128, 64),      # more parts than chunks
    (1, 16, 1024),     # largest split
]


def gemm_ranges(nb, L, split):
    """column range [lo, hi) of every part over the nb * L columns, sample-major: `per` = the columns per part, rounded
    up to whole 64-column chunks (the rule in front of gemm_nt_kernel, csrc/sa_votes.hip)"""
    total = nb * L
    per = -(-(-(-total // split)) // 64) * 64
    return [(min(p * per, total), min((p + 1) * per, total)) for p in range(split)]


@functools.lru_cache(maxsize=None)
def gemm_operands(nb, L, seed=0):
    g = torch.Generator().manual_seed(9000 + 131 * nb + L + seed)
    return torch.randn(nb, C, L, generator=g), torch.randn(nb, C, L, generator=g)


def gemm_reference(A, B, lo, hi):
    """sum over the columns [lo, hi) of the sample-major column axis of A[:, m, col] B[:, n, col] -> (value, E) float64
    with E = gamma(cols + 1) |A| |B|^T"""
    nb, _, L = A.shape
    a = A.double().permute(1, 0, 2).reshape(C, nb * L)[:, lo:hi]
    b = B.double().permute(1, 0, 2).reshape(C, nb * L)[:, lo:hi]
    return torch.einsum("ml,nl->mn", a, b), gamma(hi - lo + 1) * torch.einsum("ml,nl->mn", a.abs(), b.abs())
