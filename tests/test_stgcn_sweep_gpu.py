"""GPU: the exact-fp32 ST-GCN convolution kernels of all three generations against the float64 stage references of
tests/stgcn_cases.py, through the C entry points of include/p2r_hip.h on raw pointers.

Stage level, every output poison-filled inside poisoned guard bands (tests/memguard.py: nothing written outside, no
element left unwritten), every stage on the kernel's OWN fp32 input, per element within the derived running-error bound
on the bounded cases and EQUAL to the float64 value on the exact cases (tests/test_stgcn_reference_cpu.py proves the same
`check` sensitive to fourteen named defects):
  * third generation, forward + (count, mean, M2) entries, data gradient with plain / masked addend (bytes 0, 1, 2, 255)
    with and without the BatchNorm-backward sums epilogue, at (N, T) = (1, 16), (2, 32), (3, 48) and at (17, 256): 272
    tiles over 256 workgroups, the second round in another sample;
  * second generation at the same shapes, T in 1, 7, 15, 17, 31, 33, the extra-link adjacency, a misaligned addend;
  * first generation at V = 17, 25, 56 with T = 384 // V and one above: forward, data gradient, weight, bias-table and
    adjacency gradients;
  * gcn3_weight_grad at T = 4, 8, 20 (3, 8, 25 tiles) x n_blocks 1, 3, 8, 16, 24, 256 (both tile orders, tile counts
    below, equal to and above n_blocks and no multiple of it), gcn3_coef_grad at n_blocks 1, 3, 8, 256;
  * tconv3 / tconv2 / tconv forward with three taps and one, tconv3_forward_add, the data gradient with its sums epilogue,
    tconv_weight_grad (53 joints, another joint count, the 12-frame instance of 20 columns) and tconv_weight_grad_dz;
  * the gate case in every kernel that forms the ReLU gate, p2r_bn_bwd_reduce / p2r_bn_bwd_apply (relu = 2) included;
  * every refusal of the header (P2R_EINVAL, outputs untouched) and N == 0 per entry point.
Op level: gcn_op.graph_conv and tconv_op.bn_relu_tconv (train and eval, with add_ct) on one bounded and one exact case,
every gradient per element against the bound composed from the stage bounds.

Findings, fixed in this change:
  * p2r_stgcn_gcn_coef_grad (first generation) added, into every slot below the LONGEST list of an n-tile's joints, the
    products with joint 0 -- a padded slot of a joint with a shorter list came out non-zero (61 to 294 slots of the ring
    skeletons here).  gcn_op drops those slots when it scatters the table, so no gradient was wrong, but the header's table
    convention was not kept; the kernel now adds real slots only (stgcn_cases mutant 'pad_below_tile_longest').
  * N == 0: p2r_stgcn_gcn3_weight_grad refused, p2r_stgcn_gcn3_coef_grad zero-filled, and p2r_stgcn_gcn_weight_grad /
    p2r_stgcn_gcn_coef_grad / p2r_stgcn_tconv_weight_grad(_dz) returned P2R_OK with their [n_blocks][...] partials
    UNWRITTEN, which their callers then add up.  All of them zero-fill now; the header states it (test_empty_batch).
  * p2r_stgcn_tconv_weight_grad refuses more than 57 joints with three taps (LDS) while tconv_op.supported allowed 64:
    `supported` now says 57, the header states both limits.
No test exposed a wrong value; no kernel arithmetic changed.

Worst observed error / derived bound per stage over the whole sweep (one run on an MI355X; 1 would be at the limit).
Every exact and gate case, 54 stages, was bit for bit the float64 value.
  gcn3: forward 0.029, data gradient 0.0072 (masked addend 0.0073), (count, mean, M2) 0.015, sums epilogue 0.018,
        weight gradient 0.0099, colsum 0.41, adjacency gradient 0.0012
  gcn2: forward 0.030 (extra link 0.023), data gradient 0.0058, (sum, sum sq) 0.0038, sums epilogue 0.0016
  gcn (first generation): forward 0.0070, data gradient 0.0062, (sum, sum sq) 0.0072, weight gradient 0.010, colsum 0.0088,
        adjacency gradient < 1e-4 (the any-order bound of a float-atomic sum is wide)
  tconv3: three taps 0.036, one tap 0.10, forward_add 0.097, data gradient 0.030, (count, mean, M2) 0.029, sums epilogue 0.017
  tconv2: three taps 0.037, one tap 0.10, data gradient 0.030, (sum, sum sq) 0.0034, sums epilogue 0.0016
  tconv (first generation): three taps 0.029, one tap 0.099, data gradient 0.026, (sum, sum sq) 0.041
  tconv_weight_grad: dW 0.011 (one tap 0.0092; V = 20 / 25 / 57 / 64: 0.0076 / 0.013 / 0.0051 / 0.0035), dbias 0.030,
        dz of the fused apply pass 0.85 (five roundings: little room by construction)
  op level: graph_conv z 0.0046, dx 0.0054, dW 0.0013, db 0.0009, dAeff 0.0006; bn_relu_tconv (train) out 0.12, dz 0.042,
        dW 0.0013, dbias 0.0003, dgamma 0.0005, dbeta 0.0004, dadd_ct 0.064
As fractions of the reference's largest entry -- what the borrowed tolerances of tests/test_gcn_gpu.py and
tests/test_tconv_gpu.py are fractions of -- the worst errors were 1.0e-7 .. 2.6e-6 (graph conv forward 2.1e-6, gcn3 weight
gradient 2.6e-6, temporal conv 6.5e-7, statistics 2.2e-7): the old 2e-5 (z, dx, gcn3 adjacency gradient) had a headroom of
10 to 70, 5e-5 (dW, db, d importance) of 19 to 430, 3e-5 / 1e-4 (temporal conv output / gradients) of 50 to 950, the
statistics' rtol 1e-4 of 450, the chained blocks' 2e-4 of at least 75.  The derived bounds leave 2.4 (colsum) to some
hundred, per element and relative to each element's own terms.
"""
import ctypes

import pytest
import torch

from tests import memguard
from tests import stgcn_cases as S

pytestmark = pytest.mark.gpu

EINVAL = "failed with status -22"
F32 = torch.float32
V = 53
K = S.K
SHAPES = [(1, 16), (2, 32), (3, 48)]
FAMILIES = ["bounded", "exact"]

RATIOS = {}     # stage -> worst error / bound of this session (printed by the last test)
# (the sums of squares of the statistics are no exact quantity -- z^2 leaves the exact range -- and the merges divide by
# counts: statistics are judged by their bounds in every family)


REL = {}        # stage -> worst error / largest entry of the reference: what the borrowed tolerances were fractions of


def _note(stage, ratio):
    RATIOS[stage] = max(RATIOS.get(stage, 0.0), float(ratio))


def _out(shape, dev, dtype=F32, offset_bytes=0):
    return memguard.guarded(shape, dtype, dev, fill="poison", halo="poison", offset_bytes=offset_bytes)


def _in(t, dev, offset_bytes=0):
    return memguard.guarded(t.shape, t.dtype, dev, fill=t, halo="zero", offset_bytes=offset_bytes)[1]


def _written(*pairs):
    torch.cuda.synchronize()
    res = []
    for p in pairs:
        if p is None:
            res.append(None)
            continue
        assert int(memguard.halo_damage(p[0], p[1], "poison")) == 0, "written outside the buffer"
        assert int(memguard.poison_count(p[1])) == 0, "an element was never written"
        res.append(p[1])
    return res


def _untouched(*pairs):
    torch.cuda.synchronize()
    for buf, view in pairs:
        assert int(memguard.halo_damage(buf, view, "poison")) == 0, "written outside the buffer"
        assert int(memguard.poison_count(view)) == view.numel(), "written although the call does nothing"


def _launch(dev, name, *args):
    from pose2room_amd import _lib
    _lib.launch(name, dev, *args)


def _refused(dev, name, args, outs):
    with pytest.raises(RuntimeError, match=name + " " + EINVAL):
        _launch(dev, name, *args)
    _untouched(*outs)


class Dev:
    """the operands of one case on the device, each inside a zero halo, made on first use"""

    def __init__(self, ops, dev):
        self.ops, self.dev, self._c = ops, dev, {}
        self.tab = ops.tab

    def __getitem__(self, key):
        if key not in self._c:
            from pose2room_amd.p2rnet import gcn_op, tconv_op
            o = self.ops
            if key == "Wp":
                t = gcn_op.permute_planes(self["W"])
            elif key == "WpT":
                t = gcn_op.permute_planes(self["W"].transpose(1, 2).contiguous())
            elif key == "WT":
                t = self["W"].transpose(1, 2).contiguous()
            elif key in ("W3p", "W1p", "W3gp", "W1gp"):
                t = tconv_op._permute_taps(self[key[:-1]])
            elif key == "W3b":
                t = self["W3"].flip(0).transpose(1, 2).contiguous()
            elif key == "W3bp":
                t = tconv_op._permute_taps(self["W3b"])
            elif key in ("scale", "shift"):
                t = self["fin"][2 if key == "scale" else 3].contiguous()
            elif key in ("P0", "P1"):
                t = S.planes_of(self.tab, int(key[1]), self["coef" + key[1]])
            else:
                t = _in(o[key], self.dev)
            self._c[key] = t
        return self._c[key]


_CASES = {}


def _case(dev, N, T, family, kind="skeleton", Vn=V, **kw):
    key = (N, T, family, kind, Vn, tuple(sorted(kw.items())))
    if key not in _CASES:
        _CASES[key] = Dev(S.Operands(N, T, V=Vn, family=family, kind=kind, **kw), dev)
    return _CASES[key]


_TABLES = {}


def _graph(dev, kind="skeleton", Vn=V):
    """(gcn_op.GraphTables, its device tables) of an adjacency of stgcn_cases.tables"""
    if (kind, Vn) not in _TABLES:
        from pose2room_amd.p2rnet import gcn_op
        gt = gcn_op.GraphTables(S.tables(kind, Vn)["A"].numpy())
        assert torch.equal(gt.gidx_r, S.tables(kind, Vn)[1]["gidx"])
        _TABLES[(kind, Vn)] = (gt, gt.on(dev))
    return _TABLES[(kind, Vn)]


def _check(stage, got, ref, exact, unit=None):
    if exact and unit is not None and len(ref) > 2:
        assert S.exact_cap(ref[2], unit) < S.TWO24, f"{stage}: the exact case leaves the exact range"
    _note(stage + (" (exact)" if exact else ""), S.check(got, ref, exact, stage))
    if not exact and ref[0].numel():
        rel = float((got.double() - ref[0]).abs().max() / ref[0].abs().max().clamp_min(1e-300))
        REL[stage] = max(REL.get(stage, 0.0), rel)


def _nb16(N, T):
    return min(N * ((T + 15) // 16), 256)


# ---- graph convolution, third generation ----------------------------------------------------------------------------------------
def _gcn3_all(dev, d, N, T):
    """forward + statistics, data gradient with plain addend, masked addend with and without the sums epilogue"""
    ex = d.ops.exact
    nb = _nb16(N, T)
    ltc, ltr = d.tab[0]["ltot"], d.tab[1]["ltot"]
    z, part = _out((N, 64, T, V), dev), _out((nb, 64, 3), dev)
    _launch(dev, "p2r_stgcn_gcn3_forward", N, T, V, K, ltc, 0, d["x"], d["Wp"], d["coef0"], d["bias_cv"], None, z[1], part[1],
            None, None, None, None)
    zv, pv = _written(z, part)
    _check("gcn3 forward", zv, S.graph_conv_ref(d["x"], d["W"], d["P0"], d["bias_cv"]), ex, 0.25)
    if not ex:
        _check("gcn3 forward statistics", pv, S.stats3_ref(zv, nb), False)
    else:
        assert torch.equal(pv[:, :, 0], S.stats3_ref(zv, nb)[0][:, :, 0].float())         # the counts
    # data gradient, plain addend, no statistics
    dx = _out((N, 64, T, V), dev)
    _launch(dev, "p2r_stgcn_gcn3_forward", N, T, V, K, ltr, 1, d["dz"], d["WpT"], d["coef1"], None, d["addend"], dx[1], None,
            None, None, None, None)
    (dxv,) = _written(dx)
    _check("gcn3 data gradient", dxv, S.graph_conv_ref(d["dz"], d["WT"], d["P1"], None, d["addend"]), ex, 0.25)
    # the same launch with the sums epilogue (unmasked addend)
    dx, sums = _out((N, 64, T, V), dev), _out((nb, 64, 2), dev)
    _launch(dev, "p2r_stgcn_gcn3_forward", N, T, V, K, ltr, 1, d["dz"], d["WpT"], d["coef1"], None, d["addend"], dx[1], sums[1],
            None, d["u"], d["bmask"], d["fin"])
    dxv2, sv = _written(dx, sums)
    assert torch.equal(dxv2, dxv)
    _check("gcn3 sums epilogue", sv, S.bwd_sums_ref(dxv2, d["u"], d["fin"], nb, "gcn3", bmask=d["bmask"]), ex, 0.125)
    # masked addend: with the epilogue, and plain
    ref = S.graph_conv_ref(d["dz"], d["WT"], d["P1"], None, d["addend"], d["amask"])
    dx, sums = _out((N, 64, T, V), dev), _out((nb, 64, 2), dev)
    _launch(dev, "p2r_stgcn_gcn3_data_gradient_masked_addend", N, T, V, K, ltr, d["dz"], d["WpT"], d["coef1"], d["addend"],
            d["amask"], dx[1], sums[1], d["u"], d["bmask"], d["fin"])
    dxm, sv = _written(dx, sums)
    _check("gcn3 data gradient, masked addend", dxm, ref, ex, 0.25)
    _check("gcn3 sums epilogue", sv, S.bwd_sums_ref(dxm, d["u"], d["fin"], nb, "gcn3", bmask=d["bmask"]), ex, 0.125)
    dx = _out((N, 64, T, V), dev)
    _launch(dev, "p2r_stgcn_gcn3_data_gradient_masked_addend", N, T, V, K, ltr, d["dz"], d["WpT"], d["coef1"], d["addend"],
            d["amask"], dx[1], None, None, None, None)
    (dxp,) = _written(dx)
    assert torch.equal(dxp, dxm)


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("N,T", SHAPES)
def test_gcn3_forward_and_data_gradient(dev, N, T, family):
    _gcn3_all(dev, _case(dev, N, T, family), N, T)


@pytest.mark.parametrize("family", FAMILIES)
def test_gcn3_more_tiles_than_workgroups(dev, family):
    """(17, 256): 272 tiles over 256 workgroups; tiles 256 .. 271 are in sample 16, so workgroups 0 .. 15 walk two tiles
    of different samples and their statistics entries count twice as many values"""
    N, T = 17, 256
    d = _case(dev, N, T, family, density=0.125)
    _gcn3_all(dev, d, N, T)
    _CASES.clear()          # 60 MB per tensor


# ---- graph convolution, second generation ---------------------------------------------------------------------------------------
def _gcn2(dev, d, gt, N, T, form, addend=None, bwd=False, stats=True, z=None):
    t = gt[1]
    stream = t["stream_c" if form == 0 else "stream_r"]
    work = _out(tuple(stream.shape), dev, dtype=torch.int32)
    nb = _nb16(N, T)
    z = z or _out((N, 64, T, V), dev)
    part = _out((nb, 64, 2), dev) if stats or bwd else None
    x, Wp, coef = (d["x"], d["Wp"], d["coef0"]) if form == 0 else (d["dz"], d["WpT"], d["coef1"])
    _launch(dev, "p2r_stgcn_gcn2_forward", N, T, V, K, coef.shape[0], x, Wp, coef, stream, work[1], d["bias_cv"] if form == 0 else None,
            addend, z[1], part[1] if part else None, None, d["u"] if bwd else None, d["bmask"] if bwd else None,
            d["fin"] if bwd else None)
    return _written(z, part)


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("N,T", SHAPES + [(2, 1), (2, 7), (2, 15), (2, 17), (2, 31), (2, 33)])
def test_gcn2_forward_and_data_gradient(dev, N, T, family):
    d, gt = _case(dev, N, T, family), _graph(dev)
    ex, nb = d.ops.exact, _nb16(N, T)
    zv, pv = _gcn2(dev, d, gt, N, T, 0)
    _check("gcn2 forward", zv, S.graph_conv_ref(d["x"], d["W"], d["P0"], d["bias_cv"]), ex, 0.25)
    _check("gcn2 forward statistics", pv, S.stats2_ref(zv, nb, 16), False)
    dxv, sv = _gcn2(dev, d, gt, N, T, 1, addend=d["addend"], bwd=True)
    _check("gcn2 data gradient", dxv, S.graph_conv_ref(d["dz"], d["WT"], d["P1"], None, d["addend"]), ex, 0.25)
    _check("gcn2 sums epilogue", sv, S.bwd_sums_ref(dxv, d["u"], d["fin"], nb, "any", bmask=d["bmask"]), ex, 0.125)


@pytest.mark.parametrize("family", FAMILIES)
def test_gcn2_extra_link_and_misaligned_addend(dev, family):
    N, T = 2, 32
    d, gt = _case(dev, N, T, family, kind="extra"), _graph(dev, "extra")
    assert gt[0].gen2 and not gt[0].gen3
    ex = d.ops.exact
    zv, _ = _gcn2(dev, d, gt, N, T, 0)
    _check("gcn2 forward, extra link", zv, S.graph_conv_ref(d["x"], d["W"], d["P0"], d["bias_cv"]), ex, 0.25)
    ref = S.graph_conv_ref(d["dz"], d["WT"], d["P1"], None, d["addend"])
    mis = _in(d.ops["addend"], dev, offset_bytes=4)
    assert mis.data_ptr() % 16 == 4
    for addend in (d["addend"], mis):
        dxv, _ = _gcn2(dev, d, gt, N, T, 1, addend=addend, stats=False)
        _check("gcn2 data gradient, extra link", dxv, ref, ex, 0.25)
    zmis = _out((N, 64, T, V), dev, offset_bytes=4)
    zv, _ = _gcn2(dev, d, gt, N, T, 0, stats=False, z=zmis)
    _check("gcn2 forward, misaligned output", zv, S.graph_conv_ref(d["x"], d["W"], d["P0"], d["bias_cv"]), ex, 0.25)


# ---- graph convolution, first generation ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("Vn,T", [(17, 22), (17, 23), (25, 15), (25, 16), (56, 6), (56, 7)])
def test_gcn_first_generation(dev, Vn, T, family):
    N = 2
    d, (gt, t) = _case(dev, N, T, family, kind="ring", Vn=Vn), _graph(dev, "ring", Vn)
    assert not gt.gen2
    ex = d.ops.exact
    F = min(384 // Vn, T)
    tiles = N * (-(-T // F))
    z, part = _out((N, 64, T, Vn), dev), _out((tiles, 64, 2), dev)
    _launch(dev, "p2r_stgcn_gcn_forward", N, T, Vn, K, gt.LkA_c, d["x"], d["W"], t["nbr_c"], d["coef0"], d["bias_cv"], z[1], part[1])
    zv, pv = _written(z, part)
    _check("gcn forward", zv, S.graph_conv_ref(d["x"], d["W"], d["P0"], d["bias_cv"]), ex, 0.25)
    _check("gcn forward statistics", pv, S.stats2_ref(zv, tiles, F), False)
    dx = _out((N, 64, T, Vn), dev)
    _launch(dev, "p2r_stgcn_gcn_forward", N, T, Vn, K, gt.LkA_r, d["dz"], d["WT"], t["nbr_r"], d["coef1"], None, dx[1], None)
    (dxv,) = _written(dx)
    _check("gcn data gradient", dxv, S.graph_conv_ref(d["dz"], d["WT"], d["P1"]), ex, 0.25)
    for nb in (3, 256):
        dw, cs = _out((nb, K, 64, 64), dev), _out((nb, 64, Vn), dev)
        _launch(dev, "p2r_stgcn_gcn_weight_grad", N, T, Vn, K, gt.LkA_r, d["dz"], d["x"], t["nbr_r"], d["coef1"], nb, dw[1], cs[1], 1)
        dwv, csv = _written(dw, cs)
        ref = S.weight_grad_ref(d["x"], d["dz"], d["P1"], nb)
        _check("gcn weight gradient", dwv.double().sum(0).float(), ref["dw"], ex, 0.5)
        cref = (ref["colsum"][0], S.gamma(ref["cols"]) * ref["colsum"][2], ref["colsum"][2])
        _check("gcn colsum", csv.double().sum(0).float(), cref, ex, 1.0)
        dc = _out((nb, d.tab[1]["ltot"], Vn), dev)
        _launch(dev, "p2r_stgcn_gcn_coef_grad", N, T, Vn, K, gt.LkA_r, d["dz"], d["x"], d["W"], t["nbr_r"], t["real_r"], nb, dc[1])
        (dcv,) = _written(dc)
        _check("gcn adjacency gradient", dcv.double().sum(0).float(),
               S.coef_grad_ref(d["x"], d["dz"], d["W"], d.tab, nb, F=F, first_gen=True), ex, 0.5)
        assert bool((dcv[:, t["gidx_r"] < 0] == 0).all()), "a padded slot got a gradient"


# ---- weight and adjacency gradients, third generation ---------------------------------------------------------------------------
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("n_blocks", [1, 3, 8, 16, 24, 256])
@pytest.mark.parametrize("N,T", [(3, 4), (4, 8), (5, 20)])            # 3, 8, 25 tiles of 4 frames
def test_gcn3_weight_grad(dev, N, T, n_blocks, family):
    d = _case(dev, N, T, family)
    dw, cs = _out((n_blocks, K, 64, 64), dev), _out((n_blocks, 64, V), dev)
    _launch(dev, "p2r_stgcn_gcn3_weight_grad", N, T, V, K, d.tab[1]["ltot"], d["x"], d["dz"], d["coef1"], n_blocks, dw[1], cs[1])
    dwv, csv = _written(dw, cs)
    ref = S.weight_grad_ref(d["x"], d["dz"], d["P1"], n_blocks)
    _check("gcn3 weight gradient", dwv.double().sum(0).float(), ref["dw"], d.ops.exact, 0.5)
    _check("gcn3 colsum", csv.double().sum(0).float(), ref["colsum"], d.ops.exact, 1.0)
    tiles = N * T // 4
    if n_blocks > tiles:            # the workgroups without a tile wrote zeros
        idle = [b for b in range(n_blocks) if not S.dw_tile_order(b, n_blocks, tiles)]
        assert idle and not bool(dwv[idle].any()) and not bool(csv[idle].any())
    # without the bias-table gradient: the same dW
    dw2 = _out((n_blocks, K, 64, 64), dev)
    _launch(dev, "p2r_stgcn_gcn3_weight_grad", N, T, V, K, d.tab[1]["ltot"], d["x"], d["dz"], d["coef1"], n_blocks, dw2[1], None)
    assert torch.equal(_written(dw2)[0], dwv)


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("n_blocks", [1, 3, 8, 256])
@pytest.mark.parametrize("N,T", [(1, 16), (3, 48)])
def test_gcn3_coef_grad(dev, N, T, n_blocks, family):
    d = _case(dev, N, T, family)
    ltot = d.tab[1]["ltot"]
    dc = _out((n_blocks, ltot, V), dev)
    _launch(dev, "p2r_stgcn_gcn3_coef_grad", N, T, V, K, ltot, d["x"], d["dz"], d["Wp"], n_blocks, dc[1])
    (dcv,) = _written(dc)
    _check("gcn3 adjacency gradient", dcv.double().sum(0).float(), S.coef_grad_ref(d["x"], d["dz"], d["W"], d.tab, n_blocks),
           d.ops.exact, 0.5)
    pad = (d.tab[1]["gidx"] < 0).to(dev)
    assert bool((dcv[:, pad] == 0).all()), "a padded slot got a gradient"
    if not d.ops.exact:             # real entries whose current coefficient is zero have their gradient
        zero_now = ((d["coef1"] == 0) & ~pad)
        assert bool(zero_now.any()) and bool((dcv.sum(0)[zero_now] != 0).all())


# ---- temporal convolution ---------------------------------------------------------------------------------------------------------
TFAMILIES = ["bounded", "exact", "gate"]


def _tconv_forward(dev, d, name, N, T, Vn, taps, stats_width, scale=True, bias=True, bwd=False, gate_w=False):
    """one launch of tconv / tconv2 / tconv3 -> (out, partials or None)"""
    g = "g" if gate_w else ""
    F = 16 if name != "p2r_stgcn_tconv_forward" else min(384 // Vn, T)
    nb = min(N * (-(-T // F)), 256)
    out = _out((N, 64, T, Vn), dev)
    part = _out((nb, 64, stats_width), dev) if stats_width else None
    if bwd:
        x, W = d["dout"], d["W3bp"]
    else:
        x = d["x"]
        W = d[f"W{taps}{g}"] if name == "p2r_stgcn_tconv_forward" else d[f"W{taps}{g}p"]
    args = [N, T, Vn, taps, x, d["scale"] if scale else None, d["shift"] if scale else None, W, d["bias"] if bias else None,
            out[1], part[1] if part else None, None]
    if name != "p2r_stgcn_tconv_forward":
        args += [d["x"] if bwd else None, d["fin"] if bwd else None]
    _launch(dev, name, *args)
    return _written(out, part)


def _tconv_generation(dev, d, name, N, T, Vn, family):
    ex, gate = d.ops.exact, family == "gate"
    g = "g" if gate else ""
    gen3 = name == "p2r_stgcn_tconv3_forward"
    F = 16 if name != "p2r_stgcn_tconv_forward" else min(384 // Vn, T)
    nb = min(N * (-(-T // F)), 256)
    tag = name[len("p2r_stgcn_"):-len("_forward")]
    for taps in (3, 1):
        ov, pv = _tconv_forward(dev, d, name, N, T, Vn, taps, 3 if gen3 else 2, gate_w=gate)
        _check(f"{tag} forward, {taps} tap(s)", ov, S.tconv_ref(d["x"], d["scale"], d["shift"], d[f"W{taps}{g}"], d["bias"]), ex, 0.25)
        if gen3 and not ex:
            _check(f"{tag} forward statistics", pv, S.stats3_ref(ov, nb), False)
        elif gen3:
            assert torch.equal(pv[:, :, 0], S.stats3_ref(ov, nb)[0][:, :, 0].float())
        else:
            _check(f"{tag} forward statistics", pv, S.stats2_ref(ov, nb, F), False)
    # no transform, no bias, no statistics: the plain data gradient; then with the sums epilogue
    ref = S.tconv_ref(d["dout"], None, None, d["W3b"])
    if name == "p2r_stgcn_tconv_forward":
        out = _out((N, 64, T, Vn), dev)
        _launch(dev, name, N, T, Vn, 3, d["dout"], None, None, d["W3b"], None, out[1], None, None)
        _check(f"{tag} data gradient", _written(out)[0], ref, ex, 0.5)
        return
    dhv, sv = _tconv_forward(dev, d, name, N, T, Vn, 3, 2, scale=False, bias=False, bwd=True)
    _check(f"{tag} data gradient", dhv, ref, ex, 0.5)
    sref = S.bwd_sums_ref(dhv, d["x"], d["fin"], nb, "tconv3" if gen3 else "any")
    if ex:                          # unit per channel: the gate / control channels hold z - mean = -m 2^-12
        special = list(S.GATE_CH + S.REV_CH)
        units = torch.full((64,), 0.125, dtype=torch.float64, device=dev)
        if gate:
            units[special] = 2.0 ** -14
        assert float((sref[2] / units[None, :, None]).max()) < S.TWO24
    _check(f"{tag} sums epilogue", sv, sref, ex)


@pytest.mark.parametrize("family", TFAMILIES)
@pytest.mark.parametrize("N,T", SHAPES)
def test_tconv3(dev, N, T, family):
    d = _case(dev, N, T, family)
    _tconv_generation(dev, d, "p2r_stgcn_tconv3_forward", N, T, V, family)
    gate = family == "gate"
    out = _out((N, 64, T, V), dev)
    _launch(dev, "p2r_stgcn_tconv3_forward_add", N, T, V, d["x"], d["scale"], d["shift"], d["W1gp" if gate else "W1p"], d["bias"],
            d["add_ct"], out[1])
    _check("tconv3 forward_add", _written(out)[0],
           S.tconv_ref(d["x"], d["scale"], d["shift"], d["W1g" if gate else "W1"], d["bias"], d["add_ct"]), d.ops.exact, 0.25)


def test_tconv3_more_tiles_than_workgroups(dev):
    N, T = 17, 256
    d = _case(dev, N, T, "gate", density=0.125)
    _tconv_generation(dev, d, "p2r_stgcn_tconv3_forward", N, T, V, "gate")
    _CASES.clear()


@pytest.mark.parametrize("family", TFAMILIES)
@pytest.mark.parametrize("N,T", SHAPES + [(2, 1), (2, 7), (2, 15), (2, 17), (2, 31), (2, 33)])
def test_tconv2(dev, N, T, family):
    _tconv_generation(dev, _case(dev, N, T, family), "p2r_stgcn_tconv2_forward", N, T, V, family)


@pytest.mark.parametrize("family", TFAMILIES)
@pytest.mark.parametrize("Vn,T", [(17, 22), (17, 23), (25, 15), (25, 16), (56, 6), (56, 7), (53, 1), (53, 8)])
def test_tconv_first_generation(dev, Vn, T, family):
    N = 2
    d = _case(dev, N, T, family, kind="ring" if Vn != V else "skeleton", Vn=Vn)
    _tconv_generation(dev, d, "p2r_stgcn_tconv_forward", N, T, Vn, family)


@pytest.mark.parametrize("family", TFAMILIES)
@pytest.mark.parametrize("n_blocks", [3, 16, 256])
@pytest.mark.parametrize("N,T", [(2, 8), (1, 6), (3, 20)])            # 4, 2 (the second ragged), 15 tiles of 4 frames
def test_tconv_weight_grad(dev, N, T, n_blocks, family):
    d = _case(dev, N, T, family)
    ex, gate = d.ops.exact, family == "gate"
    special = list(S.GATE_CH + S.REV_CH)

    def check_dw(stage, dwv, ref):
        got = dwv.double().sum(0).float()
        if gate:                    # two units: 2^-25 in the gate / control channels ci, 0.5 elsewhere
            assert S.exact_cap(ref["dw"][2][:, special], 2.0 ** -25) < S.TWO24
            keep = [c for c in range(64) if c not in special]
            assert S.exact_cap(ref["dw"][2][:, keep], 0.5) < S.TWO24
            assert bool((got[:, list(S.GATE_CH)] != 0).any()), "no open gate reached dW"
            _check(stage, got, ref["dw"], True)
        else:
            _check(stage, got, ref["dw"], ex, 0.5)

    for taps in (3, 1):
        dw, db = _out((n_blocks, 64, 64, taps), dev), _out((n_blocks, 64), dev)
        _launch(dev, "p2r_stgcn_tconv_weight_grad", N, T, V, taps, d["x"], d["scale"], d["shift"], d["dout"], n_blocks, dw[1], db[1])
        dwv, dbv = _written(dw, db)
        ref = S.tconv_weight_grad_ref(d["x"], d["scale"], d["shift"], d["dout"], taps, n_blocks)
        check_dw(f"tconv weight gradient, {taps} tap(s)", dwv, ref)
        _check("tconv bias gradient", dbv.double().sum(0).float(), ref["dbias"], ex, 1.0)
    # no transform (scale NULL), no bias gradient
    dw = _out((n_blocks, 64, 64, 3), dev)
    _launch(dev, "p2r_stgcn_tconv_weight_grad", N, T, V, 3, d["x"], None, None, d["dout"], n_blocks, dw[1], None)
    _check("tconv weight gradient, no transform", _written(dw)[0].double().sum(0).float(),
           S.tconv_weight_grad_ref(d["x"], None, None, d["dout"], 3, n_blocks)["dw"], ex and not gate, 0.5)
    # fused with the BatchNorm-backward apply pass
    dw, db, dz = _out((n_blocks, 64, 64, 3), dev), _out((n_blocks, 64), dev), _out((N, 64, T, V), dev)
    _launch(dev, "p2r_stgcn_tconv_weight_grad_dz", N, T, V, 3, d["x"], d["fin"], d["dout"], d["dh"], d["m12"], dz[1], n_blocks,
            dw[1], db[1])
    dwv, dbv, dzv = _written(dw, db, dz)
    ref = S.tconv_weight_grad_ref(d["x"], d["scale"], d["shift"], d["dout"], 3, n_blocks)
    check_dw("tconv weight gradient (fused dz)", dwv, ref)
    _check("tconv bias gradient", dbv.double().sum(0).float(), ref["dbias"], ex, 1.0)
    _check("tconv dz of the fused apply pass", dzv, S.bn_dz_ref(d["x"], d["fin"], d["dh"], d["m12"]), ex)


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("Vn,T,taps,F", [(25, 9, 3, 4), (20, 25, 1, 12), (20, 12, 1, 12), (57, 5, 3, 4), (64, 5, 1, 4)])
def test_tconv_weight_grad_other_joint_counts(dev, Vn, T, taps, F, family):
    """run-time joint count (V = 25; the largest: 57 with three taps, 64 with one) and the 12-frame single-tap instance of
    20 columns; one joint more is refused"""
    N, nb = 2, 3
    d = _case(dev, N, T, family, kind="ring", Vn=Vn)
    if Vn == 57:
        from pose2room_amd.p2rnet import tconv_op
        bn, conv = torch.nn.BatchNorm2d(64).to(dev), torch.nn.Conv2d(64, 64, (3, 1), (1, 1), (1, 0)).to(dev)
        assert tconv_op.supported(d["x"], bn, conv) and not tconv_op.supported(torch.zeros(1, 64, 4, 58, device=dev), bn, conv)
        wide = _case(dev, N, T, family, kind="ring", Vn=58)
        dw, db = _out((nb, 64, 64, 3), dev), _out((nb, 64), dev)
        _refused(dev, "p2r_stgcn_tconv_weight_grad", [N, T, 58, 3, wide["x"], wide["scale"], wide["shift"], wide["dout"], nb, dw[1],
                                                      db[1]], (dw, db))
    dw, db = _out((nb, 64, 64, taps), dev), _out((nb, 64), dev)
    _launch(dev, "p2r_stgcn_tconv_weight_grad", N, T, Vn, taps, d["x"], d["scale"], d["shift"], d["dout"], nb, dw[1], db[1])
    dwv, dbv = _written(dw, db)
    ref = S.tconv_weight_grad_ref(d["x"], d["scale"], d["shift"], d["dout"], taps, nb, F=F)
    _check(f"tconv weight gradient, V = {Vn}", dwv.double().sum(0).float(), ref["dw"], d.ops.exact, 0.5)
    _check("tconv bias gradient", dbv.double().sum(0).float(), ref["dbias"], d.ops.exact, 1.0)


@pytest.mark.parametrize("N,T", [(2, 32), (3, 7)])
def test_bn_backward_takes_the_fused_gate(dev, N, T):
    """p2r_bn_bwd_reduce / p2r_bn_bwd_apply with relu = 2 on the gate case: the recomputed gate is fmaf's"""
    d = _case(dev, N, T, "gate")
    fin, L = d["fin"], T * V
    mean, invstd = fin[0].contiguous(), fin[1].contiguous()
    part = _out((N * 64, 2), dev)
    _launch(dev, "p2r_bn_bwd_reduce", N, 64, L, d["dh"], None, d["x"], mean, invstd, 2, d["scale"], d["shift"], part[1])
    (pv,) = _written(part)
    f = fin.double()
    cv = lambda r: f[r][None, :, None, None]
    xd = d["x"].double()
    g = d["dh"].double() * (xd * cv(2) + cv(3) > 0)
    want = torch.stack([g.sum((2, 3)), (g * ((xd - cv(0)) * cv(1))).sum((2, 3))], -1).reshape(N * 64, 2)
    assert bool(g[:, list(S.GATE_CH)].any()) and not bool(g[:, list(S.REV_CH)].any())
    units = torch.full((64,), 0.125, dtype=torch.float64, device=dev)                               # the exact range
    units[list(S.GATE_CH + S.REV_CH)] = 2.0 ** -14
    assert float(((g * ((xd - cv(0)) * cv(1))).abs().sum((2, 3)) / units).max()) < S.TWO24
    _check("bn_bwd_reduce, gate case", pv, (want, torch.zeros_like(want)), True)
    dx = _out((N, 64, T, V), dev)
    m1, m2 = d["m12"][0].contiguous(), d["m12"][1].contiguous()
    _launch(dev, "p2r_bn_bwd_apply", N, 64, L, d["dh"], None, d["x"], mean, invstd, d["scale"], m1, m2, 2, d["scale"], d["shift"],
            dx[1], None)
    _check("bn_bwd_apply, gate case", _written(dx)[0], S.bn_dz_ref(d["x"], fin, d["dh"], d["m12"]), True)


# ---- refusals and empty batches ---------------------------------------------------------------------------------------------------
def test_refusals(dev):
    """every refusal the header lists: P2R_EINVAL and the outputs untouched.  Only arguments the entry point checks are
    varied; the tables and ltot are always the schedule's own."""
    N, T = 2, 32
    d = _case(dev, N, T, "bounded")
    ltc, ltr = d.tab[0]["ltot"], d.tab[1]["ltot"]
    z, part = _out((N, 64, T + 1, V), dev), _out((256, 64, 3), dev)
    zm = _out((N, 64, T, V), dev, offset_bytes=4)
    xm, um, mm = _in(d.ops["x"], dev, 4), _in(d.ops["u"], dev, 4), _in(d.ops["bmask"], dev, 2)

    def fwd(**k):       # form 1 with the row tables and their ltot, every other form value with the column tables
        row = k.get("form", 0) == 1
        return [k.get("N", N), k.get("T", T), k.get("V", V), k.get("K", K), ltr if row else ltc, k.get("form", 0),
                k.get("x", d["dz"] if row else d["x"]), d["WpT" if row else "Wp"], d["coef1" if row else "coef0"],
                None if row else d["bias_cv"], k.get("addend"), k.get("z", z[1]), k.get("part", part[1]), None, k.get("u"),
                k.get("mask"), k.get("fin")]

    for kw in (dict(T=T + 1), dict(T=24), dict(V=52), dict(K=10), dict(form=2), dict(N=-1), dict(x=xm), dict(z=zm[1]), dict(addend=xm),
               dict(form=1, u=d["u"]), dict(form=1, u=d["u"], mask=d["bmask"]), dict(form=1, mask=d["bmask"], fin=d["fin"]),
               dict(form=1, u=d["u"], mask=d["bmask"], fin=d["fin"], part=None),
               dict(form=0, u=d["u"], mask=d["bmask"], fin=d["fin"]),
               dict(form=1, u=um, mask=d["bmask"], fin=d["fin"]), dict(form=1, u=d["u"], mask=mm, fin=d["fin"])):
        _refused(dev, "p2r_stgcn_gcn3_forward", fwd(**kw), (z, part, zm))
    madd = lambda **k: [N, k.get("T", T), V, K, ltr, d["dz"], d["WpT"], d["coef1"], k.get("addend", d["addend"]),
                        k.get("amask", d["amask"]), z[1], k.get("part"), k.get("u"), None, None]
    for kw in (dict(amask=None), dict(addend=None), dict(amask=mm), dict(T=40), dict(u=d["u"], part=part[1])):
        _refused(dev, "p2r_stgcn_gcn3_data_gradient_masked_addend", madd(**kw), (z, part))
    dw, cs, dc = _out((3, K, 64, 64), dev), _out((3, 64, V), dev), _out((3, ltr, V), dev)
    wg = lambda **k: [k.get("N", N), k.get("T", T), k.get("V", V), k.get("K", K), ltr, k.get("x", d["x"]), k.get("dz", d["dz"]),
                      d["coef1"], k.get("nb", 3), dw[1], cs[1]]
    for kw in (dict(T=6), dict(T=30), dict(V=25), dict(K=12), dict(nb=0), dict(N=-1), dict(x=xm), dict(dz=xm)):
        _refused(dev, "p2r_stgcn_gcn3_weight_grad", wg(**kw), (dw, cs))
    cg = lambda **k: [k.get("N", N), k.get("T", T), k.get("V", V), k.get("K", K), ltr, d["x"], k.get("dz", d["dz"]), d["Wp"],
                      k.get("nb", 3), dc[1]]
    for kw in (dict(T=24), dict(T=36), dict(V=25), dict(K=12), dict(nb=0), dict(N=-1), dict(dz=xm)):
        _refused(dev, "p2r_stgcn_gcn3_coef_grad", cg(**kw), (dc,))
    out = _out((N, 64, T + 1, V), dev)
    t3 = lambda **k: [N, k.get("T", T), k.get("V", V), k.get("taps", 3), k.get("x", d["x"]), k.get("scale", d["scale"]),
                      k.get("shift", d["shift"]), d["W3p"], d["bias"], k.get("out", out[1]), k.get("part"), None, k.get("z"),
                      k.get("fin")]
    for kw in (dict(T=24), dict(T=T + 1), dict(V=25), dict(taps=2), dict(shift=None), dict(x=xm), dict(out=zm[1]),
               dict(scale=None, shift=None, z=d["x"]), dict(scale=None, shift=None, fin=d["fin"], part=part[1]),
               dict(scale=None, shift=None, z=d["x"], fin=d["fin"]), dict(z=d["x"], fin=d["fin"], part=part[1]),
               dict(scale=None, shift=None, z=xm, fin=d["fin"], part=part[1])):
        _refused(dev, "p2r_stgcn_tconv3_forward", t3(**kw), (out, part, zm))
    for kw in (dict(taps=2), dict(V=25), dict(shift=None), dict(scale=None, shift=None, z=d["x"])):
        _refused(dev, "p2r_stgcn_tconv2_forward", t3(**kw), (out, part))
    add = lambda **k: [N, k.get("T", T), V, d["x"], d["scale"], d["shift"], d["W1p"], d["bias"], k.get("add", d["add_ct"]), out[1]]
    for kw in (dict(add=None), dict(T=24)):
        _refused(dev, "p2r_stgcn_tconv3_forward_add", add(**kw), (out,))
    tw, tb, tz = _out((3, 64, 64, 3), dev), _out((3, 64), dev), _out((N, 64, T, V), dev)
    for kw in (dict(V=65), dict(taps=2), dict(nb=0)):
        _refused(dev, "p2r_stgcn_tconv_weight_grad", [N, T, kw.get("V", V), kw.get("taps", 3), d["x"], d["scale"], d["shift"], d["dout"],
                                                      kw.get("nb", 3), tw[1], tb[1]], (tw, tb))
    dzargs = lambda **k: [N, T, k.get("V", V), k.get("taps", 3), d["x"], k.get("fin", d["fin"]), d["dout"], k.get("dh", d["dh"]),
                          k.get("m12", d["m12"]), k.get("dz", tz[1]), k.get("nb", 3), tw[1], tb[1]]
    for kw in (dict(V=25), dict(taps=1), dict(nb=0), dict(fin=None), dict(dh=None), dict(m12=None), dict(dz=None)):
        _refused(dev, "p2r_stgcn_tconv_weight_grad_dz", dzargs(**kw), (tw, tb, tz))


def test_empty_batch(dev):
    """N == 0, as include/p2r_hip.h states it: P2R_OK, *n_partials = 0 and nothing launched where every output has a
    leading N; the [n_blocks][...] partials of the gradient entry points zero-filled -- their callers add the rows up.
    Every pointer is a real buffer (an empty tensor's would be NULL)."""
    T, nb = 32, 5
    d = _case(dev, 2, T, "bounded")
    gt, t = _graph(dev)
    ltc, ltr = d.tab[0]["ltot"], d.tab[1]["ltot"]
    x, dz = d["x"], d["dz"]
    z, part = _out((1, 64, T, V), dev), _out((4, 64, 3), dev)
    n = ctypes.c_int(7)
    byref = ctypes.byref(n)
    _launch(dev, "p2r_stgcn_gcn3_forward", 0, T, V, K, ltc, 0, x, d["Wp"], d["coef0"], d["bias_cv"], None, z[1], part[1], byref,
            None, None, None)
    assert n.value == 0
    n.value = 7
    work = _out(tuple(t["stream_c"].shape), dev, dtype=torch.int32)
    _launch(dev, "p2r_stgcn_gcn2_forward", 0, T, V, K, ltc, x, d["Wp"], d["coef0"], t["stream_c"], work[1], d["bias_cv"], None, z[1],
            part[1], byref, None, None, None)
    assert n.value == 0
    _launch(dev, "p2r_stgcn_gcn_forward", 0, T, V, K, gt.LkA_c, x, d["W"], t["nbr_c"], d["coef0"], d["bias_cv"], z[1], part[1])
    _launch(dev, "p2r_stgcn_gcn3_data_gradient_masked_addend", 0, T, V, K, ltr, dz, d["WpT"], d["coef1"], d["addend"], d["amask"],
            z[1], None, None, None, None)
    for name in ("p2r_stgcn_tconv3_forward", "p2r_stgcn_tconv2_forward"):
        n.value = 7
        _launch(dev, name, 0, T, V, 3, x, d["scale"], d["shift"], d["W3p"], d["bias"], z[1], part[1], byref, None, None)
        assert n.value == 0
    n.value = 7
    _launch(dev, "p2r_stgcn_tconv_forward", 0, T, V, 3, x, d["scale"], d["shift"], d["W3"], d["bias"], z[1], part[1], byref)
    assert n.value == 0
    _launch(dev, "p2r_stgcn_tconv3_forward_add", 0, T, V, x, d["scale"], d["shift"], d["W1p"], d["bias"], d["add_ct"], z[1])
    _untouched(z, part, work)

    def zeros(*pairs):
        for v in _written(*pairs):
            assert not bool(v.any())

    dw, cs, dc = _out((nb, K, 64, 64), dev), _out((nb, 64, V), dev), _out((nb, ltr, V), dev)
    _launch(dev, "p2r_stgcn_gcn3_weight_grad", 0, T, V, K, ltr, x, dz, d["coef1"], nb, dw[1], cs[1])
    _launch(dev, "p2r_stgcn_gcn3_coef_grad", 0, T, V, K, ltr, x, dz, d["Wp"], nb, dc[1])
    zeros(dw, cs, dc)
    dw, cs, dc = _out((nb, K, 64, 64), dev), _out((nb, 64, V), dev), _out((nb, ltr, V), dev)
    _launch(dev, "p2r_stgcn_gcn_weight_grad", 0, T, V, K, gt.LkA_r, dz, x, t["nbr_r"], d["coef1"], nb, dw[1], cs[1], 1)
    _launch(dev, "p2r_stgcn_gcn_coef_grad", 0, T, V, K, gt.LkA_r, dz, x, d["W"], t["nbr_r"], t["real_r"], nb, dc[1])
    zeros(dw, cs, dc)
    dw = _out((nb, K, 64, 64), dev)
    _launch(dev, "p2r_stgcn_gcn3_weight_grad", 0, T, V, K, ltr, x, dz, d["coef1"], nb, dw[1], None)
    zeros(dw)
    for taps in (3, 1):
        tw, tb = _out((nb, 64, 64, taps), dev), _out((nb, 64), dev)
        _launch(dev, "p2r_stgcn_tconv_weight_grad", 0, T, V, taps, x, d["scale"], d["shift"], d["dout"], nb, tw[1], tb[1])
        zeros(tw, tb)
    tw, tb = _out((nb, 64, 64, 3), dev), _out((nb, 64), dev)
    _launch(dev, "p2r_stgcn_tconv_weight_grad_dz", 0, T, V, 3, x, d["fin"], d["dout"], d["dh"], d["m12"], z[1], nb, tw[1], tb[1])
    zeros(tw, tb)
    _untouched(z)


# ---- op level -----------------------------------------------------------------------------------------------------------------------
P_SUM = 256         # gcn_op._N_BLOCKS / tconv_op._N_BLOCKS partial rows, added by p2r_sum_leading: at most P more additions


@pytest.mark.parametrize("family", FAMILIES)
def test_graph_conv_op(dev, family):
    """gcn_op.graph_conv: z and every gradient per element.  Composed bounds: bias_cv = b^T colsum(Aeff) is formed in fp32
    torch (V + K + 1 operations on |b| |Aeff|) and passes the kernel's 64 K + 1 additions; the partial rows pass 256 more
    additions in p2r_sum_leading; db = dbias_cv colsum(Aeff)^T and the bias share of dAeff, b_k^T dbias_cv, are fp32 matrix
    products over V and 64 terms of the bias-table gradient."""
    from pose2room_amd.p2rnet import gcn_op
    N, T = 2, 32
    d, (gt, _) = _case(dev, N, T, family), _graph(dev)
    ex = d.ops.exact
    g = S._gen("op", family)
    b = (S._ints(g, (K * 64,), 4, 1.0) / 4 if ex else torch.randn(K * 64, generator=g) * 0.1).to(dev)
    x, w, Aeff, go = d["x"], d["W"].reshape(K * 64, 64), _in(d.ops["Aeff"], dev), d["dz"]
    leaves = [t.clone().requires_grad_(True) for t in (x, w, b, Aeff)]
    z = gcn_op.graph_conv(leaves[0], leaves[1], leaves[2], leaves[3], gt)
    z.backward(go)
    torch.cuda.synchronize()
    gx, gw, gb, gA = (t.grad for t in leaves)
    # float64 chain on the same fp32 leaves
    Ad, bd = Aeff.double(), b.double().view(K, 64)
    pattern = (S.tables()["A"] != 0).to(dev)
    colsum, colabs = Ad.sum(1), Ad.abs().sum(1)                                  # [K][V]
    bias_cv, bias_mag = bd.t() @ colsum, bd.t().abs() @ colabs
    P0, P1 = S.planes_of(d.tab, 0, d["coef0"]), S.planes_of(d.tab, 1, d["coef1"])
    zr, _, zmag = S.graph_conv_ref(x, d["W"], P0)
    zref = (zr + bias_cv[None, :, None, :], S.gamma(S.K_GCN) * zmag + S.gamma(V + K + 1 + 64 * K + 1) * bias_mag[None, :, None, :])
    _check("op graph_conv z", z.detach(), zref, ex)
    _check("op graph_conv dx", gx, S.graph_conv_ref(go, d["WT"], P1), ex)
    wref = S.weight_grad_ref(x, go, P1, P_SUM)
    dwr, dwm = wref["dw"][0].transpose(1, 2).reshape(K * 64, 64), wref["dw"][2].transpose(1, 2).reshape(K * 64, 64)
    _check("op graph_conv dW", gw, (dwr, S.gamma(S.LMAX + 1 + wref["cols"] + P_SUM) * dwm), ex)
    cs, csm = wref["colsum"][0], wref["colsum"][2]                                # [64][V]: the bias-table gradient
    kcs = 2 + S.wg_tiles(N * T // 4, P_SUM) + P_SUM
    _check("op graph_conv db", gb, ((colsum @ cs.t()).reshape(-1), S.gamma(kcs + 2 * V + 1) * (colabs @ csm.t()).reshape(-1)), ex)
    cref = S.coef_grad_ref(x, go, d["W"], d.tab, P_SUM)
    gidx = d.tab[1]["gidx"].to(dev)
    dA = torch.zeros(K * V * V, dtype=torch.float64, device=dev)
    dAE = torch.zeros_like(dA)
    dA[gidx[gidx >= 0]] = cref[0][gidx >= 0]
    dAE[gidx[gidx >= 0]] = (cref[1] + S.gamma(P_SUM + 1) * cref[2])[gidx >= 0]
    share, share_mag = bd @ cs, bd.abs() @ csm                                    # [K][V(w)], the same for every source joint v
    dA = dA.view(K, V, V) + share[:, None, :]
    dAE = dAE.view(K, V, V) + S.gamma(kcs + 64 + 2) * share_mag[:, None, :] + S.U * dA.abs()
    _check("op graph_conv dAeff", gA, (dA, dAE), ex)        # dense: the bias share reaches every source joint
    assert bool((gA[pattern] != 0).any())


def _bn_conv(dev, d, taps, ex):
    bn = torch.nn.BatchNorm2d(64, eps=0.0 if ex else 1e-5).to(dev)
    conv = (torch.nn.Conv2d(64, 64, (3, 1), (1, 1), (1, 0)) if taps == 3 else torch.nn.Conv1d(64, 64, 1)).to(dev)
    fin = d["fin"]
    with torch.no_grad():
        W = d["W3" if taps == 3 else "W1"]                       # [taps][c][ci] -> the module's (c, ci, taps[, 1])
        conv.weight.copy_(W.permute(1, 2, 0).reshape(conv.weight.shape))
        conv.bias.copy_(d["bias"])
        if ex:          # evaluation mode: invstd = 1, scale = weight, shift = bias - mean scale, all dyadic
            bn.running_var.fill_(1.0)
            bn.running_mean.copy_(fin[0])
            bn.weight.copy_(fin[2])
            bn.bias.copy_(fin[3] + fin[0] * fin[2])
        else:
            bn.weight.uniform_(0.5, 1.5)
            bn.bias.uniform_(-0.5, 0.5)
    return bn, conv


@pytest.mark.parametrize("taps", [3, 1])
def test_bn_relu_tconv_op_exact(dev, taps):
    """tconv_op.bn_relu_tconv in evaluation mode on the exact case (with add_ct on the single tap): output and every
    gradient EQUAL the float64 chain"""
    from pose2room_amd.p2rnet import tconv_op
    N, T = 2, 32
    d = _case(dev, N, T, "exact")
    bn, conv = _bn_conv(dev, d, taps, True)
    bn.eval()
    z = d["x"].clone().requires_grad_(True)
    add = d["add_ct"].clone().requires_grad_(True) if taps == 1 else None
    out = tconv_op.bn_relu_tconv(z, bn, conv, add_ct=add)
    out.backward(d["dout"])
    torch.cuda.synchronize()
    scale, shift = bn.weight.detach(), (bn.bias - bn.running_mean * bn.weight).detach()
    assert torch.equal(shift, d["fin"][3]) and torch.equal(scale, d["fin"][2])
    W = d["W3" if taps == 3 else "W1"]
    _check("op bn_relu_tconv out (eval)", out.detach(), S.tconv_ref(d["x"], scale, shift, W, d["bias"], d["add_ct"] if add is not None else None), True)
    Wb = W.flip(0).transpose(1, 2)
    dh = S.tconv_ref(d["dout"], None, None, Wb)[0]
    gate = d["x"].double() * scale.double()[None, :, None, None] + shift.double()[None, :, None, None] > 0
    g = dh * gate
    zero = lambda t: torch.zeros_like(t)
    dzr = scale.double()[None, :, None, None] * g
    _check("op bn_relu_tconv dz (eval)", z.grad, (dzr, zero(dzr)), True)
    wr = S.tconv_weight_grad_ref(d["x"], scale, shift, d["dout"], taps, P_SUM)
    _check("op bn_relu_tconv dW (eval)", conv.weight.grad.reshape(64, 64, taps), (wr["dw"][0], zero(wr["dw"][0])), True)
    _check("op bn_relu_tconv dbias (eval)", conv.bias.grad, (wr["dbias"][0], zero(wr["dbias"][0])), True)
    xhat = d["x"].double() - bn.running_mean.double()[None, :, None, None]          # invstd = 1
    _check("op bn_relu_tconv dbeta (eval)", bn.bias.grad, (g.sum((0, 2, 3)), zero(g.sum((0, 2, 3)))), True)
    _check("op bn_relu_tconv dgamma (eval)", bn.weight.grad, ((g * xhat).sum((0, 2, 3)), zero(g.sum((0, 2, 3)))), True)
    if add is not None:
        da = d["dout"].double().sum(3)
        _check("op bn_relu_tconv dadd_ct (eval)", add.grad, (da, zero(da)), True)


@pytest.mark.parametrize("taps", [3, 1])
def test_bn_relu_tconv_op_train(dev, taps):
    """tconv_op.bn_relu_tconv in training mode on the bounded case (with add_ct on the single tap).  The op's own `fin`
    (p2r_bn_stats + p2r_bn_finalize, deterministic: recomputed here from a copy of the module) is the stage input; the
    bounds compose: E_dh of the data gradient enters the sums (with |xhat|), the sums of the workgroups and their
    p2r_bn_bwd_finalize (one rounding each) give dbeta, dgamma and m1, m2 = ./M (one more), and
    dz = k ((gq - m1) - xhat m2) takes E_dh, E_m1, |xhat| E_m2 on top of its own roundings."""
    import copy
    from pose2room_amd.p2rnet import tconv_op, bn_op
    N, T = 2, 32
    d = _case(dev, N, T, "bounded")
    bn, conv = _bn_conv(dev, d, taps, False)
    bn.train()
    x = d["x"]
    M = N * T * V
    fin = bn_op.finalize(bn_op._stats_partial(x.contiguous()), M, copy.deepcopy(bn))
    z = x.clone().requires_grad_(True)
    add = d["add_ct"].clone().requires_grad_(True) if taps == 1 else None
    out = tconv_op.bn_relu_tconv(z, bn, conv, add_ct=add)
    out.backward(d["dout"])
    torch.cuda.synchronize()
    W = d["W3" if taps == 3 else "W1"]
    scale, shift = fin[2].contiguous(), fin[3].contiguous()
    _check("op bn_relu_tconv out (train)", out.detach(), S.tconv_ref(x, scale, shift, W, d["bias"], d["add_ct"] if add is not None else None), False)
    dh, Edh, _ = S.tconv_ref(d["dout"], None, None, W.flip(0).transpose(1, 2))
    f = fin.double()
    cv = lambda r: f[r][None, :, None, None]
    xd = x.double()
    gate = xd * cv(2) + cv(3) > 0
    xh = (xd - cv(0)) * cv(1)
    g, Eg = dh * gate, Edh * gate
    nb = _nb16(N, T)
    _, Esum, _ = S.bwd_sums_ref(dh.float(), x, fin, nb, "tconv3")
    dbeta, dgamma = g.sum((0, 2, 3)), (g * xh).sum((0, 2, 3))
    # dh.float() above only sizes the stage bound; the rounding of dh to fp32 is inside E_dh
    Eb = Esum[..., 0].sum(0) + Eg.sum((0, 2, 3)) + S.gamma(2) * g.abs().sum((0, 2, 3))
    Eg2 = Esum[..., 1].sum(0) + (Eg * xh.abs()).sum((0, 2, 3)) + S.gamma(2) * (g * xh).abs().sum((0, 2, 3))
    _check("op bn_relu_tconv dbeta (train)", bn.bias.grad, (dbeta, Eb), False)
    _check("op bn_relu_tconv dgamma (train)", bn.weight.grad, (dgamma, Eg2), False)
    m1, m2 = dbeta / M, dgamma / M
    Em1, Em2 = Eb / M + S.U * m1.abs(), Eg2 / M + S.U * m2.abs()
    c4 = lambda v: v[None, :, None, None]
    k = cv(2)
    dzr = k * (g - c4(m1) - xh * c4(m2))
    Edz = (k.abs() * (Eg + c4(Em1) + xh.abs() * c4(Em2)) + S.gamma(3) * ((k * g).abs() + (k * c4(m1)).abs())
           + S.gamma(5) * (k * xh * c4(m2)).abs())
    _check("op bn_relu_tconv dz (train)", z.grad, (dzr, Edz), False)
    wr = S.tconv_weight_grad_ref(x, scale, shift, d["dout"], taps, P_SUM)
    cols = 4 * V * S.wg_tiles(N * T // 4, P_SUM)
    _check("op bn_relu_tconv dW (train)", conv.weight.grad.reshape(64, 64, taps), (wr["dw"][0], S.gamma(2 + cols + P_SUM) * wr["dw"][2]), False)
    _check("op bn_relu_tconv dbias (train)", conv.bias.grad, (wr["dbias"][0], S.gamma(9 + P_SUM) * wr["dbias"][2]), False)
    if add is not None:             # seed_op._rowsum over the joints: two accumulators, ceil(V / 2) + 2 operations
        da = d["dout"].double()
        _check("op bn_relu_tconv dadd_ct (train)", add.grad, (da.sum(3), S.gamma((V + 1) // 2 + 2) * da.abs().sum(3)), False)


def test_report_ratios():
    """prints the worst error / bound per stage of this session (the figures of the module docstring)"""
    for stage in sorted(RATIOS):
        print(f"RATIO {stage}: {RATIOS[stage]:.4f}" + (f"   error / largest entry {REL[stage]:.2e}" if stage in REL else ""))
