"""GPU: the split16 ST-GCN kernels (csrc/stgcn_gcn3h_body.h, stgcn_gcn3dwh.hip, stgcn_gcn3h_grad.hip, stgcn_tconvh.hip) and
p2r_stgcn_tconv_weight_grad_dz_amax against the float64 stage references of tests/split16_cases.py, through the C entry
points of include/p2r_hip.h on raw pointers (_lib.launch), every output poison-filled inside poisoned guard bands
(tests/memguard.py: nothing written outside, no element left unwritten), every stage on the kernel's OWN fp32 input.

Bounded families ('bounded': normal data; 'tail': frames differing by 2^20, for EVERY stage that takes a range word): per
element |got - ref| <= the bound derived in split16_cases' docstring.  Exact families (E0, EW, EX, and the gate case of
stgcn_cases in tconvh's forward and data-gradient forms): EQUAL to the float64 value, at every (N, T), n_blocks and with the
range word from p2r_absmax_bits or a hand-built word of the same exponent.  tests/test_split16_reference_cpu.py asserts the
families' conditions and shows the same `check` sensitive to thirteen named defects.

Sweep: gcn3h forward (with / without bias table, statistics, range word) and data gradient (plain, addend, masked addend
with bytes 0, 1, 2, 255) at (N, T) = (1, 16), (3, 48), (2, 64), (1, 256) and (17, 256) -- 272 tiles over 256 workgroups;
gcn3h_coef_grad at n_blocks 1, 2, 3, tiles, tiles + 1, 256; gcn3dwh at T = 4, 8, 20, 64 with the same n_blocks, with and
without the bias-table partials, each range word given or NULL; tconvh at T = 16 .. 128 (every chunk length, one and several
chunks) x N = 1, 3 in its three forms, *n_partials queried with out == NULL; range words at a power of two, one ulp below,
of an all-zero tensor, NULL, and from an unaligned view; p2r_stgcn_tconv_weight_grad_dz_amax against its plain twin; N == 0
and every refusal of the header.

Findings, fixed in this change (no wrong VALUE was found; no kernel arithmetic changed):
  * p2r_stgcn_tconvh_forward wrote *n_partials before it refused a misaligned Wh: the alignment is now checked with the
    other refusals (test_refusals).
  * p2r_stgcn_gcn3h_coef_grad took any n_blocks >= 1; like p2r_stgcn_gcn3h_weight_grad it now refuses more than 65535
    (test_refusals).
  * the header did not state the refusals, the T limits present in the launch code (2^19, 2^20, 2^31 bytes per sample) or
    N == 0 for the split entry points: stated now, N == 0 as the exact twins (test_empty_batch).

Worst observed error / derived bound per bounded stage over the whole sweep, all measured on one run of this file on an
MI355X (1 would be at the limit; "tail" = the heavy-tail family).  Every exact case -- 41 (stage, family) pairs, E0 / EW / EX
and the gate case, at every shape, n_blocks and word source above -- was bit for bit the float64 value.
  gcn3h: forward 0.0062 (tail 0.053; no range word 0.0052), (count, mean, M2) 0.019 (tail 0.018), data gradient 0.0015
        (tail 0.0015; no range word 0.0015; addend 0.0014 / 0.0012; masked addend 0.0018 / 0.0018)
  gcn3dwh: weight gradient 0.0026 (tail 0.0024; a word missing 0.0026), bias table 0.41 (tail 0.42: three additions and one
        per tile, little room by construction)
  gcn3h_coef_grad: 0.0003 (tail 0.0004)
  tconvh: forward 0.0075 (clamped activations 0.0071), (count, mean, M2) 0.0067, plain / data gradient 0.0060 (tail 0.012),
        sums epilogue 0.0084 (tail 0.042)
The bounds are running-error bounds over up to 2,126 accumulations, so ordinary data sits a factor 20 to 3,000 inside
them; what pins the two-part arithmetic to the last bit is the exact families.  The heavy-tail rows are where the
per-element bound bites: the forward's plain residual uses a tenth of its bound there, ten times the ordinary case.
As fractions of the reference's largest entry -- what the criterion of tests/test_split16_gpu.py (1.5 x the exact kernel's
figure + 2e-7) is a fraction of -- the worst errors against float64 on the same run were: gcn3h forward 1.3e-6 (tail
1.3e-6), data gradient 8.0e-7 (with addend 2.1e-7), gcn3dwh weight gradient 2.3e-6, bias table 2.1e-7, adjacency gradient
2.7e-7, tconvh 2.2e-7 .. 2.6e-7, statistics 2.0e-7 .. 2.9e-7.  The 2e-7 floor alone is 0.09 to 1.0 times these errors, so
the old criterion was carried by its 1.5 x term: with the exact kernels' worst figures recorded in
tests/test_stgcn_sweep_gpu.py (graph conv 2.1e-6, weight gradient 2.6e-6, temporal conv 6.5e-7; other data, so indicative
only) it admitted 3.4e-6, 4.1e-6 and 1.2e-6: a headroom of 2.6 (forward), 4.2 (data gradient), 1.8 (weight gradient) and
4.5 (temporal conv) over the errors observed here -- per tensor, not per element: an element 2^-20 of the maximum was
allowed an error 2^20 times its size, where the bounds above hold it to its own terms.  (The exact kernels were not run by
this file; those four quotients are not measurements of this run.)
"""
import ctypes

import pytest
import torch

from tests import split16_cases as H
from tests import stgcn_cases as S
from tests.bn_cases import check_amax
from tests.test_stgcn_sweep_gpu import _in, _launch, _out, _refused, _untouched, _written

pytestmark = pytest.mark.gpu

V, K, C = 53, H.K, H.C
LTC, LTR = 47, 62
GCN_SHAPES = [(1, 16), (3, 48), (2, 64), (1, 256)]
FAMILIES = ["bounded", "tail", "E0", "EW", "EX"]
UNITS = {"gcn": {"E0": 0.25, "EW": 2.0 ** -15, "EX": 2.0 ** -15}, "tconvh": {"E0": 0.25, "EW": 2.0 ** -15, "EX": 2.0 ** -15},
         "dwh": {"E0": 0.5, "EW": 2.0 ** -14, "EX": 2.0 ** -14}, "dcoef": {"E0": 0.5, "EW": 2.0 ** -14, "EX": 2.0 ** -14}}

RATIOS = {}     # stage -> worst error / bound of this session
REL = {}        # stage -> worst error / largest entry of the reference (what the old criterion's 2e-7 is a fraction of)
EXACT_STAGES = set()


def _check(stage, got, ref, fam, kind=None):
    exact = fam not in ("bounded", "tail")
    if exact and kind is not None and fam in UNITS[kind]:
        cap = S.exact_cap(ref[2], UNITS[kind][fam]) * (1 + 2.0 ** -9)
        assert cap < S.TWO24, f"{stage} {fam}: {cap:.3g} units: the case leaves the exact range"
    r = H.check(got, ref, exact, f"{stage} [{fam}]")
    if exact:
        EXACT_STAGES.add(f"{stage} [{fam}]")
        return
    key = stage + (" (tail)" if fam == "tail" else "")
    RATIOS[key] = max(RATIOS.get(key, 0.0), float(r))
    if ref[0].numel():
        rel = float((got.double() - ref[0]).abs().max() / ref[0].abs().max().clamp_min(1e-300))
        REL[key] = max(REL.get(key, 0.0), rel)


def _host_family(fam):
    return "bounded" if fam in ("bounded", "tail") else ("gate" if fam == "gate" else "exact")


class Dev:
    """the operands of one case on the device, each inside a zero halo, made on first use; derived keys: 'sp<form>:<W>'
    (plane pairs), 'sd:<W>' (adjacency-gradient planes), 'st:<W3>' (taps) -> (fp16 operand, winv), 'T:<W>' transposed planes"""

    def __init__(self, ops, dev):
        self.ops, self.dev, self._c, self.tab = ops, dev, {}, ops.tab

    def __getitem__(self, key):
        if key not in self._c:
            from pose2room_amd.p2rnet import gcn_op, tconv_op
            if key.startswith("sp"):
                form = int(key[2])
                t = gcn_op.split_planes(self[key[4:]], H.PAIRS[form], transposed=form == 1)
            elif key.startswith("sd:"):
                t = gcn_op.split_planes_coef_grad(self[key[3:]])
            elif key.startswith("st:"):
                t = tconv_op.split_taps(self[key[3:]])
            elif key.startswith("T:"):
                t = self[key[2:]].transpose(1, 2).contiguous()
            elif key.startswith("P"):
                t = S.planes_of(self.tab, int(key[1]), self[key[3:]])
            elif key in ("scale", "shift", "scale1", "shift1"):
                t = self["fin1" if key.endswith("1") else "fin"][2 if key.startswith("scale") else 3].contiguous()
            else:
                t = _in(self.ops[key], self.dev)
            self._c[key] = t
        return self._c[key]


_CASES = {}


def _case(dev, N, T, fam, **kw):
    key = (N, T, _host_family(fam), tuple(sorted(kw.items())))
    if key not in _CASES:
        _CASES[key] = Dev(H.Operands(N, T, family=_host_family(fam), **kw), dev)
    return _CASES[key]


def _word(dev, t):
    """the range word of t from p2r_absmax_bits -> (device word, its value)"""
    w = torch.full((1,), 0x5A5A5A5A, dtype=torch.int32, device=dev)
    _launch(dev, "p2r_absmax_bits", t.numel(), t, w)
    return w, int(w.item()) & 0xFFFFFFFF


def _hand(dev, bits):
    return torch.tensor([bits if bits < 1 << 31 else bits - (1 << 32)], dtype=torch.int32, device=dev), bits


def _words(dev, t, fam):
    """the word sources a family is run with"""
    own = _word(dev, t)
    assert own[1] == H.amax_word(t)
    return [own] if fam in ("bounded", "tail") else [own, _hand(dev, H.same_exponent_word(own[1]))]


def test_schedule_pairs_and_tables(dev):
    from pose2room_amd.p2rnet import gcn_op
    gt = gcn_op.GraphTables(S.tables()["A"].numpy())
    assert gt.gen3h and [tuple(p) for p in gt.pairs_c] == H.PAIRS[0] and [tuple(p) for p in gt.pairs_r] == H.PAIRS[1]
    assert S.tables()[0]["ltot"] == LTC and S.tables()[1]["ltot"] == LTR


# ---- graph conv forward / data gradient -------------------------------------------------------------------------------------------
def _gcn3h_all(dev, d, N, T, fam, variants=True):
    nb = min(N * (T // 16), 256)
    shape = (N, 64, T, V)
    xk, wk, ck = H.gcn_keys(0, fam)
    x, W, coef = d[xk], d[wk], d[ck]
    wh, winv = d["sp0:" + wk]
    P = d["P0:" + ck]
    first = None
    for wd, wv in _words(dev, x, fam):
        z, part = _out(shape, dev), _out((nb, 64, 3), dev)
        n = ctypes.c_int(-1)
        _launch(dev, "p2r_stgcn_gcn3h_forward", N, T, V, K, LTC, x, wh, winv, coef, d["bias_cv"], z[1], part[1], ctypes.byref(n), wd)
        zv, pv = _written(z, part)
        assert n.value == nb
        _check("gcn3h forward", zv, H.gcnh_ref(x, W, P, wv, False, d["bias_cv"]), fam, "gcn")
        if fam in ("bounded", "tail"):
            _check("gcn3h forward statistics", pv, S.stats3_ref(zv, nb), fam)
        else:
            assert torch.equal(pv[:, :, 0], S.stats3_ref(zv, nb)[0][:, :, 0].float())
        first = zv if first is None else first
        assert torch.equal(zv, first)                       # either word source: the same bits
    if variants:
        z = _out(shape, dev)                                # no bias table, no statistics
        _launch(dev, "p2r_stgcn_gcn3h_forward", N, T, V, K, LTC, x, wh, winv, coef, None, z[1], None, None, _word(dev, x)[0])
        _check("gcn3h forward", _written(z)[0], H.gcnh_ref(x, W, P, H.amax_word(x), False), fam, "gcn")
        if fam != "tail":                                   # x_amax == NULL: scale 1
            z = _out(shape, dev)
            _launch(dev, "p2r_stgcn_gcn3h_forward", N, T, V, K, LTC, x, wh, winv, coef, d["bias_cv"], z[1], None, None, None)
            _check("gcn3h forward, no range word", _written(z)[0], H.gcnh_ref(x, W, P, None, False, d["bias_cv"]), fam, "gcn")
    # data gradient
    xk, wk, ck = H.gcn_keys(1, fam)
    if variants and fam == "bounded":                       # dz_amax == NULL: scale 1
        dx = _out(shape, dev)
        _launch(dev, "p2r_stgcn_gcn3h_data_gradient", N, T, V, K, LTR, d[xk], d["sp1:" + wk][0], d["sp1:" + wk][1], d[ck], None, None,
                dx[1], None)
        _check("gcn3h data gradient, no range word", _written(dx)[0], H.gcnh_ref(d[xk], d["T:" + wk], d["P1:" + ck], None, True), fam)
    dz, WT, coef = d[xk], d["T:" + wk], d[ck]
    wh, winv = d["sp1:" + wk]
    P = d["P1:" + ck]
    for wd, wv in _words(dev, dz, fam):
        for addend, mask in ((None, None), (d["addend"], None), (d["addend"], d["amask"])) if variants else ((d["addend"], d["amask"]),):
            dx = _out(shape, dev)
            _launch(dev, "p2r_stgcn_gcn3h_data_gradient", N, T, V, K, LTR, dz, wh, winv, coef, addend, mask, dx[1], wd)
            stage = "gcn3h data gradient" + (", masked addend" if mask is not None else (", addend" if addend is not None else ""))
            _check(stage, _written(dx)[0], H.gcnh_ref(dz, WT, P, wv, True, None, addend, mask), fam, "gcn")


@pytest.mark.parametrize("fam", FAMILIES)
@pytest.mark.parametrize("N,T", GCN_SHAPES)
def test_gcn3h_forward_and_data_gradient(dev, N, T, fam):
    _gcn3h_all(dev, _case(dev, N, T, fam), N, T, fam)


@pytest.mark.parametrize("fam", FAMILIES)
def test_gcn3h_more_tiles_than_workgroups(dev, fam):
    """(17, 256): 272 tiles over 256 workgroups: workgroups 0 .. 15 walk a second tile, in another sample"""
    N, T = 17, 256
    _gcn3h_all(dev, _case(dev, N, T, fam), N, T, fam, variants=False)
    _CASES.clear()


# ---- adjacency gradient -----------------------------------------------------------------------------------------------------------
def _nbs(tiles):
    return sorted({1, 2, 3, tiles, tiles + 1, 256})


def _dcoef(dev, d, N, T, fam, nbs):
    xk, wk = H.dcoef_keys(fam)
    x, dz, W = d[xk], d["dz"], d[wk]
    wd_, winv = d["sd:" + wk]
    pad = (d.tab[1]["gidx"] < 0).to(dev)
    for nb in nbs:
        for word, wv in _words(dev, x, fam) + ([(None, None)] if fam == "bounded" else []):
            dc = _out((nb, LTR, V), dev)
            _launch(dev, "p2r_stgcn_gcn3h_coef_grad", N, T, V, K, LTR, x, dz, wd_, winv, nb, dc[1], word)
            (dcv,) = _written(dc)
            _check("gcn3h adjacency gradient", dcv.double().sum(0).float(), H.dcoefh_ref(x, dz, W, d.tab, nb, wv), fam, "dcoef")
            assert bool((dcv[:, pad] == 0).all()), "a padded slot got a gradient"
            tiles = N * (T // 16)
            if nb > tiles:
                assert not bool(dcv[tiles:].any()), "a workgroup without a tile left something else than zeros"


@pytest.mark.parametrize("fam", FAMILIES)
@pytest.mark.parametrize("N,T", [(1, 16), (3, 48)])
def test_gcn3h_coef_grad(dev, N, T, fam):
    _dcoef(dev, _case(dev, N, T, fam, density=1 / 16), N, T, fam, _nbs(N * (T // 16)))


@pytest.mark.parametrize("fam", FAMILIES)
@pytest.mark.parametrize("N,T", [(2, 64), (1, 256)])
def test_gcn3h_coef_grad_longer_sequences(dev, N, T, fam):
    _dcoef(dev, _case(dev, N, T, fam, density=1 / 16), N, T, fam, [3, 256])


# ---- weight gradient --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fam", FAMILIES)
@pytest.mark.parametrize("T", [4, 8, 20, 64])
def test_gcn3dwh(dev, T, fam):
    N = 3
    d = _case(dev, N, T, fam)
    tiles = N * (T // 4)
    xk, zk, ck = H.dwh_keys(fam)
    x, dz, coef = d[xk], d[zk], d[ck]
    P = d["P1:" + ck]
    (xw, xv), (zw, zv) = _word(dev, x), _word(dev, dz)
    for nb in _nbs(tiles):
        dw, cb = _out((nb, K, 64, 64), dev), _out((nb, 64, V), dev)
        _launch(dev, "p2r_stgcn_gcn3h_weight_grad", N, T, V, K, LTR, x, dz, coef, nb, dw[1], cb[1], xw, zw)
        dwv, cbv = _written(dw, cb)
        ref = H.dwh_ref(x, dz, P, nb, xv, zv)
        _check("gcn3dwh weight gradient", dwv.double().sum(0).float(), ref["dw"], fam, "dwh")
        _check("gcn3dwh bias table", cbv.double().sum(0).float(), ref["colsum"], fam)
        if nb > tiles:
            idle = [b for b in range(nb) if not S.dw_tile_order(b, nb, tiles)]
            assert idle and not bool(dwv[idle].any()) and not bool(cbv[idle].any())
        dw2 = _out((nb, K, 64, 64), dev)                    # without the bias-table partials: the same dW
        _launch(dev, "p2r_stgcn_gcn3h_weight_grad", N, T, V, K, LTR, x, dz, coef, nb, dw2[1], None, xw, zw)
        assert torch.equal(_written(dw2)[0], dwv)
    if fam != "tail":                                       # each word given or NULL; hand-built words of the same exponent
        combos = [(None, None), (xw, None), (None, zw)]
        for a, b in combos:
            dw = _out((3, K, 64, 64), dev)
            _launch(dev, "p2r_stgcn_gcn3h_weight_grad", N, T, V, K, LTR, x, dz, coef, 3, dw[1], None, a, b)
            ref = H.dwh_ref(x, dz, P, 3, xv if a is not None else None, zv if b is not None else None)
            _check("gcn3dwh weight gradient, a word missing", _written(dw)[0].double().sum(0).float(), ref["dw"], fam, "dwh")
    if fam not in ("bounded", "tail"):
        dw = _out((3, K, 64, 64), dev)
        _launch(dev, "p2r_stgcn_gcn3h_weight_grad", N, T, V, K, LTR, x, dz, coef, 3, dw[1], None,
                _hand(dev, H.same_exponent_word(xv))[0], _hand(dev, H.same_exponent_word(zv))[0])
        _check("gcn3dwh weight gradient", _written(dw)[0].double().sum(0).float(), H.dwh_ref(x, dz, P, 3, xv, zv)["dw"], fam, "dwh")


# ---- temporal conv ----------------------------------------------------------------------------------------------------------------
def _tconvh_forms(dev, d, N, T, fam):
    FC = H.chunk_of(T)
    nb = N * (T // FC)
    shape = (N, 64, T, V)
    gate = fam == "gate"
    for form in ("forward", "plain", "bwd"):
        if (gate and form == "plain") or (fam == "tail" and form == "forward"):
            continue                                        # no gate in the plain form; the forward form takes no range word
        xk, wk, fk = H.tconvh_keys(form, fam)
        x, W3, fin = d[xk], d[wk], d[fk]
        wh, winv = d["st:" + wk]
        one = "1" if fk == "fin1" else ""
        n = ctypes.c_int(-1)
        if form == "forward":
            _launch(dev, "p2r_stgcn_tconvh_forward", N, T, V, x, d["scale" + one], d["shift" + one], wh, winv, d["bias"], None, None,
                    ctypes.byref(n), None, None, None)
            assert n.value == nb                            # the header's formula, queried with out == NULL
            out, part = _out(shape, dev), _out((nb, 64, 3), dev)
            _launch(dev, "p2r_stgcn_tconvh_forward", N, T, V, x, d["scale" + one], d["shift" + one], wh, winv, d["bias"], out[1], part[1],
                    ctypes.byref(n), None, None, None)
            ov, pv = _written(out, part)
            assert n.value == nb
            _check("tconvh forward", ov, H.tconvh_ref(x, d["scale" + one], d["shift" + one], W3, None, d["bias"]), fam, "tconvh")
            if fam == "bounded":
                _check("tconvh forward statistics", pv, H.stats_chunk_ref(ov, FC), fam)
            else:
                assert bool((pv[:, :, 0] == FC * V).all())
            continue
        for wd, wv in _words(dev, x, fam) + ([(None, None)] if fam == "bounded" else []):
            ref = H.tconvh_ref(x, None, None, W3, wv)
            if form == "plain":
                out = _out(shape, dev)
                _launch(dev, "p2r_stgcn_tconvh_forward", N, T, V, x, None, None, wh, winv, None, out[1], None, None, None, None, wd)
                _check("tconvh plain", _written(out)[0], ref, fam, "tconvh")
            else:
                out, part = _out(shape, dev), _out((nb, 64, 2), dev)
                _launch(dev, "p2r_stgcn_tconvh_forward", N, T, V, x, None, None, wh, winv, None, out[1], part[1], ctypes.byref(n),
                        d["x"], fin, wd)
                ov, pv = _written(out, part)
                assert n.value == nb
                _check("tconvh data gradient", ov, ref, fam, "tconvh")
                sref = H.bwd_chunk_ref(ov, d["x"], fin, FC)
                if fam in ("E0", "gate"):                   # the sums of the other exact families leave the exact range
                    units = torch.full((64,), 0.125, dtype=torch.float64, device=dev)
                    if gate:
                        units[list(S.GATE_CH + S.REV_CH)] = 2.0 ** -14
                    assert float((sref[2] / units[None, :, None]).max()) < S.TWO24
                _check("tconvh sums epilogue", pv, sref, fam if fam in ("E0", "gate", "tail") else "bounded")


@pytest.mark.parametrize("fam", FAMILIES + ["gate"])
@pytest.mark.parametrize("N", [1, 3])
@pytest.mark.parametrize("T", [16, 32, 48, 64, 80, 96, 128])
def test_tconvh(dev, T, N, fam):
    _tconvh_forms(dev, _case(dev, N, T, fam), N, T, fam)


def test_tconvh_takes_the_fused_gate_and_clamps(dev):
    """the gate case tells fmaf from a product and an addition; activations beyond 65504 are clamped, not infinite"""
    N, T = 2, 32
    d = _case(dev, N, T, "gate")
    fused, unfused = S.gate_forms(d["x"], d["scale"], d["shift"])
    assert bool(((fused > 0) != (unfused > 0)).any())
    d = _case(dev, 1, 16, "bounded")
    x = _in(d.ops["xbig"], dev)
    wh, winv = d["st:W3"]
    out = _out((1, 64, 16, V), dev)
    _launch(dev, "p2r_stgcn_tconvh_forward", 1, 16, V, x, d["scale"], d["shift"], wh, winv, d["bias"], out[1], None, None, None, None, None)
    assert float(H.clamp_h(x, d["scale"], d["shift"]).max()) == H.H16_MAX
    _check("tconvh forward, clamped", _written(out)[0], H.tconvh_ref(x, d["scale"], d["shift"], d["W3"], None, d["bias"]), "bounded")


# ---- range words ------------------------------------------------------------------------------------------------------------------
def test_range_words(dev):
    """maximum exactly a power of two and one ulp below (the scale changes by 2 between them), an all-zero tensor (word 0,
    scale 1: z is the bias table exactly), a word from p2r_absmax_bits on an unaligned view"""
    N, T = 1, 16
    d = _case(dev, N, T, "E0")
    shape = (N, 64, T, V)
    wh, winv = d["sp0:W"]
    P = d["P0:coef0"]
    results = []
    for top in (4.0, 4.0 - 2.0 ** -22):
        x = d.ops["x"].clone()
        x[0, 5, 3, 7] = top
        x = _in(x, dev)
        wd, wv = _word(dev, x)
        assert wv == H.bits_of(top)
        z = _out(shape, dev)
        _launch(dev, "p2r_stgcn_gcn3h_forward", N, T, V, K, LTC, x, wh, winv, d["coef0"], d["bias_cv"], z[1], None, None, wd)
        results.append(H.word_scale(wv))
        _check(f"gcn3h forward, maximum {top!r}", _written(z)[0], H.gcnh_ref(x, d["W"], P, wv, False, d["bias_cv"]), "bounded")
    assert results[1] == 2 * results[0]
    zero = _in(torch.zeros(shape), dev)
    wd, wv = _word(dev, zero)
    assert wv == 0
    z = _out(shape, dev)
    _launch(dev, "p2r_stgcn_gcn3h_forward", N, T, V, K, LTC, zero, wh, winv, d["coef0"], d["bias_cv"], z[1], None, None, wd)
    assert torch.equal(_written(z)[0], d["bias_cv"][None, :, None, :].expand(shape))
    whr, winvr = d["sp1:W"]
    dx = _out(shape, dev)
    _launch(dev, "p2r_stgcn_gcn3h_data_gradient", N, T, V, K, LTR, zero, whr, winvr, d["coef1"], None, None, dx[1], wd)
    assert not bool(_written(dx)[0].any())
    buf = _in(torch.cat([torch.tensor([9.0]), d.ops["dout"].reshape(-1)]), dev)
    view = buf[1:]
    assert view.data_ptr() % 16 == 4
    wd, wv = _word(dev, view)
    assert wv == H.amax_word(d.ops["dout"])
    th, tinv = d["st:W3"]
    out = _out(shape, dev)
    _launch(dev, "p2r_stgcn_tconvh_forward", N, T, V, d["dout"], None, None, th, tinv, None, out[1], None, None, None, None, wd)
    _check("tconvh plain, word of an unaligned view", _written(out)[0], H.tconvh_ref(d["dout"], None, None, d["W3"], wv), "E0", "tconvh")


@pytest.mark.parametrize("family", ["bounded", "exact", "gate"])
def test_tconv_weight_grad_dz_amax(dev, family):
    """its dz, dW and dbias are the plain entry point's bit for bit; the word is max |dz|; a second call on smaller data
    leaves the smaller word; N == 0 leaves 0"""
    N, T, nb = 2, 20, 3
    d = _case(dev, N, T, family if family != "exact" else "E0")
    outs = {}
    word = torch.full((1,), 0x7F7FFFFF, dtype=torch.int32, device=dev)
    for name in ("p2r_stgcn_tconv_weight_grad_dz", "p2r_stgcn_tconv_weight_grad_dz_amax"):
        dw, db, dz = _out((nb, 64, 64, 3), dev), _out((nb, 64), dev), _out((N, 64, T, V), dev)
        tail_ = (word,) if name.endswith("amax") else ()
        _launch(dev, name, N, T, V, 3, d["x"], d["fin"], d["dout"], d["dh"], d["m12"], dz[1], nb, dw[1], db[1], *tail_)
        outs[name] = _written(dw, db, dz)
    for a, b in zip(*outs.values()):
        assert torch.equal(a, b)
    dzv = outs["p2r_stgcn_tconv_weight_grad_dz_amax"][2]
    check_amax(int(word.item()) & 0xFFFFFFFF, dzv.cpu(), "dz_amax")
    small = _in(d.ops["dh"] * 0.125, dev)
    m0 = torch.zeros_like(d["m12"])
    dw, db, dz = _out((nb, 64, 64, 3), dev), _out((nb, 64), dev), _out((N, 64, T, V), dev)
    _launch(dev, "p2r_stgcn_tconv_weight_grad_dz_amax", N, T, V, 3, d["x"], d["fin"], d["dout"], small, m0, dz[1], nb, dw[1], db[1], word)
    dz2 = _written(dw, db, dz)[2]
    assert float(dz2.abs().max()) < float(dzv.abs().max())
    check_amax(int(word.item()) & 0xFFFFFFFF, dz2.cpu(), "dz_amax, second call on smaller data")
    dw, db, dz = _out((nb, 64, 64, 3), dev), _out((nb, 64), dev), _out((1, 64, T, V), dev)
    _launch(dev, "p2r_stgcn_tconv_weight_grad_dz_amax", 0, T, V, 3, d["x"], d["fin"], d["dout"], d["dh"], d["m12"], dz[1], nb, dw[1],
            db[1], word)
    for v in _written(dw, db):
        assert not bool(v.any())
    _untouched(dz)
    assert int(word.item()) == 0
    _refused(dev, "p2r_stgcn_tconv_weight_grad_dz_amax", [N, T, V, 3, d["x"], d["fin"], d["dout"], d["dh"], d["m12"], dz[1], nb, dw[1],
                                                          db[1], None], (dz,))


# ---- N == 0 and refusals ----------------------------------------------------------------------------------------------------------
def test_empty_batch(dev):
    """N == 0 as include/p2r_hip.h states it for the split entry points: P2R_OK, *n_partials = 0 and nothing written by the
    forwards; the [n_blocks][...] partial rows of the gradient entry points zero-filled, as their exact twins"""
    T, nb = 32, 5
    d = _case(dev, 2, T, "bounded")
    x, dz = d["x"], d["dz"]
    xw = _word(dev, x)[0]
    z, part = _out((1, 64, T, V), dev), _out((4, 64, 3), dev)
    n = ctypes.c_int(7)
    wh, winv = d["sp0:W"]
    _launch(dev, "p2r_stgcn_gcn3h_forward", 0, T, V, K, LTC, x, wh, winv, d["coef0"], d["bias_cv"], z[1], part[1], ctypes.byref(n), xw)
    assert n.value == 0
    wh, winv = d["sp1:W"]
    _launch(dev, "p2r_stgcn_gcn3h_data_gradient", 0, T, V, K, LTR, dz, wh, winv, d["coef1"], d["addend"], d["amask"], z[1], xw)
    th, tinv = d["st:W3"]
    for args in ((d["scale"], d["shift"], th, tinv, d["bias"], z[1], part[1], ctypes.byref(n), None, None, None),
                 (None, None, th, tinv, None, z[1], part[1], ctypes.byref(n), d["x"], d["fin"], xw)):
        n.value = 7
        _launch(dev, "p2r_stgcn_tconvh_forward", 0, T, V, x, *args)
        assert n.value == 0
    _untouched(z, part)
    dw, cb, dc = _out((nb, K, 64, 64), dev), _out((nb, 64, V), dev), _out((nb, LTR, V), dev)
    _launch(dev, "p2r_stgcn_gcn3h_weight_grad", 0, T, V, K, LTR, x, dz, d["coef1"], nb, dw[1], cb[1], xw, xw)
    wd_, dinv = d["sd:W"]
    _launch(dev, "p2r_stgcn_gcn3h_coef_grad", 0, T, V, K, LTR, x, dz, wd_, dinv, nb, dc[1], xw)
    for v in _written(dw, cb, dc):
        assert not bool(v.any())
    dw = _out((nb, K, 64, 64), dev)
    _launch(dev, "p2r_stgcn_gcn3h_weight_grad", 0, T, V, K, LTR, x, dz, d["coef1"], nb, dw[1], None, None, None)
    assert not bool(_written(dw)[0].any())


def test_refusals(dev):
    """every refusal of the header and of the launch code: P2R_EINVAL, every poisoned output untouched, *n_partials as it
    was.  Only arguments the entry point checks are varied."""
    N, T = 2, 32
    d = _case(dev, N, T, "bounded")
    x, dz = d["x"], d["dz"]
    xw = _word(dev, x)[0]
    shape = (N, 64, T, V)
    z, part = _out((N, 64, T + 1, V), dev), _out((256, 64, 3), dev)
    zm = _out(shape, dev, offset_bytes=4)
    xm, mm = _in(d.ops["x"], dev, 4), _in(d.ops["amask"], dev, 2)
    n = ctypes.c_int(7)

    def misaligned(pair):
        buf = torch.zeros(pair[0].numel() + 8, dtype=pair[0].dtype, device=dev)
        v = buf.view(-1)[2:2 + pair[0].numel()].view(pair[0].shape)         # 4 bytes in for fp16, 8 for fp32: not 16
        v.copy_(pair[0])
        assert v.data_ptr() % 16 != 0
        return v

    wh0, winv0 = d["sp0:W"]
    wh1, winv1 = d["sp1:W"]
    fwd = lambda **k: [k.get("N", N), k.get("T", T), k.get("V", V), k.get("K", K), k.get("ltot", LTC), k.get("x", x), k.get("wh", wh0),
                       k.get("winv", winv0), k.get("coef", d["coef0"]), d["bias_cv"], k.get("z", z[1]), part[1], ctypes.byref(n), xw]
    for kw in (dict(T=24), dict(T=T + 1), dict(V=52), dict(K=10), dict(ltot=LTR), dict(ltot=LTC + 1), dict(N=-1), dict(x=xm),
               dict(z=zm[1]), dict(wh=misaligned(d["sp0:W"])), dict(wh=None), dict(winv=None), dict(coef=None)):
        _refused(dev, "p2r_stgcn_gcn3h_forward", fwd(**kw), (z, part, zm))
        assert n.value == 7 or kw in (dict(wh=None), dict(winv=None), dict(coef=None))       # (those follow the *n_partials query)
        n.value = 7
    dxa = lambda **k: [N, k.get("T", T), k.get("V", V), k.get("K", K), k.get("ltot", LTR), k.get("dz", dz), k.get("wh", wh1), winv1,
                       d["coef1"], k.get("addend", d["addend"]), k.get("mask", d["amask"]), k.get("dx", z[1]), xw]
    for kw in (dict(T=40), dict(V=25), dict(K=12), dict(ltot=LTC), dict(dz=xm), dict(dx=zm[1]), dict(addend=xm), dict(mask=mm),
               dict(addend=None), dict(wh=misaligned(d["sp1:W"]))):
        _refused(dev, "p2r_stgcn_gcn3h_data_gradient", dxa(**kw), (z, zm))
    dw, cb, dc = _out((3, K, 64, 64), dev), _out((3, 64, V), dev), _out((3, LTR, V), dev)
    wg = lambda **k: [k.get("N", N), k.get("T", T), k.get("V", V), k.get("K", K), k.get("ltot", LTR), k.get("x", x), k.get("dz", dz),
                      k.get("coef", d["coef1"]), k.get("nb", 3), k.get("dw", dw[1]), cb[1], xw, xw]
    for kw in (dict(T=6), dict(T=30), dict(V=25), dict(K=12), dict(ltot=LTC), dict(nb=0), dict(nb=65536), dict(N=-1), dict(x=xm),
               dict(dz=xm), dict(x=None), dict(coef=None), dict(dw=None)):
        _refused(dev, "p2r_stgcn_gcn3h_weight_grad", wg(**kw), (dw, cb))
    wd_, dinv = d["sd:W"]
    cg = lambda **k: [k.get("N", N), k.get("T", T), k.get("V", V), k.get("K", K), k.get("ltot", LTR), k.get("x", x), k.get("dz", dz),
                      k.get("wd", wd_), k.get("winv", dinv), k.get("nb", 3), dc[1], xw]
    for kw in (dict(T=24), dict(T=36), dict(V=25), dict(K=12), dict(ltot=0), dict(nb=0), dict(nb=65536), dict(N=-1), dict(x=xm),
               dict(dz=xm), dict(wd=misaligned(d["sd:W"])), dict(wd=None), dict(winv=None)):
        _refused(dev, "p2r_stgcn_gcn3h_coef_grad", cg(**kw), (dc,))
    th, tinv = d["st:W3"]
    part2 = _out((N * 1, 64, 3), dev)
    tc = lambda **k: [N, k.get("T", T), k.get("V", V), x, k.get("scale", d["scale"]), k.get("shift", d["shift"]), k.get("wh", th),
                      k.get("winv", tinv), d["bias"], z[1], k.get("part", part2[1]), ctypes.byref(n), k.get("bz"), k.get("bfin"), None]
    for kw in (dict(T=24), dict(T=T + 1), dict(V=25), dict(shift=None), dict(scale=None), dict(wh=misaligned(d["st:W3"])),
               dict(scale=None, shift=None, bz=d["x"]), dict(scale=None, shift=None, bfin=d["fin"]),
               dict(bz=d["x"], bfin=d["fin"]), dict(scale=None, shift=None, bz=d["x"], bfin=d["fin"], part=None),
               dict(wh=None), dict(winv=None)):
        n.value = 7
        _refused(dev, "p2r_stgcn_tconvh_forward", tc(**kw), (z, part2))
        assert n.value == 7 or kw in (dict(wh=None), dict(winv=None))


def test_zz_report(dev):
    """prints the session's worst error / bound per bounded stage, the old criterion's floor over the observed error, and
    the number of exact stages (the figures of the module docstring)"""
    for stage in sorted(RATIOS):
        rel = REL.get(stage, 0.0)
        print(f"{stage}: error / bound {RATIOS[stage]:.4f}; error / max |ref| {rel:.3e}; 2e-7 / that = {2e-7 / rel if rel else float('inf'):.3g}")
    print(f"{len(EXACT_STAGES)} exact (stage, family) pairs were bit for bit the float64 value")
    assert all(r <= 1 for r in RATIOS.values())
