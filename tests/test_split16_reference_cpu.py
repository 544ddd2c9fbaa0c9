"""CPU: the float64 stage references, derived bounds, exact families and torch emulators of tests/split16_cases.py for the
split16 ST-GCN kernels.  Shows, without a GPU, that
  * every emulator (the kernels' partitioning and two-part arithmetic in torch) is inside its derived per-element bound on
    ordinary and on heavy-tailed operands;
  * every exact case (E0, EW, EX and the gate case) satisfies the conditions the families are built on -- every scaled
    operand finite in fp16 and represented exactly, no value-carrying part an fp16 subnormal, the dropped term a2 b2
    identically zero, the sum of absolute part products below 2^24 units -- asserted from the float64 reference and the
    host split alone, and that the emulator then EQUALS the float64 value;
  * `check` rejects every named mutant of split16_cases.MUTANTS on a named case.
"""
import pytest
import torch

from tests import split16_cases as H
from tests import stgcn_cases as S

K, C, V = H.K, H.C, H.V53


def _ops(N, T, family="exact", **kw):
    return H.Operands(N, T, family=family, **kw)


def _fam_ops(N, T, fam, **kw):
    return _ops(N, T, "bounded" if fam in ("bounded", "tail") else ("gate" if fam == "gate" else "exact"), **kw)


def _wf(ops, wkey, form):
    return ops[wkey].transpose(1, 2).contiguous() if form == 1 else ops[wkey]


# ---- graph conv forward / data gradient -------------------------------------------------------------------------------------------
def _gcn(ops, form, fam, word="own", mutant=None, addend=False, masked=False):
    xk, wk, ck = H.gcn_keys(form, fam)
    w = H.amax_word(ops[xk]) if word == "own" else word
    got = H.emulate_gcn3h(ops, form, xk, wk, ck, w, with_bias=form == 0, addend=addend, masked=masked, mutant=mutant)
    ref = H.gcnh_ref(ops[xk], _wf(ops, wk, form), H.planes(ops, form, ops[ck]), w, form == 1,
                     ops["bias_cv"] if form == 0 else None, ops["addend"] if addend else None,
                     ops["amask"] if masked else None)
    return got, ref


def _gcn_conditions(ops, form, fam):
    xk, wk, ck = H.gcn_keys(form, fam)
    x, W = ops[xk], _wf(ops, wk, form)
    assert float(x.abs().max()) in (2.0, (2047 + 0.375) / 1024), "the maximum the range word is built from"
    s_x = H.word_scale(H.amax_word(x))
    assert s_x == (2.0 ** 11 if fam != "EX" else 2.0 ** 12)
    w1, w2, s_w = H.weight_parts(W, f"gcn form {form} {fam}")
    P = H.planes(ops, form, ops[ck])
    agg = torch.einsum("kws,ncts->knctw", P, x.double()) * s_x
    assert torch.equal(agg.float().double(), agg), "the aggregate is not an fp32 number"
    b1, b2 = H.exact_split(agg, 1.0, form == 1, f"gcn form {form} {fam}: aggregate")
    if fam == "EW":
        assert bool((w2 != 0).any()) and not bool((b2 != 0).any())
        for pair in H.PAIRS[form]:                   # the w2 plane of every pair and phase carries value
            for k in pair:
                if k >= 0:
                    for ph in range(4):
                        assert bool((w2[k][:, 16 * ph:16 * ph + 16] != 0).any()), (pair, k, ph)
    if fam == "EX":
        assert bool((b2 != 0).any()) and not bool((w2 != 0).any())
    if fam == "E0":
        assert not bool((w2 != 0).any()) and not bool((b2 != 0).any())
    contract = lambda wa, ba: torch.einsum("kdc,knctw->ndtw", wa, ba)
    extra = ops["bias_cv"].double()[None, :, None, :] * (s_x * s_w) if form == 0 else ops["addend"].double() * (s_x * s_w)
    return H.product_conditions(w1, w2, b1, b2, contract, f"gcn form {form} {fam}", extra)


@pytest.mark.parametrize("fam", H.EXACT_FAMILIES)
@pytest.mark.parametrize("form", [0, 1])
def test_graph_conv_exact_families(form, fam):
    ops = _ops(2, 32)
    _gcn_conditions(ops, form, fam)
    for word in ("own", H.same_exponent_word(H.amax_word(ops[H.gcn_keys(form, fam)[0]]))):
        got, ref = _gcn(ops, form, fam, word=word, addend=form == 1, masked=form == 1)
        H.check(got, ref, True, f"gcn3h form {form} {fam}")


@pytest.mark.parametrize("fam", ["bounded", "tail"])
@pytest.mark.parametrize("form", [0, 1])
def test_graph_conv_emulator_in_bound(form, fam):
    ops = _fam_ops(1, 48, fam)
    for addend, masked in ((False, False), (True, False), (True, True)) if form == 1 else ((False, False),):
        got, ref = _gcn(ops, form, fam, addend=addend, masked=masked)
        assert H.check(got, ref, False, f"gcn3h form {form} {fam}") <= 1
    got, ref = _gcn(ops, form, "bounded", word=None)                      # x_amax == NULL: scale 1
    H.check(got, ref, False, "gcn3h, no range word")


# ---- temporal conv ----------------------------------------------------------------------------------------------------------------
def _tconvh(ops, form, fam, word="own", mutant=None, xkey=None):
    xk, wk, fk = H.tconvh_keys(form, fam)
    xk = xkey or xk
    w = None if form == "forward" else (H.amax_word(ops[xk]) if word == "own" else word)
    fwd = form == "forward"
    got, part = H.emulate_tconvh(ops, xk, wk, w, form, fk, with_bias=fwd, mutant=mutant)
    fin = ops[fk]
    ref = H.tconvh_ref(ops[xk], fin[2] if fwd else None, fin[3] if fwd else None, ops[wk], w, ops["bias"] if fwd else None)
    return got, part, ref


def _tconvh_conditions(ops, form, fam):
    xk, wk, fk = H.tconvh_keys(form, fam)
    x, W3, fin = ops[xk], ops[wk], ops[fk]
    fwd = form == "forward"
    s_x = 1.0 if fwd else H.word_scale(H.amax_word(x))
    h = H.clamp_h(x, fin[2], fin[3]) if fwd else x.double()
    assert torch.equal(h.float().double(), h)
    special = list(S.GATE_CH + S.REV_CH)
    gate_fwd = fam == "gate" and fwd
    w1, w2, s_w = H.weight_parts(W3, f"tconvh {form} {fam}", special if gate_fwd else None)
    if gate_fwd:                                    # the tiny open gates: p = 0, q' = 2^-14 (normal); everything else residual-free
        p, q = H.parts_of(h, s_x, True)
        assert torch.equal(p + q, h * s_x) and float(h[h != 0].abs().min()) == 2.0 ** -25
        keep = [c for c in range(C) if c not in special]
        assert not bool(q[:, keep].any()) and not bool(p[:, special][h[:, special] < 1e-3].any())
        b1, b2 = p, q
    else:
        b1, b2 = H.exact_split(h, s_x, True, f"tconvh {form} {fam}")
    if fam == "EW":
        assert bool((w2 != 0).any()) and all(bool((w2[p] != 0).any()) for p in range(3))
    if fam == "EX":
        assert bool((b2 != 0).any())
    contract = lambda wa, ba: sum(torch.einsum("dc,nctv->ndtv", wa[p], S._shifted(ba, p, 3)) for p in range(3))
    extra = ops["bias"].double()[None, :, None, None] * (s_x * s_w) if fwd else None
    if not gate_fwd:
        return H.product_conditions(w1, w2, b1, b2, contract, f"tconvh {form} {fam}", extra)
    # two kinds of terms: 2^25-weights times 2^-25 gates (0.5 or 1 each) and ordinary ones (multiples of 0.25)
    total, units = 0.0, []
    for chans, ex in ((special, None), (keep, extra)):
        m = torch.zeros(C, dtype=torch.float64)
        m[chans] = 1.0
        cap, unit = H.product_conditions(w1 * m, w2 * m, b1 * m[None, :, None, None], b2 * m[None, :, None, None], contract,
                                         f"tconvh {form} {fam}", ex)
        total, units = total + cap * unit, units + [unit]
    assert total / min(units) < S.TWO24


TCONVH_EXACT = [(form, fam) for form in ("forward", "plain", "bwd") for fam in H.EXACT_FAMILIES] + [("forward", "gate"), ("bwd", "gate")]


@pytest.mark.parametrize("form,fam", TCONVH_EXACT)
@pytest.mark.parametrize("T", [16, 96])
def test_tconvh_exact_families(T, form, fam):
    ops = _fam_ops(2, T, fam)
    _tconvh_conditions(ops, form, fam)
    got, part, ref = _tconvh(ops, form, fam)
    H.check(got, ref, True, f"tconvh {form} {fam}")
    if fam == "gate" and form == "forward":
        fused, unfused = S.gate_forms(ops["x"], ops["fin"][2], ops["fin"][3])
        assert bool(((fused > 0) != (unfused > 0)).any()), "no element tells the fused gate from the unfused one"
    if form == "bwd":
        sref = H.bwd_chunk_ref(got, ops["x"], ops["fin"], H.chunk_of(T))
        H.check(part, sref, fam in ("E0", "gate"), f"tconvh sums {fam}")    # the other families' sums leave the exact range


@pytest.mark.parametrize("fam", ["bounded", "tail"])
@pytest.mark.parametrize("T", [16, 32, 48, 64, 128])
def test_tconvh_emulator_in_bound(T, fam):
    ops = _fam_ops(1, T, fam)
    for form in ("forward", "plain", "bwd"):
        if fam == "tail" and form == "forward":
            continue                                 # the forward form takes no range word
        got, part, ref = _tconvh(ops, form, fam)
        H.check(got, ref, False, f"tconvh {form} {fam}")
        if form == "forward":
            H.check_bound(part, H.stats_chunk_ref(got, H.chunk_of(T)), "tconvh statistics")
        if form == "bwd":
            H.check(part, H.bwd_chunk_ref(got, ops["x"], ops["fin"], H.chunk_of(T)), False, "tconvh sums")


# ---- weight and adjacency gradients -----------------------------------------------------------------------------------------------
def _dwh(ops, fam, nb, words=(True, True), mutant=None):
    xk, zk, ck = H.dwh_keys(fam)
    xw = H.amax_word(ops[xk]) if words[0] else None
    zw = H.amax_word(ops[zk]) if words[1] else None
    dw, cb = H.emulate_gcn3dwh(ops, xk, zk, ck, nb, xw, zw, mutant)
    ref = H.dwh_ref(ops[xk], ops[zk], H.planes(ops, 1, ops[ck]), nb, xw, zw)
    return dw, cb, ref


def _dwh_conditions(ops, fam):
    xk, zk, ck = H.dwh_keys(fam)
    x, dz = ops[xk], ops[zk]
    s_x, s_g = H.word_scale(H.amax_word(x)), H.word_scale(H.amax_word(dz))
    x1, x2 = H.exact_split(x, s_x, False, f"gcn3dwh {fam}: x")
    assert float(x1[x1 != 0].abs().min()) >= 2.0 ** -3, "2^-11 x1 is not a normal number"
    P = H.planes(ops, 1, ops[ck])
    agg = torch.einsum("kvw,nctw->knctv", P, dz.double()) * s_g
    assert torch.equal(agg.float().double(), agg)
    v1, v2 = H.exact_split(agg, 1.0, True, f"gcn3dwh {fam}: aggregate")
    assert bool((x2 != 0).any()) == (fam == "EW") and bool((v2 != 0).any()) == (fam == "EX")
    contract = lambda xa, va: torch.einsum("nitv,knctv->kic", xa, va)
    return H.product_conditions(x1, x2, v1, v2, contract, f"gcn3dwh {fam}")


@pytest.mark.parametrize("fam", H.EXACT_FAMILIES)
def test_weight_grad_exact_families(fam):
    ops = _ops(2, 8)
    _dwh_conditions(ops, fam)
    for nb in (1, 3, 5):
        dw, cb, ref = _dwh(ops, fam, nb)
        H.check(dw.double().sum(0).float(), ref["dw"], True, f"gcn3dwh {fam}")
        H.check(cb.double().sum(0).float(), ref["colsum"], True, f"gcn3dwh bias table {fam}")


@pytest.mark.parametrize("fam", ["bounded", "tail"])
def test_weight_grad_emulator_in_bound(fam):
    ops = _fam_ops(2, 8, fam)
    for words in ((True, True), (False, True), (True, False)):
        if fam == "tail" and not all(words):
            continue
        dw, cb, ref = _dwh(ops, fam, 3, words)
        H.check(dw.double().sum(0).float(), ref["dw"], False, f"gcn3dwh {fam}")
        H.check(cb.double().sum(0).float(), ref["colsum"], False, f"gcn3dwh bias table {fam}")


def _dcoef(ops, fam, nb, mutant=None):
    xk, wk = H.dcoef_keys(fam)
    xw = H.amax_word(ops[xk])
    got = H.emulate_gcn3h_dcoef(ops, xk, wk, nb, xw, mutant)
    return got, H.dcoefh_ref(ops[xk], ops["dz"], ops[wk], ops.tab, nb, xw)


def _dcoef_conditions(ops, fam):
    xk, wk = H.dcoef_keys(fam)
    x, W, dz = ops[xk], ops[wk], ops["dz"]
    s_x = H.word_scale(H.amax_word(x))
    w1, w2, s_w = H.weight_parts(W, f"dcoef {fam}")
    x1, x2 = H.exact_split(x, s_x, False, f"dcoef {fam}: x")
    assert bool((w2 != 0).any()) == (fam == "EW") and bool((x2 != 0).any()) == (fam == "EX")
    t = ops.tab[1]
    da = dz.double().abs()
    gathered = torch.stack([da[:, :, :, t["nbr"][l].long()] for l in range(t["ltot"])])          # [l][n][c][t][v]

    def contract(wa, xa):
        out = torch.zeros(t["ltot"], V, dtype=torch.float64)
        for k in range(K):
            Y = torch.einsum("dc,nctv->ndtv", wa[k], xa)
            for l in range(t["lofs"][k], t["lofs"][k + 1]):
                out[l] = (Y * gathered[l]).sum((0, 1, 2))
        return out
    return H.product_conditions(w1, w2, x1, x2, contract, f"dcoef {fam}")


@pytest.mark.parametrize("fam", H.EXACT_FAMILIES)
def test_coef_grad_exact_families(fam):
    ops = _ops(1, 32)
    _dcoef_conditions(ops, fam)
    for nb in (1, 2, 3):
        got, ref = _dcoef(ops, fam, nb)
        H.check(got.double().sum(0).float(), ref, True, f"gcn3h_coef_grad {fam}")


@pytest.mark.parametrize("fam", ["bounded", "tail"])
def test_coef_grad_emulator_in_bound(fam):
    ops = _fam_ops(1, 32, fam)
    got, ref = _dcoef(ops, fam, 3)
    H.check(got.double().sum(0).float(), ref, False, f"gcn3h_coef_grad {fam}")
    assert not bool(got[:, ops.tab[1]["gidx"] < 0].any())


# ---- mutants ----------------------------------------------------------------------------------------------------------------------
def _rejected(fn):
    with pytest.raises(AssertionError):
        fn()


def test_every_mutant_is_rejected():
    """each defect on the case that is built to see it; the same call without the mutant passes (the tests above)"""
    seen = set()

    def gcn(mutant, form, fam, **kw):
        ops = _ops(1, 16)
        got, ref = _gcn(ops, form, fam, mutant=mutant, **kw)
        _rejected(lambda: H.check(got, ref, True, mutant))
        seen.add(mutant)

    def tconv(mutant, form, fam, exact=True, N=2, T=32, xkey=None):
        ops = _fam_ops(N, T, fam)
        got, _, ref = _tconvh(ops, form, fam, mutant=mutant, xkey=xkey)
        _rejected(lambda: H.check(got, ref, exact, mutant))
        seen.add(mutant)

    gcn("drop_a2b1_plane_b", 0, "EW")                       # forward, weight residual alive
    gcn("drop_a2b1_plane_b", 1, "EW")
    gcn("res_unscaled", 1, "EX")                            # data gradient, operand residual alive
    gcn("w1s_as_w1", 1, "EX")
    gcn("single_pair_plane0", 0, "E0")                      # pair (2, -1) of the forward
    gcn("single_pair_plane0", 1, "E0")                      # pair (10, -1) of the data gradient
    gcn("scale_one_rescaled", 0, "E0")
    gcn("mask_eq_1", 1, "E0", addend=True, masked=True)
    gcn("addend_before_mask", 1, "E0", addend=True, masked=True)
    tconv("res_unscaled", "plain", "EX")
    tconv("w1s_as_w1", "plain", "EX")
    tconv("scale_one_rescaled", "plain", "E0")
    tconv("halo_relu_shift", "forward", "E0")               # shift != 0 in most channels of the exact family
    tconv("halo_neighbour_sample", "plain", "E0")           # N = 2: sample 1 starts behind sample 0's last frame
    tconv("halo_neighbour_sample", "forward", "E0")
    # the clamp: activations beyond fp16's range, a bounded case (with the clamp it is inside its bound)
    ops = _ops(1, 16, "bounded")
    got, _, ref = _tconvh(ops, "forward", "bounded", xkey="xbig")
    assert float(H.clamp_h(ops["xbig"], ops["fin"][2], ops["fin"][3]).max()) == H.H16_MAX
    H.check(got, ref, False, "clamped activations")
    tconv("no_clamp", "forward", "bounded", exact=False, N=1, T=16, xkey="xbig")
    # per-workgroup rows: more workgroups than tiles, and a workgroup with one tile fewer
    ops = _ops(1, 8)
    dw, cb, ref = _dwh(ops, "E0", 3, mutant="idle_unwritten")                 # 2 tiles, 3 workgroups
    _rejected(lambda: H.check(dw.double().sum(0).float(), ref["dw"], True, "idle_unwritten"))
    ops = _ops(1, 16)
    got, ref = _dcoef(ops, "E0", 2, mutant="idle_unwritten")                  # 1 tile, 2 workgroups
    _rejected(lambda: H.check(got.double().sum(0).float(), ref, True, "idle_unwritten"))
    seen.add("idle_unwritten")
    ops = _ops(1, 48, "bounded")                                               # 3 tiles over 2 workgroups
    z, _ = _gcn(ops, 0, "bounded")
    H.check_bound(S.emulate_stats3(z, 2), S.stats3_ref(z, 2), "gcn3h statistics")
    _rejected(lambda: H.check_bound(S.emulate_stats3(z, 2, mutant="full_count"), S.stats3_ref(z, 2), "full_count"))
    seen.add("full_count")
    # the range word of p2r_stgcn_tconv_weight_grad_dz_amax: a second call on smaller data leaves the smaller word
    from tests.bn_cases import check_amax
    big, small = ops["dz"] * 8, ops["dz"]
    w = H.emulate_amax_word(0x12345678, big)
    check_amax(w, big)
    check_amax(H.emulate_amax_word(w, small), small)
    _rejected(lambda: check_amax(H.emulate_amax_word(w, small, mutant="word_not_cleared"), small))
    seen.add("word_not_cleared")
    assert seen == set(H.MUTANTS), set(H.MUTANTS) - seen


def test_range_word_scale():
    """p2r_split_scale on the host: the maximum lands in [2^12, 2^13); a power of two and one ulp below it differ by one
    exponent; zero, subnormal, infinite and NaN words give scale 1"""
    for v in (1.0, 2.0, 3.999, 1e-6, 1e3, 2.0 ** -100):
        s = H.word_scale(H.bits_of(v))
        assert 2.0 ** 12 <= v * s < 2.0 ** 13
    assert H.word_scale(H.bits_of(2.0)) * 2 == H.word_scale(H.bits_of(2.0) - 1)
    for word in (0, 1, 0x7F800000, 0x7FC00000, None):
        assert H.word_scale(word) == 1.0
    assert H.word_scale(H.same_exponent_word(H.bits_of(2.0))) == H.word_scale(H.bits_of(2.0))
