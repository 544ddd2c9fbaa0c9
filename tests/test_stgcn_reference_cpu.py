"""CPU: the float64 references, bounds, exact cases and emulators of tests/stgcn_cases.py prove themselves before
tests/test_stgcn_sweep_gpu.py trusts them with the kernels.

  * every exact case stays in range: from the float64 reference alone, the sum of absolute terms of every output is
    below 2^24 units of its smallest term and every value is a whole number of units;
  * every case has the edge it is named for (long lists, empty lists, padded slots, zero-valued real coefficients, all
    four mask bytes, the gate elements with the property they are built for, non-zero frames next to every halo);
  * every emulator (the kernels' partitioning in fp32 torch) sits inside its bound on the bounded cases and is bit-exact
    on the exact ones;
  * every mutant of stgcn_cases.MUTANTS is rejected on a named case by the same `check` the GPU sweep uses.
"""
import pytest
import torch

from tests import stgcn_cases as S

SPECIAL = list(S.GATE_CH + S.REV_CH)


@pytest.fixture(scope="module")
def tab():
    return S.tables()


def _ops(N, T, family, **kw):
    return S.Operands(N, T, family=family, **kw)


def _gcn_ref(ops, form, bias=True, addend=False, masked=False):
    x = ops["dz"] if form == 1 else ops["x"]
    W = ops["W"].transpose(1, 2) if form == 1 else ops["W"]
    P = S.planes_of(ops.tab, form, ops["coef1" if form == 1 else "coef0"])
    return S.graph_conv_ref(x, W, P, ops["bias_cv"] if bias else None, ops["addend"] if addend else None,
                            ops["amask"] if masked else None)


def _in_range(val, mag, unit, unit_special):
    """channel axis 1: the gate / control channels have a smaller unit than the ordinary ones"""
    units = torch.full((64,), unit, dtype=torch.float64)
    units[SPECIAL] = unit_special
    units = units.view([1, 64] + [1] * (val.dim() - 2))
    assert float((mag / units).max()) < S.TWO24
    q = val / units
    assert bool((q == q.round()).all())


# ---- exact range --------------------------------------------------------------------------------------------------------------
EXACT_SHAPES = [(1, 16), (2, 32), (3, 48)]


@pytest.mark.parametrize("N,T", EXACT_SHAPES)
def test_exact_graph_conv_cases_stay_in_range(N, T):
    ops = _ops(N, T, "exact")
    for form in (0, 1):
        z, _, mag = _gcn_ref(ops, form, addend=True, masked=True)
        assert S.exact_cap(mag, 0.25) < S.TWO24 and S.is_multiple(z, 0.25)
        nb = min(N * T // 16, 256)
        val, _, smag = S.bwd_sums_ref(z.float(), ops["u"], ops["fin"], nb, "gcn3", bmask=ops["bmask"])
        assert torch.equal(z.float().double(), z)
        assert S.exact_cap(smag, 0.125) < S.TWO24 and S.is_multiple(val, 0.125)
    P1 = S.planes_of(ops.tab, 1, ops["coef1"])
    for nb in (1, 256):
        r = S.weight_grad_ref(ops["x"], ops["dz"], P1, nb)
        assert S.exact_cap(r["dw"][2], 0.5) < S.TWO24 and S.is_multiple(r["dw"][0], 0.5)
        assert S.exact_cap(r["colsum"][2], 1.0) < S.TWO24 and S.is_multiple(r["colsum"][0], 1.0)
    val, _, mag = S.coef_grad_ref(ops["x"], ops["dz"], ops["W"], ops.tab, 1)
    assert S.exact_cap(mag, 0.5) < S.TWO24 and S.is_multiple(val, 0.5)


@pytest.mark.parametrize("family", ["exact", "gate"])
@pytest.mark.parametrize("N,T", EXACT_SHAPES)
def test_exact_tconv_cases_stay_in_range(N, T, family):
    ops = _ops(N, T, family)
    fin = ops["fin"]
    gate = family == "gate"
    for taps, key in ((3, "W3"), (1, "W1")):
        out, _, mag = S.tconv_ref(ops["x"], fin[2], fin[3], ops[key + ("g" if gate else "")], ops["bias"],
                                  ops["add_ct"] if taps == 1 else None)
        assert S.exact_cap(mag, 0.25) < S.TWO24 and S.is_multiple(out, 0.25)
        r = S.tconv_weight_grad_ref(ops["x"], fin[2], fin[3], ops["dout"], taps, 1)
        dw, mag = r["dw"][0], r["dw"][2]
        ordinary = [c for c in range(64) if c not in SPECIAL] if gate else list(range(64))
        assert S.exact_cap(mag[:, ordinary], 0.5) < S.TWO24 and S.is_multiple(dw[:, ordinary], 0.5)
        if gate:
            assert S.exact_cap(mag[:, SPECIAL], 2.0 ** -25) < S.TWO24 and S.is_multiple(dw[:, SPECIAL], 2.0 ** -25)
            assert bool((dw[:, list(S.GATE_CH)] != 0).any()) and not bool(dw[:, list(S.REV_CH)].any())
        assert S.exact_cap(r["dbias"][2], 1.0) < S.TWO24
    # the data gradient of the three-tap convolution and its BatchNorm-backward sums
    dh, _, mag = S.tconv_ref(ops["dout"], None, None, ops["W3"].flip(0).transpose(1, 2))
    assert S.exact_cap(mag, 0.5) < S.TWO24 and S.is_multiple(dh, 0.5)
    val, _, smag = S.bwd_sums_ref(dh.float(), ops["x"], fin, min(N * T // 16, 256), "tconv3")
    _in_range(val, smag, 0.125, 2.0 ** -14 if gate else 0.125)
    val, _, mag = S.bn_dz_ref(ops["x"], fin, ops["dh"], ops["m12"])
    _in_range(val, mag, 2.0 ** -4, 2.0 ** -13 if gate else 2.0 ** -4)
    assert torch.equal(val.float().double(), val)


def test_exact_cases_with_more_tiles_than_workgroups_stay_in_range():
    """(17, 256): the 272 tiles pair tile b of sample 0 with tile b of sample 16 in workgroups 0 .. 15 -- the two samples
    over 16 workgroups are the same pairs"""
    pick = [0, 16]
    ops = S.Operands(17, 256, family="exact", density=0.125)
    for form in (0, 1):
        x = (ops["dz"] if form == 1 else ops["x"])[pick]
        W = ops["W"].transpose(1, 2) if form == 1 else ops["W"]
        P = S.planes_of(ops.tab, form, ops["coef1" if form == 1 else "coef0"])
        z, _, mag = S.graph_conv_ref(x, W, P, ops["bias_cv"] if form == 0 else None, ops["addend"][pick], ops["amask"][pick])
        assert S.exact_cap(mag, 0.25) < S.TWO24 and S.is_multiple(z, 0.25)
        val, _, smag = S.bwd_sums_ref(z.float(), ops["u"][pick], ops["fin"], 16, "gcn3", bmask=ops["bmask"][pick])
        assert S.exact_cap(smag, 0.125) < S.TWO24 and S.is_multiple(val, 0.125)
    ops = S.Operands(17, 256, family="gate", density=0.125)
    fin = ops["fin"]
    for key in ("W3g", "W1g"):
        out, _, mag = S.tconv_ref(ops["x"][pick], fin[2], fin[3], ops[key], ops["bias"])
        assert S.exact_cap(mag, 0.25) < S.TWO24 and S.is_multiple(out, 0.25)
    dh, _, mag = S.tconv_ref(ops["dout"][pick], None, None, ops["W3"].flip(0).transpose(1, 2))
    assert S.exact_cap(mag, 0.5) < S.TWO24
    val, _, smag = S.bwd_sums_ref(dh.float(), ops["x"][pick], fin, 16, "tconv3")
    _in_range(val, smag, 0.125, 2.0 ** -14)


# ---- the cases have their edges ---------------------------------------------------------------------------------------------------
def test_tables_have_their_edges(tab):
    for form in (0, 1):
        t = tab[form]
        nreal, gidx = t["nreal"], t["gidx"]
        assert int(nreal.max()) == 12 and bool((nreal >= 6).any())          # steps of six entries, a second step
        assert bool((nreal == 0).any()) and bool((nreal == 1).any())        # empty units; a joint with one neighbour in a plane
        assert bool((gidx < 0).any())                                       # padded slots
        # padded slots point at joint 0, real entries are sorted by joint
        assert bool((t["nbr"][gidx < 0] == 0).all())
    extra = S.tables("extra")
    assert int((extra[0]["gidx"] >= 0).sum()) == int((tab[0]["gidx"] >= 0).sum()) + 1
    ring = S.tables("ring", 17)
    assert ring["V"] == 17 and ring[0]["ltot"] != tab[0]["ltot"]


def test_operands_have_their_edges(tab):
    ops = _ops(2, 32, "bounded")
    for key in ("amask", "bmask"):
        assert sorted(set(ops[key].reshape(-1).tolist())) == list(S.MASK_BYTES)
    for form in (0, 1):
        coef, real = ops[f"coef{form}"], tab[form]["gidx"] >= 0
        assert bool((coef[real] == 0).any()), "no real entry with a zero coefficient"
        assert bool((coef[~real] == 0).all())
    ex = _ops(2, 32, "exact")
    assert set(ex["coef1"][tab[1]["gidx"] >= 0].abs().tolist()) == {0.5, 1.0, 2.0}
    assert set(ex["W"].abs().reshape(-1).tolist()) == {0.0, 0.5, 1.0}
    for o in (ops, ex):         # non-zero frames on both sides of every halo and every interior tile edge
        h = S.transform_ref(o["x"], o["fin"][2], o["fin"][3])
        for t in (0, 15, 16, 31):
            assert bool(((h[:, :, t] != 0).any(-1).sum(-1) >= 32).all()), t          # in most channels of every sample


def test_gate_case_is_what_it_is_named_for():
    ops = _ops(3, 48, "gate")
    x, fin = ops["x"], ops["fin"]
    fused, unfused = S.gate_forms(x, fin[2], fin[3])
    zc = x == torch.tensor(S.ZC, dtype=torch.float32)
    g, r = list(S.GATE_CH), list(S.REV_CH)
    at_gate, at_rev = zc[:, g], zc[:, r]
    assert 200 <= int(at_gate.sum()) <= 1500 and 200 <= int(at_rev.sum()) <= 1500
    assert bool((unfused[:, g][at_gate] <= 0).all()) and bool((fused[:, g][at_gate] > 0).all())
    assert bool((unfused[:, r][at_rev] >= 0).all()) and bool((fused[:, r][at_rev] < 0).all())
    # no other element of the case tells the two forms apart
    differ = (fused > 0) != (unfused > 0)
    assert int(differ.sum()) == int(at_gate.sum())
    assert sorted({c // 16 for c in g}) == [0, 1, 2, 3] and sorted({c // 16 for c in r}) == [0, 1, 2, 3]
    where = at_gate.nonzero()
    assert len(set(where[:, 0].tolist())) == 3 and len(set((where[:, 2] // 16).tolist())) == 3       # samples, tiles
    assert len(set(where[:, 3].tolist())) > 40 and len(set((where[:, 2] % 4).tolist())) == 4         # joints, frames of a 4-tile
    assert bool((where[:, 2] == 0).any()) and bool((where[:, 2] == 47).any())                        # next to both halos
    # the float64 gate of the references is the fused one
    ref_gate = x.double() * fin[2].double()[None, :, None, None] + fin[3].double()[None, :, None, None] > 0
    assert torch.equal(ref_gate, fused > 0)


# ---- emulators inside their bounds, exact on the exact cases --------------------------------------------------------------------
FAMILIES = ["bounded", "exact"]


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("gen,kind,V,N,T", [(3, "skeleton", 53, 2, 32), (2, "extra", 53, 1, 17), (1, "ring", 17, 1, 23)])
def test_graph_conv_emulator(family, gen, kind, V, N, T):
    ops = _ops(N, T, family, kind=kind, V=V)
    ex = ops.exact
    z = S.emulate_graph_conv(ops, 0, gen=gen, max_blocks=3)
    S.check(z, _gcn_ref(ops, 0), ex, "forward")
    dx = S.emulate_graph_conv(ops, 1, gen=gen, with_bias=False, addend=True, masked=True, max_blocks=3)
    S.check(dx, _gcn_ref(ops, 1, bias=False, addend=True, masked=True), ex, "data gradient, masked addend")
    if gen == 3:
        nb = 3
        sums = S.emulate_bwd_sums(dx, ops["u"], ops["fin"], nb, bmask=ops["bmask"])
        S.check(sums, S.bwd_sums_ref(dx, ops["u"], ops["fin"], nb, "gcn3", bmask=ops["bmask"]), ex, "BatchNorm-backward sums")
        if not ex:
            S.check(S.emulate_stats3(z, nb), S.stats3_ref(z, nb), False, "statistics")


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("n_blocks", [1, 3, 8, 16, 24])
def test_gcn3_weight_grad_emulator(family, n_blocks):
    ops = _ops(3, 16, family)                       # 12 tiles: more than 1, 3, 8 (one and a half rounds), fewer than 16, 24
    dw, cs = S.emulate_gcn3_dw(ops, n_blocks)
    ref = S.weight_grad_ref(ops["x"], ops["dz"], S.planes_of(ops.tab, 1, ops["coef1"]), n_blocks)
    assert not torch.isnan(dw).any() and not torch.isnan(cs).any()
    S.check(dw.double().sum(0).float() if ops.exact else _sum32(dw), ref["dw"], ops.exact, "dW")
    S.check(cs.double().sum(0).float() if ops.exact else _sum32(cs), ref["colsum"], ops.exact, "colsum")


def _sum32(part):
    """the partial rows summed in float64 and rounded once: the rounding is one of the bound's operations"""
    return part.double().sum(0).float()


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("n_blocks", [1, 3])
def test_gcn3_coef_grad_emulator(family, n_blocks):
    ops = _ops(2, 16, family)
    part = S.emulate_gcn3_dcoef(ops, n_blocks)
    ref = S.coef_grad_ref(ops["x"], ops["dz"], ops["W"], ops.tab, n_blocks)
    S.check(_sum32(part), ref, ops.exact, "dcoef")
    assert bool((part[:, ops.tab[1]["gidx"] < 0] == 0).all())


@pytest.mark.parametrize("family", ["bounded", "exact", "gate"])
@pytest.mark.parametrize("gen,V,N,T", [(3, 53, 2, 32), (2, 53, 1, 17), (1, 25, 1, 16)])
def test_tconv_emulator(family, gen, V, N, T):
    ops = _ops(N, T, family, V=V, kind="skeleton" if V == 53 else "ring")
    fin, ex, gate = ops["fin"], ops.exact, family == "gate"
    out = S.emulate_tconv(ops, 3, gen=gen, gate_weights=gate, max_blocks=3)
    S.check(out, S.tconv_ref(ops["x"], fin[2], fin[3], ops["W3g" if gate else "W3"], ops["bias"]), ex, "three taps")
    out = S.emulate_tconv(ops, 1, gen=gen, add=True, gate_weights=gate, max_blocks=3)
    S.check(out, S.tconv_ref(ops["x"], fin[2], fin[3], ops["W1g" if gate else "W1"], ops["bias"], ops["add_ct"]), ex, "one tap + add_ct")
    dh = S.emulate_tconv(ops, 3, gen=gen, data_gradient=True, max_blocks=3)
    S.check(dh, S.tconv_ref(ops["dout"], None, None, ops["W3"].flip(0).transpose(1, 2)), ex, "data gradient")
    if T % 16 == 0:
        nb = 3 if gen > 1 else 1
        sums = S.emulate_bwd_sums(dh, ops["x"], fin, nb)
        S.check(sums, S.bwd_sums_ref(dh, ops["x"], fin, nb, "tconv3"), ex, "BatchNorm-backward sums")


@pytest.mark.parametrize("family", ["bounded", "exact", "gate"])
@pytest.mark.parametrize("N,T,n_blocks", [(2, 8, 3), (1, 6, 16)])
def test_tconv_weight_grad_emulator(family, N, T, n_blocks):
    ops = _ops(N, T, family)
    fin, ex = ops["fin"], ops.exact
    dw, db, dz = S.emulate_tconv_dw(ops, 3, n_blocks, with_dz=True)
    ref = S.tconv_weight_grad_ref(ops["x"], fin[2], fin[3], ops["dout"], 3, n_blocks)
    S.check(_sum32(dw), ref["dw"], ex, "dW")
    S.check(_sum32(db), ref["dbias"], ex, "dbias")
    S.check(dz, S.bn_dz_ref(ops["x"], fin, ops["dh"], ops["m12"]), ex, "dz")
    dw1, _, _ = S.emulate_tconv_dw(ops, 1, n_blocks)
    S.check(_sum32(dw1), S.tconv_weight_grad_ref(ops["x"], fin[2], fin[3], ops["dout"], 1, n_blocks)["dw"], ex, "dW, one tap")


# ---- mutants ----------------------------------------------------------------------------------------------------------------------
def _rejected(fn):
    with pytest.raises(AssertionError):
        fn()


def _mutant_graph_conv(mutant, family, form, **kw):
    ops = _ops(2, 32, family)
    z = S.emulate_graph_conv(ops, form, max_blocks=3, mutant=mutant, **kw)
    ref = _gcn_ref(ops, form, bias=kw.get("with_bias", True), addend=kw.get("addend", False), masked=kw.get("masked", False))
    _rejected(lambda: S.check(z, ref, ops.exact, mutant))


def _mutant_dw(mutant, n_blocks, what="dw"):
    for family in FAMILIES:
        ops = _ops(3, 16, family)
        dw, cs = S.emulate_gcn3_dw(ops, n_blocks, mutant=mutant)
        ref = S.weight_grad_ref(ops["x"], ops["dz"], S.planes_of(ops.tab, 1, ops["coef1"]), n_blocks)
        got = _sum32(dw if what == "dw" else cs)
        _rejected(lambda: S.check(got, ref[what], ops.exact, mutant))


def _mutant_tconv(mutant, family="bounded"):
    ops = _ops(2, 32, family)
    fin = ops["fin"]
    out = S.emulate_tconv(ops, 3, gate_weights=family == "gate", max_blocks=3, mutant=mutant)
    ref = S.tconv_ref(ops["x"], fin[2], fin[3], ops["W3g" if family == "gate" else "W3"], ops["bias"])
    _rejected(lambda: S.check(out, ref, ops.exact, mutant))


def _mutant_unfused_gate():
    _mutant_tconv("unfused_gate", "gate")                       # forward: an open gate is +-0.5 or +-1 of an exact output
    ops = _ops(2, 8, "gate")
    fin = ops["fin"]
    dw, _, dz = S.emulate_tconv_dw(ops, 3, 3, with_dz=True, mutant="unfused_gate")
    ref = S.tconv_weight_grad_ref(ops["x"], fin[2], fin[3], ops["dout"], 3, 3)
    _rejected(lambda: S.check(_sum32(dw), ref["dw"], True, "dW"))
    _rejected(lambda: S.check(dz, S.bn_dz_ref(ops["x"], fin, ops["dh"], ops["m12"]), True, "dz"))
    ops = _ops(2, 32, "gate")
    dh = S.emulate_tconv(ops, 3, data_gradient=True, max_blocks=3)
    sums = S.emulate_bwd_sums(dh, ops["x"], ops["fin"], 3, mutant="unfused_gate")
    _rejected(lambda: S.check(sums, S.bwd_sums_ref(dh, ops["x"], ops["fin"], 3, "tconv3"), True, "sums"))


def _mutant_pad_as_joint0():
    for family in FAMILIES:
        ops = _ops(2, 16, family)
        part = S.emulate_gcn3_dcoef(ops, 3, mutant="pad_as_joint0")
        ref = S.coef_grad_ref(ops["x"], ops["dz"], ops["W"], ops.tab, 3)
        _rejected(lambda: S.check(_sum32(part), ref, ops.exact, "dcoef"))


def _mutant_pad_below_tile_longest():
    """the first-generation kernel on the ring skeleton of 17 joints, tiles of 22 frames: 16 columns are one or two joints"""
    for family in FAMILIES:
        ops = _ops(1, 23, family, kind="ring", V=17)
        assert bool((S.tile_longest(ops.tab, 22) & (ops.tab[1]["gidx"] < 0)).any()), "no padded slot below a neighbour's list"
        ref = S.coef_grad_ref(ops["x"], ops["dz"], ops["W"], ops.tab, 2, F=22, first_gen=True)
        S.check(_sum32(S.emulate_gcn3_dcoef(ops, 2, F=22)), ref, ops.exact, "dcoef")
        part = S.emulate_gcn3_dcoef(ops, 2, mutant="pad_below_tile_longest", F=22)
        _rejected(lambda: S.check(_sum32(part), ref, ops.exact, "dcoef"))


def _mutant_full_count():
    ops = _ops(2, 32, "bounded")
    z = S.emulate_graph_conv(ops, 0, max_blocks=3)
    _rejected(lambda: S.check(S.emulate_stats3(z, 3, mutant="full_count"), S.stats3_ref(z, 3), False, "statistics"))


def _mutant_mask_eq_1():
    for family in FAMILIES:
        _mutant_graph_conv("mask_eq_1", family, 1, with_bias=False, addend=True, masked=True)
    ops = _ops(2, 32, "exact")
    dx = S.emulate_graph_conv(ops, 1, with_bias=False, addend=True, masked=True, max_blocks=3)
    sums = S.emulate_bwd_sums(dx, ops["u"], ops["fin"], 3, bmask=ops["bmask"], mutant="mask_eq_1")
    _rejected(lambda: S.check(sums, S.bwd_sums_ref(dx, ops["u"], ops["fin"], 3, "gcn3", bmask=ops["bmask"]), True, "sums"))


MUTANT_CASES = {
    "halo_neighbour_row": lambda: [_mutant_tconv("halo_neighbour_row", f) for f in FAMILIES],
    "halo_missing_interior": lambda: [_mutant_tconv("halo_missing_interior", f) for f in FAMILIES],
    "drop_last_entry": lambda: [_mutant_graph_conv("drop_last_entry", f, form) for f in FAMILIES for form in (0, 1)],
    "pad_as_joint0": _mutant_pad_as_joint0,
    "pad_below_tile_longest": _mutant_pad_below_tile_longest,
    "mask_eq_1": _mutant_mask_eq_1,
    "unfused_gate": _mutant_unfused_gate,
    "xcd_skip_tail": lambda: _mutant_dw("xcd_skip_tail", 8),            # 12 tiles over 8 workgroups: half a second round
    "strided_double": lambda: _mutant_dw("strided_double", 3),
    "idle_unwritten": lambda: _mutant_dw("idle_unwritten", 16),          # 12 tiles: four workgroups idle
    "full_count": _mutant_full_count,                                    # 4 tiles over 3 workgroups: counts 2, 1, 1
    "colsum_7th": lambda: _mutant_dw("colsum_7th", 3, "colsum"),
    "dw_untransposed": lambda: _mutant_dw("dw_untransposed", 3),
    "addend_before_mask": lambda: [_mutant_graph_conv("addend_before_mask", f, 1, with_bias=False, addend=True, masked=True)
                                   for f in FAMILIES],
}


def test_every_mutant_has_a_case():
    assert sorted(MUTANT_CASES) == sorted(S.MUTANTS)


@pytest.mark.parametrize("mutant", S.MUTANTS)
def test_mutant_is_rejected(mutant):
    MUTANT_CASES[mutant]()
