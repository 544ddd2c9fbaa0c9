"""CPU: the float64 references of the BatchNorm and partial-sum kernels (tests/bn_cases.py) against float64 autograd, the
conditions on the cases that the GPU sweep (tests/test_bn_sweep_gpu.py) relies on, and the sensitivity of the comparison
functions both tests share.

The stage references, chained (statistics -> constants -> apply -> backward sums -> their constants -> backward apply),
must equal float64 autograd of relu(bn(x) + res) to float64 rounding, and that in turn nn.BatchNorm2d in float64: a
wrong formula in a reference would otherwise be "confirmed" by a kernel with the same mistake.

Sensitivity: for every stage a torch emulation of the kernel's partitioning (rows, chunks of `bn_chunks`, float4 body and
scalar tail, the 256 threads, shuffle steps and waves) passes the comparison function under the derived bound, and every
defect of bn_cases.MUTANTS fails it on at least one case of its stage.  What is proven here about the checks holds on the
GPU, which calls the same functions.
"""
import pytest
import torch

from tests import bn_cases as B

F64 = 1e-12


def _same(a, b, what, tol=F64):
    assert a.shape == b.shape, what
    assert (a - b).abs().max() <= tol * (b.abs().max() + 1e-300), (what, (a - b).abs().max().item())


def _caught(fn):
    """True when the comparison function rejects what `fn` hands it"""
    try:
        fn()
    except AssertionError:
        return True
    return False


# ---- the references against float64 autograd -----------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("with_res", [False, True], ids=["nores", "res"])
@pytest.mark.parametrize("shape", [(3, 8, 7, 5), (2, 6, 35)])
def test_stage_references_chain_to_autograd(shape, with_res, mode):
    """mode 0: no ReLU; mode 1: ReLU with the gate read from the forward's own output"""
    case = B.op_case(shape)
    relu = mode == 1
    want = B.op_ref(case, with_res, relu, True)
    N, C = shape[:2]
    x = case["x"].double().reshape(N, C, -1)
    L = x.shape[2]
    st = B.stats_ref(x.reshape(N * C, L))
    part = torch.stack([torch.full((N * C,), st["count"], dtype=torch.float64), st["mean"][0], st["M2"][0]], 1).reshape(N, C, 3)
    fcase = {"part": part, "M": float(N * L), "gamma": case["gamma"].double(), "beta": case["beta"].double(),
             "running_mean": case["running_mean"].double(), "running_var": case["running_var"].double()}
    fin = B.finalize_ref(fcase, 0.1)
    mean, invstd, scale, shift = fin["out"][0]
    _same(fin["running_mean"][0], want["running_mean"], "running_mean")
    _same(fin["running_var"][0], want["running_var"], "running_var")
    res = case["res"].double().reshape(N, C, L) if with_res else None
    pre, E = B.apply_ref(x, scale, shift, res)
    _same(pre, want["pre"].reshape(N, C, L), "pre")
    assert (E > 0).all()
    y = torch.relu(pre) if relu else pre
    back = {"x": x, "dy": case["go"].double().reshape(N, C, L), "y": y, "mean": mean, "invstd": invstd, "kscale": scale}
    sums, Es = B.bwd_reduce_ref(back, mode)
    tot, _ = B.bwd_finalize_ref(sums.reshape(N, C, 2), float(N * L))
    _same(tot[0], want["dbeta"], "dbeta")
    _same(tot[1], want["dgamma"], "dgamma", 1e-11)
    back.update(m1=tot[2], m2=tot[3])
    ref = B.bwd_apply_ref(back, mode)
    _same(ref["dx"][0], want["dx"].reshape(N, C, L), "dx", 1e-11)
    if with_res:
        _same(ref["dres"], want["dres"].reshape(N, C, L), "dres")
    assert (Es >= 0).all() and (ref["dx"][1] > 0).all()


@pytest.mark.parametrize("train", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("relu", [True, False], ids=["relu", "norelu"])
@pytest.mark.parametrize("shape", B.OP_SHAPES[:1] + B.OP_SHAPES[3:])
def test_op_ref_is_the_module_chain(shape, relu, train):
    case = B.op_case(shape)
    got = B.op_ref(case, True, relu, train)
    bn = (torch.nn.BatchNorm2d if len(shape) == 4 else torch.nn.BatchNorm1d)(shape[1]).double().train(train)
    with torch.no_grad():
        bn.weight.copy_(case["gamma"]), bn.bias.copy_(case["beta"])
        bn.running_mean.copy_(case["running_mean"]), bn.running_var.copy_(case["running_var"])
    x, res = case["x"].double().requires_grad_(True), case["res"].double().requires_grad_(True)
    y = bn(x) + res
    y = torch.relu(y) if relu else y
    y.backward(case["go"].double())
    for k, v in (("y", y.detach()), ("dx", x.grad), ("dres", res.grad), ("dgamma", bn.weight.grad), ("dbeta", bn.bias.grad),
                 ("running_mean", bn.running_mean), ("running_var", bn.running_var)):
        _same(got[k], v, k, 1e-10)
    again = B.op_ref(case, True, relu, train, gate=got["pre"] > 0)
    assert torch.equal(again["dx"], got["dx"])
    if relu:        # and a gate that is turned moves a gradient: the argument is not ignored
        assert not torch.equal(B.op_ref(case, True, relu, train, gate=got["pre"] > 0.3)["dx"], got["dx"])


def test_tr64_and_width2_helpers():
    inp = B.sum_case(3, 8192)
    value, E = B.sum_leading_ref(inp, tr64=True)
    s = inp.double().sum(0).reshape(2, 64, 64)
    assert value[4096 + 5 * 64 + 9] == s[1, 9, 5] and value[7 * 64 + 63] == s[0, 63, 7] and (E > 0).all()
    x = B.op_case((3, 8, 7, 5))["x"]
    w2 = B.width2_partials(x)
    assert w2.shape == (3, 8, 2)
    mean, m2, M = B._merge(w2, 3 * 35.0)
    _same(mean, x.double().mean((0, 2, 3)), "mean", 1e-6)
    _same(m2 / M, x.double().var((0, 2, 3), unbiased=False), "var", 1e-5)


# ---- the cases -----------------------------------------------------------------------------------------------------------------
def test_chunk_counts_and_shapes():
    assert B.CHUNK_SHAPES == [(1, 3, 8191), (1, 3, 8192), (2, 3, 8197), (1, 2, 16389), (3, 5, 35)]
    counts = [B.bn_chunks(N * C, L) for N, C, L in B.CHUNK_SHAPES]
    assert counts == B.CHUNK_COUNTS == [1, 2, 2, 4, 1]
    assert B.bn_chunks(2048, 1 << 20) == 1 and B.bn_chunks(4, 155 * 53) == 2
    spans = lambda N, C, L: [(lo, hi, b0, b1) for r, _, lo, hi, b0, b1 in B._spans(N * C, L, [True] * (N * C)) if r == 0]
    assert spans(1, 3, 8192) == [(0, 4096, 0, 4096), (4096, 8192, 4096, 8192)]
    assert spans(2, 3, 8197) == [(0, 4100, 0, 4100), (4100, 8197, 4100, 8196)]           # 4097 long, a tail of 1
    assert spans(1, 2, 16389)[-1] == (12300, 16389, 12300, 16388)                        # 4089 long
    assert len(spans(1, 2, 16389)) == 4 and spans(3, 5, 35) == [(0, 35, 0, 32)]
    assert B.STATS_L == (1, 3, 4, 1023, 1024, 1025, 1028, 2051) and max(B.STATS_L) ** 2 * B.U <= 0.26
    assert B.FIN_P == (1, 255, 256, 257, 600) and B.FIN_C == (1, 3, 64) and B.FIN_MOMENTUM == (0.1, 1.0, 0.0, -1.0)
    assert B.COLSUM_V == (1, 53, 128, 129, 255, 256) and B.COLSUM_T == (1, 5, 39)
    assert B.SUM_P == (1, 7, 8, 9, 31, 32, 33, 127, 128, 129, 256, 300) and B.SUM_M == (4, 60, 64, 68, 1028)
    assert B.SUM_M_TR64 == (4096, 8192)
    assert B.OP_SHAPES == [(3, 8, 7, 5), (2, 64, 16, 53), (1, 4, 155, 53), (2, 6, 35)]
    assert (B.Y_TOL, B.STAT_TOL, B.DX_TOL, B.PARAM_TOL) == ((1e-5, 1e-5), (1e-5, 1e-6), (1e-4, 1e-5), 1e-4)
    # rows of both alignments in one case
    assert sorted(set(B._row_vec(B.STATS_ROWS, 1025, 0).tolist())) == [False, True]
    assert sorted(set(B._row_vec(6, 8197, 0).tolist())) == [False, True]


@pytest.mark.parametrize("with_res", [False, True], ids=["nores", "res"])
@pytest.mark.parametrize("N,C,L", B.CHUNK_SHAPES + B.REDUCE_SHAPES)
def test_gate_band_share(N, C, L, with_res):
    c = B.ew_case(N, C, L)
    ref = B.apply_ref(c["x"], c["scale"], c["shift"], c["res"] if with_res else None)
    share = B.gate_band(ref).double().mean().item()
    print(f"{(N, C, L)} res {with_res}: share of the gates inside the rounding band {share:.2e}")
    assert share <= B.BAND_CAP
    if N * C * L >= 100:
        assert 0.1 < (ref[0] > 0).double().mean() < 0.9
        for mode in (1, 2, 3):
            assert 0.2 < B.gate_of(c, mode).double().mean() < 0.8, mode
        assert not torch.equal(B.gate_of(c, 1), B.gate_of(c, 3)) and not torch.equal(B.gate_of(c, 2), B.gate_of(c, 3))


@pytest.mark.parametrize("shape", B.OP_SHAPES)
@pytest.mark.parametrize("train", [True, False], ids=["train", "eval"])
def test_op_cases_band_share(shape, train):
    """op level: the share of pre-activations within the forward tolerance (1e-5 + 1e-5 |pre|) of zero"""
    case = B.op_case(shape)
    for with_res in (False, True):
        pre = B.op_ref(case, with_res, True, train)["pre"]
        share = (pre.abs() <= B.Y_TOL[1] + B.Y_TOL[0] * pre.abs()).double().mean().item()
        print(f"{shape} res {with_res}: share within the forward tolerance of zero {share:.2e}")
        assert share <= B.BAND_CAP


def test_large_mean_cases():
    for L in B.STATS_L:
        if L < 4:
            continue
        x = B.stats_case(L, "big").double()
        ratio = x.mean(1).abs() / x.std(1)
        assert (ratio > 100).all() and (ratio < 1e4).all(), (L, ratio)
    for P in B.FIN_P:
        for C in B.FIN_C:
            ref = B.finalize_ref(B.finalize_case(P, C, 3, big=True), 0.1)["out"][0]
            ratio = ref[0].abs() * ref[1]           # |mean| invstd
            assert (ratio > 100).all() and (ratio < 1e4).all(), (P, C, ratio)
    c = B.finalize_case(257, 3, 3)
    assert c["part"][:, 0, 0].unique().numel() > 5      # unequal counts
    assert (B.stats_case(1025, "const") == B.stats_case(1025, "const")[:, :1]).all()


# ---- the emulators pass ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", B.STATS_KINDS)
@pytest.mark.parametrize("L", B.STATS_L)
def test_emulated_stats(L, kind):
    x = B.stats_case(L, kind)
    ref = B.stats_ref(x)
    for align in (0, 1):
        got = B.emulate_stats(x, align)
        ratios = B.check_stats(got, ref, f"L {L} {kind}")
        if kind == "const":
            assert not got[:, 2].any() and torch.equal(got[:, 1], x[:, 0])
    print(f"stats L {L} {kind}: " + ", ".join(f"{k} {v:.3f}" for k, v in ratios.items()))


@pytest.mark.parametrize("N,C,L", B.CHUNK_SHAPES)
def test_emulated_elementwise(N, C, L):
    c = B.ew_case(N, C, L)
    for align, mask_align in ((0, 0), (1, 0), (0, 1)):
        for with_res in (False, True):
            ref = B.apply_ref(c["x"], c["scale"], c["shift"], c["res"] if with_res else None)
            for relu in (False, True):
                y, mask, word = B.emulate_apply(c, with_res, relu, align=align, mask_align=mask_align, amax_prefill=0x7f7fffff)
                B.check_apply(y, mask, ref, relu, f"{(N, C, L)} apply")
                B.check_amax(word, y)
        for mode in B.MODES:
            ref = B.bwd_apply_ref(c, mode)
            for with_dres in (False, True):
                dx, dres, word = B.emulate_bwd_apply(c, mode, with_dres, align=align, mask_align=mask_align,
                                                     amax_prefill=0x7f7fffff)
                B.check_bwd_apply(dx, dres, ref, f"{(N, C, L)} mode {mode}")
                B.check_amax(word, dx)


@pytest.mark.parametrize("mode", B.MODES)
@pytest.mark.parametrize("N,C,L", B.REDUCE_SHAPES)
def test_emulated_bwd_reduce(N, C, L, mode):
    c = B.ew_case(N, C, L)
    ref = B.bwd_reduce_ref(c, mode)
    for align, mask_align in ((0, 0), (1, 0), (0, 1)):
        ratio = B.check_bound(B.emulate_bwd_reduce(c, mode, align, mask_align), ref, f"L {L} mode {mode}")
    print(f"bwd_reduce L {L} mode {mode}: {ratio:.3f}")


@pytest.mark.parametrize("width", [3, 2])
@pytest.mark.parametrize("C", B.FIN_C)
@pytest.mark.parametrize("P", B.FIN_P)
def test_emulated_finalize(P, C, width):
    for big in ((False, True) if width == 3 else (False,)):
        case = B.finalize_case(P, C, width, big)
        for momentum in B.FIN_MOMENTUM:
            got = B.emulate_finalize(case, momentum)
            B.check_finalize(got, B.finalize_ref(case, momentum), f"P {P} C {C} width {width} momentum {momentum}")
            if momentum <= 0:
                assert torch.equal(got["running_mean"], case["running_mean"]) and torch.equal(got["running_var"], case["running_var"])
    part, M = B.bwd_finalize_case(P, C)
    B.check_bound(B.emulate_bwd_finalize(part, M), B.bwd_finalize_ref(part, M), f"bwd_finalize P {P} C {C}")


@pytest.mark.parametrize("V", B.COLSUM_V)
@pytest.mark.parametrize("T", B.COLSUM_T)
def test_emulated_colsum(T, V):
    x = B.colsum_case(T, V)
    B.check_bound(B.emulate_colsum(x), B.colsum_ref(x), f"T {T} V {V}")
    _same(B.colsum_ref(x)[0], x.double().sum(1), "colsum")


@pytest.mark.parametrize("P", B.SUM_P)
def test_emulated_sum_leading(P):
    for M in B.SUM_M + B.SUM_M_TR64[:1]:
        inp = B.sum_case(P, M)
        B.check_bound(B.emulate_sum_leading(inp), B.sum_leading_ref(inp), f"P {P} M {M}")
        if M % 4096 == 0:
            B.check_bound(B.emulate_sum_leading(inp, True), B.sum_leading_ref(inp, True), f"P {P} M {M} tr64")


# ---- every mutant is caught ----------------------------------------------------------------------------------------------------
def _apply_mutant_catches(mutant, align=0):
    """how many of the chunked shapes reject `mutant` in bn_apply, and how many in bn_bwd_apply"""
    fwd = bwd = 0
    for N, C, L in B.CHUNK_SHAPES:
        c = B.ew_case(N, C, L)
        ref = B.apply_ref(c["x"], c["scale"], c["shift"], c["res"])
        y, mask, _ = B.emulate_apply(c, True, True, align=align, mutant=mutant)
        fwd += _caught(lambda: B.check_apply(y, mask, ref, True))
        dx, dres, _ = B.emulate_bwd_apply(c, 3, True, align=align, mutant=mutant)
        bwd += _caught(lambda: B.check_bwd_apply(dx, dres, B.bwd_apply_ref(c, 3)))
    return fwd, bwd


def _mutant_drop_tail():
    fwd, bwd = _apply_mutant_catches("drop_tail")
    assert fwd >= 3 and bwd >= 3, (fwd, bwd)        # 8197, 16389 and 35 end in a tail on a vector row
    hits = [L for L in B.STATS_L if L % 4 and L > 4 and _caught(
        lambda: B.check_stats(B.emulate_stats(B.stats_case(L), mutant="stats_tail"), B.stats_ref(B.stats_case(L))))]
    assert hits == [1023, 1025, 2051], hits
    hits = [L for _, _, L in B.REDUCE_SHAPES if L % 4 and L > 4 and _caught(
        lambda: B.check_bound(B.emulate_bwd_reduce(B.ew_case(2, 3, L), 3, mutant="reduce_tail"),
                              B.bwd_reduce_ref(B.ew_case(2, 3, L), 3)))]
    assert hits == [1023, 1025, 2051], hits
    return f"apply {fwd}, bwd_apply {bwd} of {len(B.CHUNK_SHAPES)} shapes; stats and bwd_reduce at L {hits}"


def _mutant_per_unrounded():
    fwd, bwd = _apply_mutant_catches("per_unrounded")
    assert fwd >= 2 and bwd >= 2, (fwd, bwd)        # 8197 and 16389: per = 4099 / 4098
    return f"apply {fwd}, bwd_apply {bwd} of {len(B.CHUNK_SHAPES)} shapes"


def _mutant_row_div_c():
    fwd, bwd = _apply_mutant_catches("row_div_c")
    assert fwd == bwd == len(B.CHUNK_SHAPES), (fwd, bwd)
    red = sum(_caught(lambda: B.check_bound(B.emulate_bwd_reduce(B.ew_case(N, C, L), 1, mutant="row_div_c"),
                                            B.bwd_reduce_ref(B.ew_case(N, C, L), 1)))
              for N, C, L in B.REDUCE_SHAPES)
    assert red == len(B.REDUCE_SHAPES), red
    return "every shape of apply, bwd_apply and bwd_reduce"


def _mutant_unpivoted():
    hits = [L for L in B.STATS_L if L > 1 and _caught(
        lambda: B.check_stats(B.emulate_stats(B.stats_case(L, "big"), mutant="unpivoted"), B.stats_ref(B.stats_case(L, "big"))))]
    assert hits == [L for L in B.STATS_L if L > 1], hits
    return f"the large-mean rows at L {hits}"


def _sum_catches(mutant, tr64, sizes):
    hits = []
    for P in B.SUM_P:
        for M in sizes:
            inp = B.sum_case(P, M)
            if _caught(lambda: B.check_bound(B.emulate_sum_leading(inp, tr64, mutant), B.sum_leading_ref(inp, tr64))):
                hits.append(P)
                break
    return hits


def _mutant_skip_remainder():
    hits = _sum_catches("skip_remainder", False, B.SUM_M[:2])
    small, rows = [P for P in hits if P < 32], [P for P in hits if P >= 32]
    assert small == [1, 7, 9, 31] and rows == [32, 33, 127, 129, 300], hits       # 8, 128, 256: no remainder
    return f"sum_leading_kernel at P {small}, sum_leading_rows_kernel at P {rows}"


def _mutant_tr64_plain():
    hits = _sum_catches("tr64_plain", True, B.SUM_M_TR64[:1])
    assert hits == list(B.SUM_P), hits
    return "every P"


def _mutant_stride_256():
    hits = [(T, V) for T in B.COLSUM_T for V in B.COLSUM_V if _caught(
        lambda: B.check_bound(B.emulate_colsum(B.colsum_case(T, V), "stride_256"), B.colsum_ref(B.colsum_case(T, V))))]
    assert set(hits) == {(5, 53), (39, 53), (5, 129), (39, 129), (5, 255), (39, 255)}, hits
    return f"(T, V) {hits}"


def _mutant_amax_not_cleared():
    c = B.ew_case(3, 5, 35)
    y, _, word = B.emulate_apply(c, True, True, amax_prefill=0x7f7fffff, mutant="amax_not_cleared")
    dx, _, dword = B.emulate_bwd_apply(c, 3, True, amax_prefill=0x7f7fffff, mutant="amax_not_cleared")
    assert _caught(lambda: B.check_amax(word, y)) and _caught(lambda: B.check_amax(dword, dx))
    assert _caught(lambda: B.check_amax(0x7f7fffff, torch.zeros(0)))        # N == 0 must leave 0
    B.check_amax(0, torch.zeros(0))
    return "apply_amax and bwd_apply_amax"


def _finalize_catches(mutant, width=3, momentum=0.1):
    hits = []
    for P in B.FIN_P:
        for C in B.FIN_C:
            case = B.finalize_case(P, C, width)
            if _caught(lambda: B.check_finalize(B.emulate_finalize(case, momentum, mutant=mutant), B.finalize_ref(case, momentum))):
                hits.append((P, C))
    return hits


def _mutant_merge_no_between():
    hits = _finalize_catches("merge_no_between")
    assert hits == [(P, C) for P in B.FIN_P[1:] for C in B.FIN_C], hits       # a single entry has nothing between
    return f"(P, C) {hits}"


def _mutant_biased_running_var():
    hits = _finalize_catches("biased_running_var") + _finalize_catches("biased_running_var", width=2, momentum=1.0)
    assert len(hits) == 2 * len(B.FIN_P) * len(B.FIN_C), hits
    assert not _finalize_catches("biased_running_var", momentum=-1.0)          # nothing is written then
    return "every (P, C), widths 3 and 2"


CATCHERS = {"drop_tail": _mutant_drop_tail, "per_unrounded": _mutant_per_unrounded, "row_div_c": _mutant_row_div_c,
            "unpivoted": _mutant_unpivoted, "skip_remainder": _mutant_skip_remainder, "tr64_plain": _mutant_tr64_plain,
            "stride_256": _mutant_stride_256, "amax_not_cleared": _mutant_amax_not_cleared,
            "merge_no_between": _mutant_merge_no_between, "biased_running_var": _mutant_biased_running_var}


@pytest.mark.parametrize("mutant", B.MUTANTS)
def test_mutant_is_caught(mutant):
    assert set(CATCHERS) == set(B.MUTANTS)
    print(f"MUTANT {mutant} caught: {CATCHERS[mutant]()}")


def test_the_stride_loop_of_the_merges_is_checked():
    """entries beyond the first 256 lost: caught from P = 257 on, in both finalisations"""
    hits = _finalize_catches("fin_first_trip")
    assert hits == [(P, C) for P in (257, 600) for C in B.FIN_C], hits
    for P in (257, 600):
        part, M = B.bwd_finalize_case(P, 3)
        assert _caught(lambda: B.check_bound(B.emulate_bwd_finalize(part, M, "fin_first_trip"), B.bwd_finalize_ref(part, M)))


def test_unwritten_elements_and_a_wrong_mask_byte_fail():
    c = B.ew_case(3, 5, 35)
    ref = B.apply_ref(c["x"], c["scale"], c["shift"], None)
    y, mask, _ = B.emulate_apply(c, False, True)
    B.check_apply(y, mask, ref, True)
    bad = mask.clone()
    bad[2, 4, 34] ^= 1
    with pytest.raises(AssertionError, match="mask byte"):
        B.check_apply(y, bad, ref, True)
    closed = (y == 0).nonzero()[0]
    leak = y.clone()
    leak[tuple(closed)] = 1e-3                                           # a closed gate far from the band reported open
    with pytest.raises(AssertionError, match="gate outside"):
        B.check_apply(leak, None, ref, True)
    leak[tuple(closed)] = -1e-6                                          # relu must not let a negative value through
    with pytest.raises(AssertionError, match="error / bound"):
        B.check_apply(leak, None, ref, True)
    dx, dres, _ = B.emulate_bwd_apply(c, 2, True)
    dres[0, 0, 0] += 1e-3
    with pytest.raises(AssertionError, match="dres"):
        B.check_bwd_apply(dx, dres, B.bwd_apply_ref(c, 2))
