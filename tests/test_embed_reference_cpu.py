"""CPU: the float64 references of the embedding MLPs (tests/embed_cases.py) against float64 autograd of the same stage and
against the module chain, the conditions on the cases that the GPU sweep (tests/test_embed_sweep_gpu.py) relies on, and
the sensitivity of the comparison functions both tests share.

The hand-written stage references must equal autograd to float64 rounding: a wrong formula in a reference would
otherwise be "confirmed" by a kernel with the same mistake.  The conditions are asserted here so that the GPU test
cannot hide behind them: no stage-level case holds an element whose gate fp32 rounding could turn, and at most 1e-3 of
the pre-activations of an MLP-level case lie within the project's forward tolerance (5e-5 max|y|) of zero.  A failure
of a condition means the case (its seed) is wrong, not the kernel.

Sensitivity: an fp32 torch emulation of embed_bwd_kernel's work split (64-column tiles dealt to n_blocks workgroups,
per-workgroup partial rows) passes `check_layer_backward` under the derived bounds, and each of six defects the
persistent loop could have fails it; the same for the 3 -> 64 weight gradient.  What is proven here about the checks
holds on the GPU, which calls the same functions.
"""
import copy

import pytest
import torch

from tests import embed_cases as E

F64 = 1e-12     # float64 rounding of sums over at most 2048 x 64 terms, relative to the largest element


def _same(a, b, what, tol=F64):
    assert a.shape == b.shape, what
    assert (a - b).abs().max() <= tol * (b.abs().max() + 1e-300), (what, (a - b).abs().max().item())


LAYER_CASES = [(N, L, False) for N, L in E.LAYER_SHAPES] + [E.BIG_MEAN_SHAPE + (True,)]
LAYER_IDS = [f"{N}x{L}{'_bigmean' if big else ''}" for N, L, big in LAYER_CASES]


# ---- stage references against float64 autograd ------------------------------------------------------------------------------
@pytest.mark.parametrize("lazy", [True, False], ids=["coef", "nocoef"])
@pytest.mark.parametrize("N,L,big", LAYER_CASES, ids=LAYER_IDS)
def test_layer_backward_ref_is_autograd(N, L, big, lazy):
    """g_prev, dW, db are the gradients of sum(dz * (W relu(bn(zp)) + b)) with respect to the BatchNorm's output, W, b;
    S1, S2 the BatchNorm-backward sums of g_prev"""
    c = E.layer_case(N, L, big)
    coef = c["coef"] if lazy else None
    ref = E.layer_backward_ref(c["g"], c["z"], coef, c["zp"], c["fin"], c["W"])
    g, z, zp, fin = c["g"].double(), c["z"].double(), c["zp"].double(), c["fin"].double()
    dz = g if coef is None else E._c(coef[0].double()) * g + E._c(coef[1].double()) * z + E._c(coef[2].double())
    y = (zp * E._c(fin[2]) + E._c(fin[3])).requires_grad_(True)
    W, b = c["W"].double().requires_grad_(True), torch.zeros(E.C, dtype=torch.float64, requires_grad=True)
    u = torch.nn.functional.conv1d(torch.relu(y), W[:, :, None], b)
    u.backward(dz)
    _same(ref["g_prev"][0], y.grad, "g_prev")
    _same(ref["dW"][0], W.grad, "dW")
    _same(ref["db"][0], b.grad, "db")
    _same(ref["S1"][0], y.grad.sum((0, 2)), "S1")
    _same(ref["S2"][0], (y.grad * (zp - E._c(fin[0])) * E._c(fin[1])).sum((0, 2)), "S2")
    assert torch.equal(ref["gate"], y > 0) and 0.2 < ref["gate"].double().mean() < 0.8
    for k in ("S1", "S2", "dW", "db"):
        _, fixed, mag, _ = ref[k]
        assert (fixed >= 0).all() and (mag >= ref[k][0].abs() * (1 - 1e-9)).all(), k
    assert (ref["g_prev"][1][~ref["gate"]] == 0).all()
    # the one-line form of the docstring: three roundings, a product, 64 additions
    if lazy:
        mag = torch.einsum("oi,nol->nil", c["W"].double().abs(), ref["dz"][1] / E.gamma(3)) * ref["gate"]
        assert (ref["g_prev"][1] <= E.gamma(68) * mag * (1 + 1e-9)).all()


@pytest.mark.parametrize("train", [True, False], ids=["train", "eval"])
def test_bn_coef_ref_is_the_batchnorm_backward(train):
    """a g + b z + c with the reference's constants is autograd's gradient of BatchNorm (batch statistics in training
    mode, fixed statistics in evaluation mode); dgamma and dbeta are its parameter gradients"""
    c = E.layer_case(2, 192)
    z, g = c["z"].double().requires_grad_(True), c["g"].double()
    M = z.shape[0] * z.shape[2]
    gam = torch.linspace(0.5, 1.5, E.C, dtype=torch.float64).requires_grad_(True)
    bet = torch.zeros(E.C, dtype=torch.float64, requires_grad=True)
    mean, var = z.mean((0, 2)), z.var((0, 2), unbiased=False)
    if not train:
        mean, var = mean.detach() + 0.1, var.detach() * 1.3
    invstd = (var + 1e-5).rsqrt()
    xhat = (z - E._c(mean)) * E._c(invstd)
    (xhat * E._c(gam) + E._c(bet)).backward(g)
    fin = torch.stack([mean, invstd, gam * invstd, bet - mean * gam * invstd]).detach()
    ref = E.bn_bwd_coef_ref(g.sum((0, 2)), (g * xhat.detach()).sum((0, 2)), fin, M, train)
    a, b, cc = (E._c(ref["coef"][0][i]) for i in range(3))
    _same(a * g + b * z.detach() + cc, z.grad, "dz")
    _same(ref["dgamma"][0], gam.grad, "dgamma")
    _same(ref["dbeta"][0], bet.grad, "dbeta")
    if not train:
        assert not ref["coef"][0][1:].any() and not ref["coef"][1].any()


@pytest.mark.parametrize("lazy", [True, False], ids=["coef", "nocoef"])
@pytest.mark.parametrize("N,L", [(1, 7), (3, 1030)])
def test_embed3_wgrad_ref_is_autograd(N, L, lazy):
    c = E.wgrad_case(N, L)
    z, coef = (c["z"], c["coef"]) if lazy else (None, None)
    value, bound = E.embed3_wgrad_ref(c["x"], c["g"], z, coef)
    g = c["g"].double()
    dz = g if not lazy else E._c(coef[0].double()) * g + E._c(coef[1].double()) * z.double() + E._c(coef[2].double())
    for n in range(N):       # per sample: the kernel leaves the sum over samples to its caller
        W = torch.zeros(E.C, 3, 1, dtype=torch.float64, requires_grad=True)
        b = torch.zeros(E.C, dtype=torch.float64, requires_grad=True)
        torch.nn.functional.conv1d(c["x"][n:n + 1].double(), W, b).backward(dz[n:n + 1])
        _same(value[n * E.C:(n + 1) * E.C, :3], W.grad[:, :, 0], "dW")
        _same(value[n * E.C:(n + 1) * E.C, 3], b.grad, "db")
    assert (bound > 0).all()


def test_embed3_stats_ref_is_conv1d():
    x, W, b = E.stats_case(2, 1025, 50.0)
    (out, bound), mean, var = E.embed3_stats_ref(x, W, b)
    _same(out, torch.nn.functional.conv1d(x.double(), W.double()[:, :, None], b.double()), "out")
    bn = torch.nn.BatchNorm1d(E.C, momentum=1.0, affine=False).double()
    bn(out)
    _same(mean, bn.running_mean, "mean")
    _same(var * (2 * 1025 / (2 * 1025 - 1)), bn.running_var, "var")
    assert ((torch.nn.functional.conv1d(x, W[:, :, None], b).double() - out).abs() <= bound).all()


# ---- mlp_ref against the module chain ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("train", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("B,rows,inner,add", [E.MLP_CASES[1], E.MLP_CASES[3]])
def test_mlp_ref_is_the_module_chain(B, rows, inner, add, train):
    seq, x, pe, dout = E.mlp_case(B, rows, inner, add)
    params, buffers = E.mlp_inputs(seq)
    got = E.mlp_ref(x, params, buffers, train, inner, pe, dout)
    want = E.module_chain_ref(seq, x, pe, inner, dout, train)
    _same(got["out"], want["out"], "out")
    assert set(got["grads"]) == set(want["grads"]) == set(E.PARAMS)
    for k in E.PARAMS:
        _same(got["grads"][k], want["grads"][k], k, 1e-10)
    for k in E.BUFFERS:
        _same(got["running"][k], want["running"][k], k)
        assert train != torch.equal(got["running"][k], buffers[k].double()), k
    if add:
        _same(got["d_add"], want["d_add"], "d_add")
    else:
        assert got["d_add"] is None
    # its own gates given back as constants: the same run
    again = E.mlp_ref(x, params, buffers, train, inner, pe, dout, gates=(got["y1"] > 0, got["y2"] > 0))
    for k in E.PARAMS:
        assert torch.equal(again["grads"][k], got["grads"][k]), k
    # and a gate that is turned moves a gradient: the argument is not ignored
    flipped = E.mlp_ref(x, params, buffers, train, inner, pe, dout, gates=(got["y1"] > 0, got["y2"] > 1e-2))
    assert not torch.equal(flipped["grads"]["2.conv.weight"], got["grads"]["2.conv.weight"])


# ---- input conditions ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,L,big", LAYER_CASES, ids=LAYER_IDS)
def test_layer_cases_hold_no_undecided_gate(N, L, big):
    c = E.layer_case(N, L, big)
    assert N * L <= 2048 and L % 64 == 0 and (N * L) ** 2 * E.U <= 0.25
    assert c["zp"].shape == c["g"].shape == c["z"].shape == (N, E.C, L)
    assert int(E.gate_band(c["zp"], c["fin"]).sum()) == 0
    mean, std = c["zp"].double().mean((0, 2)), c["zp"].double().std((0, 2))
    assert ((c["fin"][0].double() - mean).abs() <= 1e-5 * (1 + mean.abs())).all()       # fin is zp's own BatchNorm
    ratio = (mean.abs() / std)
    assert (ratio.min() > 30 and ratio.max() < 300) if big else ratio.max() < 5
    assert 0.3 < (c["g"] == 0).double().mean() < 0.7


def test_sweep_workgroup_counts():
    assert E.n_blocks_of(1, 64) == [1, 2, 3, 512]
    assert E.n_blocks_of(2, 192) == [1, 2, 3, 5, 6, 7, 512]
    assert E.n_blocks_of(1, 2048) == [1, 2, 3, 31, 32, 33, 512]
    assert E.LAYER_SHAPES == [(1, 64), (5, 64), (2, 192), (3, 128), (1, 2048), (2, 1024)]
    assert E.MLP_CASES == [(1, 16, 20, False), (2, 16, 20, True), (2, 64, 53, True), (3, 1, 64, False), (5, 1, 64, True),
                           (2, 16, 4, False)]
    assert E.WGRAD_L == (7, 64, 1028, 1030, 2048) and E.STATS_L == (1, 1023, 1024, 1025, 2049)


@pytest.mark.parametrize("train", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("B,rows,inner,add", E.MLP_CASES)
def test_mlp_cases_band_share(B, rows, inner, add, train):
    seq, x, pe, dout = E.mlp_case(B, rows, inner, add)
    assert (rows * inner) % 64 == 0 and x.shape == (B, 3, rows * inner)
    ref = E.mlp_ref(x, *E.mlp_inputs(seq), train, inner, pe, dout)
    for k in ("y1", "y2"):
        share = E.band_share(ref[k])
        print(f"{(B, rows, inner, add)} {'train' if train else 'eval'} {k}: share within 5e-5 max|y| of zero {share:.2e}")
        assert share <= E.BAND_CAP, (k, share)
        assert 0.1 < (ref[k] > 0).double().mean() < 0.9, k


# ---- sensitivity of check_layer_backward ---------------------------------------------------------------------------------------
EMU = [(2, 192, False, 2), (1, 2048, False, 3), (5, 64, True, 1), (3, 128, False, 512)]     # N, L, big mean, n_blocks


def _layer_ref(N, L, big, lazy):
    c = E.layer_case(N, L, big)
    return c, E.layer_backward_ref(c["g"], c["z"], c["coef"] if lazy else None, c["zp"], c["fin"], c["W"])


@pytest.mark.parametrize("lazy", [True, False], ids=["coef", "nocoef"])
@pytest.mark.parametrize("N,L,big", LAYER_CASES, ids=LAYER_IDS)
def test_emulated_work_split_passes(N, L, big, lazy):
    c, ref = _layer_ref(N, L, big, lazy)
    for nb in E.n_blocks_of(N, L):
        for with_db in (True, False):
            ratios = E.check_layer_backward(E.emulate_layer_backward(c, nb, lazy, with_db), ref, f"n_blocks {nb}")
            assert ("db" in ratios) == with_db
    print(f"{N}x{L} n_blocks {nb}: worst error / bound " + ", ".join(f"{k} {v:.3f}" for k, v in ratios.items()))


@pytest.mark.parametrize("mutant", E.MUTANTS)
@pytest.mark.parametrize("N,L,big,nb", EMU)
def test_mutants_of_the_work_split_fail(N, L, big, nb, mutant):
    c, ref = _layer_ref(N, L, big, True)
    E.check_layer_backward(E.emulate_layer_backward(c, nb), ref)
    tiles = N * L // E.COLS
    if mutant == "stale_zp" and nb >= tiles:
        nb = 1                                  # the defect needs a workgroup with a second tile
    got = E.emulate_layer_backward(c, nb, mutant=mutant)
    with pytest.raises(AssertionError, match="error / bound|gate is closed"):
        E.check_layer_backward(got, ref)


def test_unwritten_and_stray_rows_fail():
    c, ref = _layer_ref(2, 192, False, True)
    got = E.emulate_layer_backward(c, 512)
    got["dw_part"][6, 3, 3] = 1e-30                                     # a row beyond the six workgroups
    with pytest.raises(AssertionError, match="beyond"):
        E.check_layer_backward(got, ref)
    got = E.emulate_layer_backward(c, 2)
    got["g_prev"][1, 63, 191] = float("nan")
    with pytest.raises(AssertionError, match="NaN"):
        E.check_layer_backward(got, ref)


# ---- sensitivity of check_embed3_wgrad --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lazy", [True, False], ids=["coef", "nocoef"])
@pytest.mark.parametrize("L", E.WGRAD_L)
@pytest.mark.parametrize("N", E.WGRAD_N)
def test_emulated_wgrad_passes_and_mutants_fail(N, L, lazy):
    c = E.wgrad_case(N, L)
    ref = E.embed3_wgrad_ref(c["x"], c["g"], c["z"] if lazy else None, c["coef"] if lazy else None)
    E.check_embed3_wgrad(E.emulate_embed3_wgrad(c, lazy), ref)
    if L % 4:
        with pytest.raises(AssertionError, match="error / bound"):
            E.check_embed3_wgrad(E.emulate_embed3_wgrad(c, lazy, "drop_tail"), ref)
    if lazy:
        with pytest.raises(AssertionError, match="error / bound"):
            E.check_embed3_wgrad(E.emulate_embed3_wgrad(c, lazy, "drop_c"), ref)


def test_bn_coef_check_rejects_a_swapped_sum():
    part, fin, M = E.finalize_case(3)
    S = part.double().sum(0)
    ref = E.bn_bwd_coef_ref(S[:, 0], S[:, 1], fin, M, True)
    good = {"coef": ref["coef"][0].float(), "dgamma": ref["dgamma"][0].float(), "dbeta": ref["dbeta"][0].float()}
    E.check_bn_bwd_coef(good, ref)
    swapped = E.bn_bwd_coef_ref(S[:, 1], S[:, 0], fin, M, True)
    with pytest.raises(AssertionError, match="error / bound"):
        E.check_bn_bwd_coef(dict(good, coef=swapped["coef"][0].float()), ref)


def test_saved_stage_tensors_of_a_function_that_returns_a_view():
    """the access the GPU test uses, on a CPU Function of the op's shape: forward saves eight tensors and returns a view"""
    class F(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x, w):
            z1, z2 = x * 2, x * 3
            ctx.save_for_backward(x, z1, z2, z1[:4], z2[:4], w, w, w)
            return (x * w).view(-1)

        @staticmethod
        def backward(ctx, g):
            return None, g.sum().expand(1)

    x, w = torch.arange(6.0), torch.ones(1, requires_grad=True)
    z1, z2, f1, f2 = E.saved_stage_tensors(F.apply(x, w))
    assert torch.equal(z1, x * 2) and torch.equal(z2, x * 3) and torch.equal(f1, z1[:4]) and torch.equal(f2, z2[:4])
    assert copy.copy(E.GRAD_TOL) == 1e-4 and E.FWD_TOL == 5e-5 and E.STAT_TOL == 2e-5
