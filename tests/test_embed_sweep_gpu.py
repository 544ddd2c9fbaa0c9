"""GPU: the kernels of the embedding MLPs (csrc/embed.hip, csrc/embed_bwd.hip, pw_bn_bwd_finalize, p2rnet/embed_op.py)
against the float64 references of tests/embed_cases.py.

Stage level, through the C entry points on NaN-filled outputs inside poisoned halos: p2r_embed_layer_backward over six
shapes (and one whose BatchNorm mean is 100 standard deviations from zero) x every workgroup count that changes how the
persistent loop runs (1, 2, 3, tiles - 1, tiles, tiles + 1, 512) x coef given / NULL x db_part given / NULL, its N == 0
and refused calls, p2r_pw_bn_bwd_finalize, the two forms of the 3 -> 64 weight gradient and the statistics of the 3 -> 64
forward at the workgroup edges.  Every stage is evaluated on the kernel's OWN fp32 inputs under the derived running-error
bounds of embed_cases.py; the comparison functions are the ones tests/test_embed_reference_cpu.py proves sensitive.

MLP level, through embed_op.embed_mlp with embed_op._N_BLOCKS at 1, 3 and the default 512 (1 and 3: every workgroup of
embed_bwd_kernel walks several tiles): the device's pre-activations z * scale + shift, read from what the op saved,
agree with the float64 chain within the forward tolerance, so every gate the device took differently lies in the band
the CPU test caps; the output and the running statistics against float64; every gradient against the float64 chain
evaluated WITH THE DEVICE'S GATES at the project's 1e-4 of max|ref|, with no slack for undecided elements and no masking.

Worst observed error / tolerance over the 36 MLP-level tests (one run on an MI355X; 1 would be at the limit):
  pre-activations (5e-5): y1 0.0031, y2 0.0085; 0 of 6,438,912 gates differed from the float64 chain's own
  output (5e-5) 0.0087; running mean / variance (2e-5): layer 0 0.0048 / 0.0041, layer 1 0.0044 / 0.0039
  gradients (1e-4): 0.conv.weight 0.0089, 0.batchnorm.weight 0.0093, 0.batchnorm.bias 0.0084, 1.conv.weight 0.0202,
  1.batchnorm.weight 0.0057, 1.batchnorm.bias 0.0044, 2.conv.weight 0.0145, 2.conv.bias 0.0022, d_add 0.0014
so the borrowed 1e-4 has a headroom of about 50.  Stage level, worst error / derived bound over the 184 calls of
p2r_embed_layer_backward: g_prev 0.073, S1 0.0046, S2 0.0050, dW 0.049, db 0.016.
"""
import copy
import functools

import pytest
import torch

from tests import embed_cases as E
from tests import memguard

pytestmark = pytest.mark.gpu

EINVAL = "failed with status -22"
F32 = torch.float32


def _nan_buffer(shape, dev):
    """(buf, view): a NaN-filled output inside a NaN halo (the poison of memguard is a quiet NaN)"""
    return memguard.guarded(shape, F32, dev, fill="poison", halo="poison")


def _intact(*pairs):
    for buf, view in pairs:
        assert int(memguard.halo_damage(buf, view, "poison")) == 0, "written outside the buffer"


# ---- p2r_embed_layer_backward ------------------------------------------------------------------------------------------------
LAYER_CASES = [(N, L, False) for N, L in E.LAYER_SHAPES] + [E.BIG_MEAN_SHAPE + (True,)]
LAYER_SWEEP = [(N, L, big, nb) for N, L, big in LAYER_CASES for nb in E.n_blocks_of(N, L)]
LAYER_IDS = [f"{N}x{L}{'_bigmean' if big else ''}-nb{nb}" for N, L, big, nb in LAYER_SWEEP]


@functools.lru_cache(maxsize=None)
def _layer_ref(N, L, big, lazy):
    c = E.layer_case(N, L, big)
    return E.layer_backward_ref(c["g"], c["z"], c["coef"] if lazy else None, c["zp"], c["fin"], c["W"])


@functools.lru_cache(maxsize=None)
def _layer_inputs(dev, N, L, big):
    return {k: v.to(dev) for k, v in E.layer_case(N, L, big).items()}


def _layer_call(dev, N, L, d, lazy, with_db, nb, **over):
    from pose2room_amd import _lib
    out = {"g_prev": _nan_buffer((max(N, 1), E.C, L), dev), "sums": _nan_buffer((nb, E.C, 2), dev),
           "dw_part": _nan_buffer((nb, E.C, E.C), dev), "db_part": _nan_buffer((nb, E.C), dev) if with_db else None}
    a = dict(g=d["g"], z=d["z"] if lazy else None, coef=d["coef"] if lazy else None, n_blocks=nb)
    a.update(over)
    view = lambda k: None if out[k] is None else out[k][1]
    try:
        _lib.launch("p2r_embed_layer_backward", dev, N, L, a["g"], a["z"], a["coef"], d["zp"], d["fin"], d["W"],
                    view("g_prev"), view("sums"), a["n_blocks"], view("dw_part"), view("db_part"))
    finally:
        torch.cuda.synchronize()
        _intact(*[p for p in out.values() if p is not None])
    return {k: None if p is None else p[1].cpu() for k, p in out.items()}


@pytest.mark.parametrize("with_db", [True, False], ids=["db", "nodb"])
@pytest.mark.parametrize("lazy", [True, False], ids=["coef", "nocoef"])
@pytest.mark.parametrize("N,L,big,nb", LAYER_SWEEP, ids=LAYER_IDS)
def test_layer_backward(dev, N, L, big, nb, lazy, with_db):
    got = _layer_call(dev, N, L, _layer_inputs(dev, N, L, big), lazy, with_db, nb)
    ratios = E.check_layer_backward(got, _layer_ref(N, L, big, lazy), f"{N}x{L} n_blocks {nb}")
    assert ("db" in ratios) == with_db
    print("RATIO layer " + " ".join(f"{k} {v:.4f}" for k, v in ratios.items()))


@pytest.mark.parametrize("nb", [1, 4])
def test_layer_backward_of_an_empty_batch_zeroes_every_partial_row(dev, nb):
    """N == 0: no kernel runs, so the host must leave all n_blocks rows of the three partial buffers zero"""
    got = _layer_call(dev, 0, 64, _layer_inputs(dev, 1, 64, False), True, True, nb)
    for k in ("sums", "dw_part", "db_part"):
        assert got[k].shape[0] == nb and not torch.isnan(got[k]).any() and not got[k].any(), k
    assert torch.isnan(got["g_prev"]).all()                             # (0,64,L) is empty: nothing to write


def test_layer_backward_refusals_write_nothing(dev):
    d = _layer_inputs(dev, 2, 192, False)
    shifted = memguard.guarded((2, E.C, 192), F32, dev, fill=E.layer_case(2, 192)["g"], halo="zero", offset_bytes=4)[1]
    for over in ({"n_blocks": 0}, {"z": None}, {"g": shifted}):
        with pytest.raises(RuntimeError, match="p2r_embed_layer_backward " + EINVAL):
            _layer_call(dev, 2, 192, d, True, True, 4, **over)
    from pose2room_amd import _lib
    g_prev, sums, dw = (_nan_buffer(s, dev)[1] for s in ((2, E.C, 192), (4, E.C, 2), (4, E.C, E.C)))
    with pytest.raises(RuntimeError, match="p2r_embed_layer_backward " + EINVAL):       # L % 64 != 0
        _lib.launch("p2r_embed_layer_backward", dev, 2, 96, d["g"], d["z"], d["coef"], d["zp"], d["fin"], d["W"], g_prev,
                    sums, 4, dw, None)
    torch.cuda.synchronize()
    assert all(torch.isnan(t).all() for t in (g_prev, sums, dw))


# ---- p2r_pw_bn_bwd_finalize on embedding-shaped jobs ---------------------------------------------------------------------------
@pytest.mark.parametrize("train", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("P", [1, 3, 512])
def test_bn_bwd_finalize(dev, P, train):
    from pose2room_amd import _lib
    from pose2room_amd.p2rnet import pw_op
    part, fin, M = E.finalize_case(P)
    cbuf, coef = _nan_buffer((3, E.C), dev)
    with torch.cuda.device(dev):
        (dg, db), = pw_op._bn_bwd_finalize([part.to(dev)], fin.to(dev), coef, [0], [E.C], M, train,
                                           _lib.current_stream(dev))
    torch.cuda.synchronize()
    _intact((cbuf, coef))
    S = part.double().sum(0)
    ratios = E.check_bn_bwd_coef({"coef": coef.cpu(), "dgamma": dg.cpu(), "dbeta": db.cpu()},
                                 E.bn_bwd_coef_ref(S[:, 0], S[:, 1], fin, M, train), f"P {P}")
    if not train:
        assert torch.equal(coef[0].cpu(), fin[2]) and not coef[1:].any()
    print("RATIO finalize " + " ".join(f"{k} {v:.4f}" for k, v in ratios.items()))


# ---- the 3 -> 64 layer -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lazy", [True, False], ids=["lazy", "plain"])
@pytest.mark.parametrize("L", E.WGRAD_L)
@pytest.mark.parametrize("N", E.WGRAD_N)
def test_embed3_weight_grad(dev, N, L, lazy):
    from pose2room_amd import _lib
    c = E.wgrad_case(N, L)
    d = {k: v.to(dev) for k, v in c.items()}
    buf, part = _nan_buffer((N * E.C, 4), dev)
    if lazy:
        _lib.launch("p2r_embed3_weight_grad_lazy", dev, N, L, d["x"], d["g"], d["z"], d["coef"], part)
    else:
        _lib.launch("p2r_embed3_weight_grad", dev, N, L, d["x"], d["g"], part)
    torch.cuda.synchronize()
    _intact((buf, part))
    ref = E.embed3_wgrad_ref(c["x"], c["g"], c["z"] if lazy else None, c["coef"] if lazy else None)
    ratio = E.check_embed3_wgrad(part.cpu(), ref, f"{N}x{L}")
    print(f"RATIO wgrad all {ratio:.4f}")


def test_embed3_weight_grad_lazy_refusals_and_empty(dev):
    from pose2room_amd import _lib
    d = {k: v.to(dev) for k, v in E.wgrad_case(1, 7).items()}
    part = _nan_buffer((E.C, 4), dev)[1]
    for z, coef in ((None, d["coef"]), (d["z"], None)):
        with pytest.raises(RuntimeError, match="p2r_embed3_weight_grad_lazy " + EINVAL):
            _lib.launch("p2r_embed3_weight_grad_lazy", dev, 1, 7, d["x"], d["g"], z, coef, part)
    _lib.launch("p2r_embed3_weight_grad_lazy", dev, 0, 7, d["x"], d["g"], d["z"], d["coef"], part)      # N = 0: nothing to do
    torch.cuda.synchronize()
    assert torch.isnan(part).all()


STATS_CASES = [(2, L, off, False) for L in E.STATS_L for off in (0.0, 50.0)] + [(2, 1025, 50.0, True), (1, 1, 0.0, False)]


@pytest.mark.parametrize("B,L,off,constant", STATS_CASES)
def test_embed3_statistics_at_the_workgroup_edges(dev, B, L, off, constant):
    """tolerances of test_pw_gpu.py::test_embed3_statistics_from_input_moments: mean 1e-6, variance 1e-5 of the largest;
    a constant input: every output equals its channel's mean, so the variance must be non-negative and below the square of
    what fp32 resolves of the output, (u sum_d |W_cd| |x_d|)^2"""
    from pose2room_amd.p2rnet import bn_op, tconv_op
    x, W, b = E.stats_case(B, L, off, constant)
    conv = torch.nn.Conv1d(3, E.C, 1)
    with torch.no_grad():
        conv.weight.copy_(W[:, :, None]), conv.bias.copy_(b)
    out, stats = tconv_op.embed3(x.to(dev), conv.to(dev), want_stats=True)
    (want, bound), mean_ref, var_ref = E.embed3_stats_ref(x, W, b)
    ratio, at = E.worst(out.detach().cpu(), want, bound)
    assert ratio <= 1, (ratio, at)
    assert stats.shape == (1, E.C, 3) and (stats[0, :, 0] == B * L).all()
    mean, var, _ = bn_op.moments(stats, B * L)
    mean, var = mean.cpu(), var.cpu()
    assert E.rel_err(mean, mean_ref) < 1e-6
    assert (var >= 0).all()
    if constant or B * L == 1:
        resolved = (E.U * torch.einsum("cd,d->c", W.double().abs(), x[0, :, 0].double().abs())) ** 2
        assert (var <= resolved).all(), (var.max().item(), resolved.min().item())
    else:
        assert E.rel_err(var, var_ref) < 1e-5
    print(f"RATIO embed3 out {ratio:.4f} mean {E.rel_err(mean, mean_ref) / 1e-6:.4f} "
          f"var {0.0 if constant or B * L == 1 else E.rel_err(var, var_ref) / 1e-5:.4f}")


# ---- the whole MLP ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _chain(case, train):
    """the float64 chain with its own gates, once per case and mode"""
    seq, x, pe, dout = E.mlp_case(*case)
    return E.mlp_ref(x, *E.mlp_inputs(seq), train, case[2], pe, dout)


def _mlp_run(dev, case, train, n_blocks, douts):
    """one forward of embed_op.embed_mlp and one backward per entry of `douts` (device tensors) with
    embed_op._N_BLOCKS = n_blocks -> (out, saved stage tensors, module, [gradients per backward])"""
    from pose2room_amd.p2rnet import embed_op
    seq, x, pe, _ = E.mlp_case(*case)
    mod = copy.deepcopy(seq).to(dev).train(train)
    xd = x.to(dev)
    ped = pe.to(dev).requires_grad_(True) if pe is not None else None
    assert embed_op.supported(mod, xd, case[2], ped)
    grads = []
    default = embed_op._N_BLOCKS
    embed_op._N_BLOCKS = n_blocks
    try:
        out = embed_op.embed_mlp(mod, xd, case[2], ped)
        saved = [t.detach().cpu() for t in E.saved_stage_tensors(out)]
        for i, dout in enumerate(douts):
            mod.zero_grad(set_to_none=True)
            if ped is not None:
                ped.grad = None
            out.backward(dout, retain_graph=i + 1 < len(douts))
            g = {k: p.grad.detach().cpu().clone() for k, p in mod.named_parameters()}
            g["d_add"] = ped.grad.detach().cpu().clone() if ped is not None else None
            grads.append(g)
        torch.cuda.synchronize()
    finally:
        embed_op._N_BLOCKS = default
    return out.detach().cpu(), saved, mod, grads


@pytest.mark.parametrize("n_blocks", [1, 3, 512])
@pytest.mark.parametrize("train", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("case", E.MLP_CASES, ids=["x".join(str(int(v)) for v in c) for c in E.MLP_CASES])
def test_mlp_against_float64_with_device_gates(dev, case, train, n_blocks):
    seq, x, pe, dout = E.mlp_case(*case)
    params, buffers = E.mlp_inputs(seq)
    out, (z1, z2, fin1, fin2), mod, (grads,) = _mlp_run(dev, case, train, n_blocks, [dout.to(dev)])
    ref = _chain(case, train)
    ratios = {}
    # 1. the device's pre-activations against the chain's: a gate taken differently lies inside the capped band
    gates = []
    for name, z, fin in (("y1", z1, fin1), ("y2", z2, fin2)):
        assert z.shape == ref[name].shape and fin.shape == (4, E.C)
        y_dev = z.double() * E._c(fin[2].double()) + E._c(fin[3].double())
        ratios[name] = E.rel_err(y_dev, ref[name]) / E.FWD_TOL
        gates.append(y_dev > 0)
        differ = gates[-1] != (ref[name] > 0)
        print(f"{name}: {int(differ.sum())} of {differ.numel()} gates differ from the chain's own")
        assert not (differ & (ref[name].abs() > E.FWD_TOL * ref[name].abs().max())).any(), name
    # 2. output and running statistics against float64
    ratios["out"] = E.rel_err(out, ref["out"]) / E.FWD_TOL
    sd = mod.state_dict()
    for k in E.BUFFERS:
        if train:
            ratios[k] = E.rel_err(sd[k].cpu(), ref["running"][k]) / E.STAT_TOL
        else:
            assert torch.equal(sd[k].cpu(), buffers[k]), k
    # 3. every gradient against the chain run with the device's gates
    want = E.mlp_ref(x, params, buffers, train, case[2], pe, dout, gates=gates)
    for k in E.PARAMS:
        assert grads[k].shape == params[k].shape and grads[k].dtype == F32, k
        ratios["grad " + k] = E.rel_err(grads[k], want["grads"][k].reshape(params[k].shape)) / E.GRAD_TOL
    if pe is not None:
        ratios["d_add"] = E.rel_err(grads["d_add"], want["d_add"]) / E.GRAD_TOL
    else:
        assert grads["d_add"] is None
    print("RATIO mlp " + " ".join(f"{k.replace(' ', '_')} {v:.4f}" for k, v in ratios.items()))
    for k, v in ratios.items():
        assert v <= 1, f"{k}: error / tolerance {v:.3f}"


@pytest.mark.parametrize("train", [True, False], ids=["train", "eval"])
def test_mlp_backward_takes_a_misaligned_output_gradient(dev, train):
    """a contiguous gradient that starts 4 bytes into its storage: the backward copies it for the kernel's 16-byte loads and
    computes the bits of the aligned run (same forward, two backwards)"""
    case = E.MLP_CASES[0]
    assert not case[3]
    dout = E.mlp_case(*case)[3].to(dev)
    store = torch.empty(dout.numel() + 1, dtype=F32, device=dev)
    shifted = store[1:].view(dout.shape)
    shifted.copy_(dout)
    assert dout.data_ptr() % 16 == 0 and shifted.data_ptr() % 16 == 4 and shifted.is_contiguous()
    _, _, _, (aligned, moved) = _mlp_run(dev, case, train, 512, [dout, shifted])
    for k in E.PARAMS:
        assert torch.equal(aligned[k], moved[k]) and aligned[k].abs().max() > 0, k
