"""GPU: the BatchNorm and partial-sum kernels (csrc/bn_act.hip, p2rnet/bn_op.py) against the float64 references of
tests/bn_cases.py.

Stage level, through the C entry points on poison-filled outputs inside poisoned halos (halos intact, no element left
unwritten): p2r_bn_stats over the row lengths at the edges of its 1024-element trips (plain, |mean| / std = 1000 and
constant rows); p2r_bn_apply (relu x residual), p2r_bn_bwd_reduce (4 mask modes) and p2r_bn_bwd_apply (4 modes x dres
given / NULL) over the chunked shapes -- one chunk just below the threshold, two chunks, two and four chunks with a ragged
last one -- with every tensor 16-byte aligned, 4 bytes past that, and with the mask bytes 1 byte past a 4-byte boundary;
p2r_bn_apply_amax / p2r_bn_bwd_apply_amax (same bits as the plain entry points, the word is the exact maximum and is
cleared first); p2r_bn_finalize (widths 3 and 2, P across the 256-entry stride, four momenta, step counter given / NULL)
and p2r_bn_bwd_finalize; p2r_colsum at every shape of lanes_used; p2r_sum_leading, both kernels, plain and tr64, each
call twice; the refused calls (-22, nothing written) and the empty ones.  Every stage is evaluated on the kernel's OWN
fp32 inputs under the derived running-error bounds; the comparison functions are the ones
tests/test_bn_reference_cpu.py proves sensitive.

Op level, through bn_op.fused_bn_act: relu x residual x train / eval over four shapes (one 3-D, one that chunks), every
gradient against the float64 chain evaluated WITH THE DEVICE'S GATES at the project's tolerances, no element masked out;
momentum=None, stats= of both widths, a non-contiguous input, split16's range words.

Worst observed error / derived bound per stage (one run on an MI355X; 1 would be at the limit):
  bn_stats (48 calls): mean 0.66, M2 0.081;  bn_apply (80): 0.99 -- the bound is the single rounding of the fused
  multiply-add, half an ulp reaches it;  bn_bwd_reduce (72): 0.10;  bn_bwd_apply (90): dx 0.84
  bn_finalize (180): constants 0.96 (one rounding), running mean 0.60, running variance 0.62;  bn_bwd_finalize (15): 0.99
  colsum (18): 0.33;  sum_leading (60): 0.29, tr64 (24): 0.37
Op level, worst error / tolerance over the 34 runs that go through `_check_op`:
  y (1e-5, 1e-5) 0.081; running mean / variance (1e-5, 1e-6) 0.017 / 0.026; dx (1e-4, 1e-5) 0.0096;
  dgamma / dbeta (1e-4 of max |ref|) 0.0019 / 0.0029; 0 of 571,916 gates differed from the float64 chain's own
  momentum=None, two calls: running mean / variance 0.016 / 0.010
so the borrowed tolerances have a headroom of 12 (y) to 500 (dgamma), while the derived stage bounds have almost none.
"""
import functools

import pytest
import torch

from tests import bn_cases as B
from tests import memguard

pytestmark = pytest.mark.gpu

EINVAL = "failed with status -22"
F32 = torch.float32
PREFILL = 0x7f7fffff          # what an amax word holds before the call: the entry point must clear it
ALIGNMENTS = [(0, 0), (1, 0), (0, 1)]     # (float tensors: elements past a 16-byte boundary, mask: bytes past a 4-byte one)


def _out(shape, dev, dtype=F32, offset_bytes=0):
    """(buf, view): a poison-filled output inside a poison halo"""
    return memguard.guarded(shape, dtype, dev, fill="poison", halo="poison", offset_bytes=offset_bytes)


def _in(t, dev, offset_bytes=0):
    return memguard.guarded(t.shape, t.dtype, dev, fill=t, halo="zero", offset_bytes=offset_bytes)[1]


def _word(dev):
    return memguard.guarded((1,), torch.int32, dev, fill=torch.tensor([PREFILL], dtype=torch.int32), halo="poison")


def _written(*pairs):
    """halos intact and no element of the output left unwritten -> the outputs on the CPU"""
    torch.cuda.synchronize()
    res = []
    for p in pairs:
        if p is None:
            res.append(None)
            continue
        buf, view = p
        assert int(memguard.halo_damage(buf, view, "poison")) == 0, "written outside the buffer"
        assert int(memguard.poison_count(view)) == 0, "an element was never written"
        res.append(view.cpu())
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


def _ids(shapes):
    return ["x".join(str(v) for v in s) for s in shapes]


# ---- p2r_bn_stats ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", B.STATS_KINDS)
@pytest.mark.parametrize("L", B.STATS_L)
def test_bn_stats(dev, L, kind):
    x = B.stats_case(L, kind)
    ref = B.stats_ref(x)
    for align in (0, 1):
        part = _out((B.STATS_ROWS, 3), dev)
        _launch(dev, "p2r_bn_stats", B.STATS_ROWS, L, _in(x, dev, 4 * align), part[1])
        got, = _written(part)
        ratios = B.check_stats(got, ref, f"L {L} {kind} align {align}")
        if kind == "const":
            assert not got[:, 2].any() and torch.equal(got[:, 1], x[:, 0])
        print("RATIO stats " + " ".join(f"{k} {v:.4f}" for k, v in ratios.items()))


# ---- p2r_bn_apply, p2r_bn_apply_amax ----------------------------------------------------------------------------------------------
def _apply_call(dev, c, with_res, relu, align=0, mask_off=0, with_mask=True, amax=False, N=None):
    """-> (y, mask or None, word or None) on the CPU; N = 0: the call must write nothing"""
    Nn, C, L = c["x"].shape
    ob = 4 * align
    x = _in(c["x"], dev, ob)
    res = _in(c["res"], dev, ob) if with_res else None
    y = _out((Nn, C, L), dev, offset_bytes=ob)
    mask = _out((Nn, C, L), dev, torch.uint8, offset_bytes=mask_off) if with_mask else None
    mview = mask[1] if mask is not None else None
    scale, shift = c["scale"].to(dev), c["shift"].to(dev)
    word = _word(dev) if amax else None
    n = Nn if N is None else N
    if amax:
        _launch(dev, "p2r_bn_apply_amax", n, C, L, x, scale, shift, res, y[1], mview, word[1])
    else:
        _launch(dev, "p2r_bn_apply", n, C, L, x, scale, shift, res, int(relu), y[1], mview)
    if n == 0:
        _untouched(*[p for p in (y, mask) if p is not None])
        return None, None, (_written(word)[0] if amax else None)
    if relu:
        yc, mc = _written(y, mask)
    else:
        yc, = _written(y)
        mc = None
        if mask is not None:
            _untouched(mask)                  # no ReLU: no mask byte is written
    return yc, mc, (_written(word)[0] if amax else None)


@pytest.mark.parametrize("relu", [True, False], ids=["relu", "norelu"])
@pytest.mark.parametrize("with_res", [False, True], ids=["nores", "res"])
@pytest.mark.parametrize("N,C,L", B.CHUNK_SHAPES, ids=_ids(B.CHUNK_SHAPES))
def test_bn_apply(dev, N, C, L, with_res, relu):
    """(align, mask offset) = (1, 0): x, y, res share a 4-byte offset, so the rows with base % 4 == 3 are 16-byte aligned
    while their mask bytes are not 4-byte aligned; (0, 1): a mask that is 1 byte past a 4-byte boundary"""
    c = B.ew_case(N, C, L)
    ref = B.apply_ref(c["x"], c["scale"], c["shift"], c["res"] if with_res else None)
    first = None
    for align, mask_off, with_mask in [a + (True,) for a in ALIGNMENTS] + [(0, 0, False)]:
        y, mask, _ = _apply_call(dev, c, with_res, relu, align, mask_off, with_mask)
        ratio = B.check_apply(y, mask, ref, relu, f"{(N, C, L)} align {align} mask {mask_off}")
        if first is None:
            first = (y, mask)
        assert memguard.same_bits(y, first[0]) and (mask is None or torch.equal(mask, first[1])), (align, mask_off)
        print(f"RATIO apply y {ratio:.4f}")


@pytest.mark.parametrize("with_res", [False, True], ids=["nores", "res"])
@pytest.mark.parametrize("N,C,L", B.CHUNK_SHAPES, ids=_ids(B.CHUNK_SHAPES))
def test_bn_apply_amax(dev, N, C, L, with_res):
    c = B.ew_case(N, C, L)
    plain = _apply_call(dev, c, with_res, True)
    for align, mask_off in ALIGNMENTS:
        y, mask, word = _apply_call(dev, c, with_res, True, align, mask_off, amax=True)
        assert memguard.same_bits(y, plain[0]) and torch.equal(mask, plain[1])
        B.check_amax(word.item(), y, f"{(N, C, L)} align {align}")
        assert word.item() == int(y.abs().max().view(torch.int32)) != PREFILL
    y, _, word = _apply_call(dev, c, with_res, True, with_mask=False, amax=True)
    assert memguard.same_bits(y, plain[0])
    B.check_amax(word.item(), y)


# ---- p2r_bn_bwd_reduce ------------------------------------------------------------------------------------------------------------
def _gate_args(dev, c, mode, ob, mask_off):
    """(y, mscale, mshift) as the backward entry points take them in mask mode `mode`"""
    y = _in(c["y"], dev, ob) if mode == 1 else _in(c["mask"], dev, mask_off) if mode == 3 else None
    return y, (c["mscale"].to(dev) if mode == 2 else None), (c["mshift"].to(dev) if mode == 2 else None)


@pytest.mark.parametrize("mode", B.MODES)
@pytest.mark.parametrize("N,C,L", B.REDUCE_SHAPES, ids=_ids(B.REDUCE_SHAPES))
def test_bn_bwd_reduce(dev, N, C, L, mode):
    c = B.ew_case(N, C, L)
    ref = B.bwd_reduce_ref(c, mode)
    for align, mask_off in ALIGNMENTS if mode == 3 else ALIGNMENTS[:2]:
        ob = 4 * align
        y, msc, msh = _gate_args(dev, c, mode, ob, mask_off)
        part = _out((N * C, 2), dev)
        _launch(dev, "p2r_bn_bwd_reduce", N, C, L, _in(c["dy"], dev, ob), y, _in(c["x"], dev, ob), c["mean"].to(dev),
                c["invstd"].to(dev), mode, msc, msh, part[1])
        got, = _written(part)
        ratio = B.check_bound(got, ref, f"L {L} mode {mode} align {align} mask {mask_off}")
        print(f"RATIO bwd_reduce sums {ratio:.4f}")


# ---- p2r_bn_bwd_apply, p2r_bn_bwd_apply_amax --------------------------------------------------------------------------------------
def _bwd_apply_call(dev, c, mode, with_dres, align=0, mask_off=0, amax=False, N=None):
    Nn, C, L = c["x"].shape
    ob = 4 * align
    y, msc, msh = _gate_args(dev, c, mode, ob, mask_off)
    dx = _out((Nn, C, L), dev, offset_bytes=ob)
    dres = _out((Nn, C, L), dev, offset_bytes=ob) if with_dres else None
    pc = [c[k].to(dev) for k in ("mean", "invstd", "kscale", "m1", "m2")]
    word = _word(dev) if amax else None
    n = Nn if N is None else N
    dview = dres[1] if dres is not None else None
    if amax:
        assert mode == 3
        _launch(dev, "p2r_bn_bwd_apply_amax", n, C, L, _in(c["dy"], dev, ob), y, _in(c["x"], dev, ob), *pc, dx[1], dview, word[1])
    else:
        _launch(dev, "p2r_bn_bwd_apply", n, C, L, _in(c["dy"], dev, ob), y, _in(c["x"], dev, ob), *pc, mode, msc, msh, dx[1],
                dview)
    if n == 0:
        _untouched(*[p for p in (dx, dres) if p is not None])
        return None, None, (_written(word)[0] if amax else None)
    dxc, drc = _written(dx, dres)
    return dxc, drc, (_written(word)[0] if amax else None)


@pytest.mark.parametrize("with_dres", [True, False], ids=["dres", "nodres"])
@pytest.mark.parametrize("mode", B.MODES)
@pytest.mark.parametrize("N,C,L", B.CHUNK_SHAPES, ids=_ids(B.CHUNK_SHAPES))
def test_bn_bwd_apply(dev, N, C, L, mode, with_dres):
    c = B.ew_case(N, C, L)
    ref = B.bwd_apply_ref(c, mode)
    first = None
    for align, mask_off in ALIGNMENTS if mode == 3 else ALIGNMENTS[:2]:
        dx, dres, _ = _bwd_apply_call(dev, c, mode, with_dres, align, mask_off)
        assert (dres is not None) == with_dres
        ratio = B.check_bwd_apply(dx, dres, ref, f"{(N, C, L)} mode {mode} align {align} mask {mask_off}")
        if first is None:
            first = dx
        assert memguard.same_bits(dx, first), (align, mask_off)
        print(f"RATIO bwd_apply dx {ratio:.4f}")


@pytest.mark.parametrize("with_dres", [True, False], ids=["dres", "nodres"])
@pytest.mark.parametrize("N,C,L", B.CHUNK_SHAPES, ids=_ids(B.CHUNK_SHAPES))
def test_bn_bwd_apply_amax(dev, N, C, L, with_dres):
    c = B.ew_case(N, C, L)
    plain = _bwd_apply_call(dev, c, 3, with_dres)
    for align, mask_off in ALIGNMENTS:
        dx, dres, word = _bwd_apply_call(dev, c, 3, with_dres, align, mask_off, amax=True)
        assert memguard.same_bits(dx, plain[0]) and (not with_dres or memguard.same_bits(dres, plain[1]))
        B.check_amax(word.item(), dx, f"{(N, C, L)} align {align}")
        assert word.item() != PREFILL


def test_amax_of_an_empty_batch_is_zero(dev):
    c = B.ew_case(3, 5, 35)
    assert _apply_call(dev, c, True, True, amax=True, N=0)[2].item() == 0
    assert _bwd_apply_call(dev, c, 3, True, amax=True, N=0)[2].item() == 0


# ---- p2r_bn_finalize, p2r_bn_bwd_finalize -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("width", [3, 2])
@pytest.mark.parametrize("C", B.FIN_C)
@pytest.mark.parametrize("P", B.FIN_P)
def test_bn_finalize(dev, P, C, width):
    worst = {}
    for big in ((False, True) if width == 3 else (False,)):
        case = B.finalize_case(P, C, width, big)
        d = {k: v.to(dev) for k, v in case.items() if k != "M"}
        for i, momentum in enumerate(B.FIN_MOMENTUM):
            with_nbt = (i + P) % 2 == 0
            out = _out((4, C), dev)
            run = [memguard.guarded((C,), F32, dev, fill=case[k], halo="poison") for k in ("running_mean", "running_var")]
            nbt = memguard.guarded((1,), torch.int64, dev, fill=torch.tensor([5]), halo="poison")
            _launch(dev, "p2r_bn_finalize", P, C, width, d["part"], case["M"], d["gamma"], d["beta"], B.EPS, momentum,
                    run[0][1], run[1][1], nbt[1] if with_nbt else None, out[1])
            fin, rm, rv, steps = _written(out, run[0], run[1], nbt)
            label = f"P {P} C {C} width {width} big {big} momentum {momentum}"
            assert steps.item() == (6 if with_nbt else 5), label
            ratios = B.check_finalize({"out": fin, "running_mean": rm, "running_var": rv}, B.finalize_ref(case, momentum), label)
            if momentum <= 0:       # 0: the update keeps the old value exactly; < 0: nothing is written
                assert memguard.same_bits(rm, case["running_mean"]) and memguard.same_bits(rv, case["running_var"]), label
            if momentum == 1.0:
                assert memguard.same_bits(rm, fin[0]), label
            for k, v in ratios.items():
                worst[k] = max(worst.get(k, 0.0), v)
    print("RATIO finalize " + " ".join(f"{k} {v:.4f}" for k, v in worst.items()))


@pytest.mark.parametrize("C", B.FIN_C)
@pytest.mark.parametrize("P", B.FIN_P)
def test_bn_bwd_finalize(dev, P, C):
    part, M = B.bwd_finalize_case(P, C)
    out = _out((4, C), dev)
    _launch(dev, "p2r_bn_bwd_finalize", P, C, part.to(dev), M, out[1])
    got, = _written(out)
    print(f"RATIO bwd_finalize out {B.check_bound(got, B.bwd_finalize_ref(part, M), f'P {P} C {C}'):.4f}")


# ---- p2r_colsum, p2r_sum_leading --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", B.COLSUM_V)
@pytest.mark.parametrize("T", B.COLSUM_T)
def test_colsum(dev, T, V):
    x = B.colsum_case(T, V)
    out = _out((B.COLSUM_ROWS, V), dev)
    _launch(dev, "p2r_colsum", B.COLSUM_ROWS, T, V, x.to(dev), out[1])
    got, = _written(out)
    print(f"RATIO colsum out {B.check_bound(got, B.colsum_ref(x), f'T {T} V {V}'):.4f}")


@pytest.mark.parametrize("tr64", [False, True], ids=["plain", "tr64"])
@pytest.mark.parametrize("P", B.SUM_P)
def test_sum_leading(dev, P, tr64):
    """P < 32: sum_leading_kernel, from 32 on sum_leading_rows_kernel; each call twice, bit-identical"""
    for M in (B.SUM_M_TR64 if tr64 else B.SUM_M):
        inp = B.sum_case(P, M)
        d = inp.to(dev)
        got = []
        for _ in range(2):
            out = _out((M,), dev)
            _launch(dev, "p2r_sum_leading", P, M, d, out[1], int(tr64))
            got.append(_written(out)[0])
        assert memguard.same_bits(got[0], got[1]), f"P {P} M {M}: two calls differ"
        ratio = B.check_bound(got[0], B.sum_leading_ref(inp, tr64), f"P {P} M {M} tr64 {tr64}")
        print(f"RATIO sum_leading{'_tr64' if tr64 else ''} out {ratio:.4f}")


# ---- refused and empty calls ------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing(dev):
    c = {k: v.to(dev) for k, v in B.ew_case(3, 5, 35).items()}
    N, C, L = 3, 5, 35
    pc = [c[k] for k in ("mean", "invstd", "kscale", "m1", "m2")]
    y, mask, dx, dres = _out((N, C, L), dev), _out((N, C, L), dev, torch.uint8), _out((N, C, L), dev), _out((N, C, L), dev)
    part3, part2, word = _out((N * C, 3), dev), _out((N * C, 2), dev), _out((1,), dev, torch.int32)
    _refused(dev, "p2r_bn_stats", (N * C, 0, c["x"], part3[1]), [part3])
    _refused(dev, "p2r_bn_stats", (-1, L, c["x"], part3[1]), [part3])
    for n, ch, l, relu in ((N, C, 0, 1), (N, 0, L, 1), (N, C, -3, 0), (-1, C, L, 1)):
        _refused(dev, "p2r_bn_apply", (n, ch, l, c["x"], c["scale"], c["shift"], c["res"], relu, y[1], mask[1]), [y, mask])
    for n, ch, l, mode in ((N, C, 0, 0), (N, 0, L, 3), (N, C, L, 4), (N, C, L, -1)):
        _refused(dev, "p2r_bn_bwd_reduce", (n, ch, l, c["dy"], c["y"], c["x"], c["mean"], c["invstd"], mode, c["mscale"],
                                            c["mshift"], part2[1]), [part2])
        _refused(dev, "p2r_bn_bwd_apply", (n, ch, l, c["dy"], c["y"], c["x"], *pc, mode, c["mscale"], c["mshift"], dx[1],
                                           dres[1]), [dx, dres])
    for n, ch, l, w in ((N, C, L, None), (N, C, 0, word[1]), (N, 0, L, word[1])):
        _refused(dev, "p2r_bn_apply_amax", (n, ch, l, c["x"], c["scale"], c["shift"], c["res"], y[1], mask[1], w), [y, mask, word])
        _refused(dev, "p2r_bn_bwd_apply_amax", (n, ch, l, c["dy"], c["mask"], c["x"], *pc, dx[1], dres[1], w), [dx, dres, word])
    fc = {k: v.to(dev) for k, v in B.finalize_case(1, 3, 3).items() if k != "M"}
    out = _out((4, 3), dev)
    for P, ch, width, M in ((1, 3, 4, 9.0), (0, 3, 3, 9.0), (1, 0, 3, 9.0), (1, 3, 2, 0.0)):
        _refused(dev, "p2r_bn_finalize", (P, ch, width, fc["part"], M, fc["gamma"], fc["beta"], B.EPS, -1.0, None, None, None,
                                          out[1]), [out])
    _refused(dev, "p2r_bn_bwd_finalize", (0, 3, fc["part"], 9.0, out[1]), [out])
    cs = _out((2, 257), dev)
    _refused(dev, "p2r_colsum", (2, 3, 257, torch.zeros(2, 3, 257, device=dev), cs[1]), [cs])
    _refused(dev, "p2r_colsum", (2, 0, 53, c["x"], cs[1]), [cs])
    inp = torch.zeros(3, 4100, device=dev)
    o = _out((4100,), dev)
    shifted_in, shifted_out = _in(torch.zeros(3, 64), dev, 4), _out((64,), dev, offset_bytes=4)
    assert inp.data_ptr() % 16 == 0 and shifted_in.data_ptr() % 16 == 4 and shifted_out[1].data_ptr() % 16 == 4
    for P, M, src, dst, tr in ((3, 6, inp, o, 0), (3, 64, shifted_in, o, 0), (3, 64, inp, shifted_out, 0), (3, 64, inp, o, 1),
                               (3, 4100, inp, o, 1), (0, 64, inp, o, 0), (40, 6, inp, o, 0)):
        _refused(dev, "p2r_sum_leading", (P, M, src, dst[1], tr), [o, shifted_out])


def test_empty_calls_write_nothing(dev):
    c = B.ew_case(3, 5, 35)
    d = {k: v.to(dev) for k, v in c.items()}
    part3, part2, cs = _out((15, 3), dev), _out((15, 2), dev), _out((3, 53), dev)
    _launch(dev, "p2r_bn_stats", 0, 35, d["x"], part3[1])
    _launch(dev, "p2r_bn_bwd_reduce", 0, 5, 35, d["dy"], d["y"], d["x"], d["mean"], d["invstd"], 1, None, None, part2[1])
    _launch(dev, "p2r_colsum", 0, 5, 53, d["x"], cs[1])
    _untouched(part3, part2, cs)
    assert _apply_call(dev, c, True, True, N=0)[0] is None
    for mode in B.MODES:
        assert _bwd_apply_call(dev, c, mode, True, N=0)[0] is None


# ---- bn_op.fused_bn_act ------------------------------------------------------------------------------------------------------------
class _Catch(torch.autograd.Function):
    """identity in front of the op: its backward sees the very tensor the op's backward returned for x"""
    seen = []

    @staticmethod
    def forward(ctx, x):
        return x.clone()

    @staticmethod
    def backward(ctx, g):
        _Catch.seen.append(g)
        return g


def _module(case, dev, dim, train, momentum=0.1):
    bn = (torch.nn.BatchNorm2d if dim == 4 else torch.nn.BatchNorm1d)(case["gamma"].numel(), momentum=momentum)
    with torch.no_grad():
        bn.weight.copy_(case["gamma"]), bn.bias.copy_(case["beta"])
        bn.running_mean.copy_(case["running_mean"]), bn.running_var.copy_(case["running_var"])
    return bn.to(dev).train(train)


def _run_op(dev, shape, with_res, relu, train, x_of=None, catch=False, **kw):
    """one forward and backward of bn_op.fused_bn_act -> dict of CPU tensors (and the op's own y / dx tensors under 'raw')"""
    from pose2room_amd.p2rnet import bn_op
    case = B.op_case(shape)
    bn = _module(case, dev, len(shape), train)
    leaf = case["x"].to(dev).requires_grad_(True)
    x = leaf if x_of is None else x_of(leaf)
    if catch:
        x = _Catch.apply(x)
    res = case["res"].to(dev).requires_grad_(True) if with_res else None
    assert bn_op.supported(x, bn)
    if "stats" in kw:
        kw["stats"] = kw["stats"](x.detach())
    y = bn_op.fused_bn_act(x, bn, res, relu=relu, **kw)
    _Catch.seen.clear()
    y.backward(case["go"].to(dev))
    torch.cuda.synchronize()
    cpu = lambda t: None if t is None else t.detach().cpu()
    return {"y": cpu(y), "dx": cpu(leaf.grad), "dres": cpu(res.grad) if with_res else None, "dgamma": cpu(bn.weight.grad),
            "dbeta": cpu(bn.bias.grad), "running_mean": cpu(bn.running_mean), "running_var": cpu(bn.running_var),
            "steps": int(bn.num_batches_tracked), "raw": (y, list(_Catch.seen))}


@functools.lru_cache(maxsize=None)
def _own_chain(shape, with_res, relu, train):
    return B.op_ref(B.op_case(shape), with_res, relu, train)


def _check_op(got, shape, with_res, relu, train, label):
    """y and the running statistics against the float64 chain, every gradient against the chain under the device's gates"""
    case = B.op_case(shape)
    own = _own_chain(shape, with_res, relu, train)
    ratios = {"y": B.close_ratio(got["y"], own["y"], *B.Y_TOL)}
    gate = got["y"] > 0
    ref = B.op_ref(case, with_res, relu, train, gate=gate) if relu else own
    if relu:
        print(f"{label}: {int((gate != (own['pre'] > 0)).sum())} of {gate.numel()} gates differ from the chain's own")
    ratios["dx"] = B.close_ratio(got["dx"], ref["dx"], *B.DX_TOL)
    if with_res:
        assert torch.equal(got["dres"], torch.where(gate, case["go"], torch.zeros(())) if relu else case["go"]), "dres"
    else:
        assert got["dres"] is None
    for k in ("dgamma", "dbeta"):
        assert got[k].dtype == F32 and got[k].shape == case["gamma"].shape, k
        ratios[k] = B.rel_ratio(got[k], ref[k], B.PARAM_TOL)
    for k in ("running_mean", "running_var"):
        if train:
            ratios[k] = B.close_ratio(got[k], ref[k], *B.STAT_TOL)
        else:
            assert torch.equal(got[k], case[k]), k
    assert got["steps"] == (1 if train else 0)
    print(f"RATIO op " + " ".join(f"{k} {v:.4f}" for k, v in ratios.items()))
    for k, v in ratios.items():
        assert v <= 1, f"{label} {k}: error / tolerance {v:.3f}"


@pytest.mark.parametrize("train", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("with_res", [False, True], ids=["nores", "res"])
@pytest.mark.parametrize("relu", [True, False], ids=["relu", "norelu"])
@pytest.mark.parametrize("shape", B.OP_SHAPES, ids=_ids(B.OP_SHAPES))
def test_fused_bn_act_against_float64_with_device_gates(dev, shape, relu, with_res, train):
    got = _run_op(dev, shape, with_res, relu, train)
    _check_op(got, shape, with_res, relu, train, f"{shape} relu {relu} res {with_res} train {train}")


def test_fused_bn_act_cumulative_average(dev):
    """momentum=None over two consecutive calls against float64 nn.BatchNorm2d(momentum=None) on the CPU"""
    from pose2room_amd.p2rnet import bn_op
    shape = B.OP_SHAPES[0]
    case = B.op_case(shape)
    bn = _module(case, dev, 4, True, momentum=None)
    want = _module(case, torch.device("cpu"), 4, True, momentum=None).double()
    for x in (case["x"], case["x"] * 1.5 + 0.3):
        y = bn_op.fused_bn_act(x.to(dev), bn, None, relu=True)
        yw = torch.relu(want(x.double()))
        assert B.close_ratio(y.cpu(), yw.detach(), *B.Y_TOL) <= 1
        for k in ("running_mean", "running_var"):
            ratio = B.close_ratio(getattr(bn, k).cpu(), getattr(want, k), *B.STAT_TOL)
            print(f"RATIO cumulative {k} {ratio:.4f}")
            assert ratio <= 1, k
        assert int(bn.num_batches_tracked) == int(want.num_batches_tracked)
    assert int(bn.num_batches_tracked) == 2


@pytest.mark.parametrize("shape", [B.OP_SHAPES[0], B.OP_SHAPES[3]], ids=_ids([B.OP_SHAPES[0], B.OP_SHAPES[3]]))
def test_fused_bn_act_takes_given_partials(dev, shape):
    """stats= as width-3 partials of the op's own statistics pass: the same bits; as width-2 (sum, sum of squares): within
    the tolerances"""
    from pose2room_amd.p2rnet import bn_op
    own = _run_op(dev, shape, True, True, True)
    given = _run_op(dev, shape, True, True, True, stats=lambda x: bn_op._stats_partial(x.contiguous()))
    for k in ("y", "dx", "dres", "dgamma", "dbeta", "running_mean", "running_var"):
        assert memguard.same_bits(own[k], given[k]), k
    sums = _run_op(dev, shape, True, True, True, stats=lambda x: B.width2_partials(x.cpu()).to(x.device))
    _check_op(sums, shape, True, True, True, f"{shape} width 2")


def test_fused_bn_act_on_a_permuted_view(dev):
    shape = B.OP_SHAPES[0]
    plain = _run_op(dev, shape, True, True, True)
    swap = lambda t: t.transpose(2, 3).contiguous().transpose(2, 3)
    view = _run_op(dev, shape, True, True, True, x_of=swap)
    assert not swap(torch.zeros(shape)).is_contiguous()
    for k in ("y", "dx", "dres", "dgamma", "dbeta", "running_mean", "running_var"):
        assert memguard.same_bits(plain[k], view[k]), k


def test_fused_bn_act_announces_exact_range_words(dev):
    """split16: the words left on y and on dx are the exact maxima, and y / dx are the bits of exact mode"""
    from pose2room_amd.p2rnet import math_mode
    shape = B.OP_SHAPES[1]
    exact = _run_op(dev, shape, True, True, True, catch=True)
    try:
        with math_mode.use("split16"):
            before = math_mode.FALLBACK_PASSES
            got = _run_op(dev, shape, True, True, True, catch=True)
            y, (dx,) = got["raw"]
            for name, t in (("y", y), ("dx", dx)):
                word = math_mode.range_word(t, keep=True)
                assert math_mode.FALLBACK_PASSES == before, f"no word was announced for {name}"
                assert word.item() == int(t.detach().abs().max().view(torch.int32)), name
    finally:
        math_mode.reset()
    for k in ("y", "dx", "dres", "dgamma", "dbeta"):
        assert memguard.same_bits(exact[k], got[k]), k
