"""GPU: the memory contract of the op wrappers and their kernels (tests/memguard.py).  Every case runs through
`run_contract` -- inputs inside guard bands of zeros / poison NaN / 3e38, every `torch.empty` of the wrappers replaced by a
poison-filled guarded view: (a) nothing written outside a tensor, (b) nothing returned unwritten, (c) results bit-identical
whatever lies around the tensors -- and keeps its family's comparison against the fp64 or oracle reference at the tolerance
that family's own test file uses.

Not under the harness, for a structural reason (2 paths, no ST-GCN kernel among them):
  * `net_utils.nms.nms_3d_faster*` take numpy boxes and copy them to the device themselves: the inputs cannot be placed
    in guard bands; the batched entry point over device tensors (`nms_3d_batched`, the same kernel) is covered instead.
  * `mdn_sample` draws from the device's Philox stream inside the wrapper, so two runs differ by design ((c) does not
    apply); its own test file checks its guard bands with a fixed seed per call.
"""
import contextlib
import copy

import numpy as np
import pytest
import torch

from tests import cases
from tests.memguard import Input, run_contract

pytestmark = pytest.mark.gpu

V53 = 53


def _close(a, ref, what, tol, where=None):
    scale = ref.abs().max().item() + 1e-12
    err = (a.double() - ref.double().to(a.device)).abs()
    if where is not None:
        err = err * where
    err = err.max().item()
    assert err <= tol * scale, f"{what}: err {err:.3e} vs scale {scale:.3e}"


@contextlib.contextmanager
def _switch(module, **flags):
    old = {k: getattr(module, k) for k in flags}
    for k, v in flags.items():
        setattr(module, k, v)
    try:
        yield
    finally:
        for k, v in old.items():
            setattr(module, k, v)


def test_the_harness_sees_the_wrappers_allocations(dev):
    """the replacements reach the op wrappers on the device: the output of a graph conv IS a recorded, guarded allocation"""
    from pose2room_amd.p2rnet import gcn_op
    from tests.memguard import GUARD, poisoned_allocations
    A = _graph()
    tables = gcn_op.GraphTables(A)
    x, w, b, imp, go = (t.to(dev) for t in cases.graph_conv_inputs(1, 16, A, 0))
    x.requires_grad_(True); w.requires_grad_(True)
    with poisoned_allocations() as pa:
        z, part = gcn_op.graph_conv(x, w, b, torch.tensor(A, dtype=torch.float32, device=dev) * imp, tables, want_stats=True)
        z.backward(go)
        torch.cuda.synchronize()
    mine = {v.data_ptr() for _, v in pa.records}
    assert len(pa.records) >= 4 and z.data_ptr() in mine and part.data_ptr() in mine
    assert z.storage_offset() == GUARD and z.data_ptr() % 512 == 0
    pa.assert_clean(z, part, x.grad, w.grad)


# ---- graph convolution ---------------------------------------------------------------------------------------------
def _graph():
    from pose2room_amd.p2rnet.modules.stgcn_layers import Graph
    return Graph().A


def _gcn_contract(dev, A, N, T, seed, want_stats=False, offset_bytes=0, tol=None):
    """graph_conv forward + all four gradients under the contract -> (results of the plain run, fp64 reference)"""
    from pose2room_amd.p2rnet import gcn_op
    tables = gcn_op.GraphTables(A)
    x, w, b, imp, go = cases.graph_conv_inputs(N, T, A, seed)
    At = torch.tensor(A, dtype=torch.float32)

    def fn(x, w, b, imp, go, At):
        out = gcn_op.graph_conv(x, w, b, At * imp, tables, want_stats=want_stats)
        (out[0] if want_stats else out).backward(go)
        return out

    got = run_contract(fn, dict(x=Input(x, True), w=Input(w, True), b=Input(b, True), imp=Input(imp, True), go=go, At=At),
                       dev, offset_bytes=offset_bytes, tol=tol)
    xr, wr, br, ir = (t.double().to(dev).requires_grad_(True) for t in (x, w, b, imp))
    zr = cases.graph_conv_reference(xr, wr, br, At.double().to(dev) * ir)
    zr.backward(go.double().to(dev))
    return got, dict(z=zr.detach(), x=xr.grad, w=wr.grad, b=br.grad, imp=ir.grad), tables


def _gcn_values(got, ref, At, tz=2e-5, tg=5e-5, key='out'):
    _close(got[key], ref['z'], "z", tz)
    _close(got['grad:x'], ref['x'], "dx", tz)
    _close(got['grad:w'], ref['w'], "dW", tg)
    _close(got['grad:b'], ref['b'], "db", tg)
    _close(got['grad:imp'], ref['imp'], "d importance", tg)
    assert (got['grad:imp'].cpu()[At == 0] == 0).all()


@pytest.mark.parametrize("want_stats", [False, True])
@pytest.mark.parametrize("N,T", [(1, 1), (2, 7), (1, 20), (3, 33), (2, 130), (5, 1000), (1, 16), (3, 48), (5, 1008)])
def test_graph_conv(dev, N, T, want_stats):
    """ragged tails (second generation, first-generation gradient kernels), T % 4 == 0 only (gcn3_weight_grad at 20), whole
    tiles (third generation), more tiles than workgroups; the adjacency gradient of a ragged length runs on the
    first-generation kernel, whose partial rows take float atomics: (c) to that test's 5e-5 there, exact otherwise"""
    from pose2room_amd.p2rnet import bn_op
    A = _graph()
    got, ref, _ = _gcn_contract(dev, A, N, T, N * 100 + T, want_stats, tol=None if T % 16 == 0 else {'grad:imp': 5e-5})
    _gcn_values(got, ref, torch.tensor(A), key='out.0' if want_stats else 'out')
    if want_stats:
        mean, var, _ = bn_op.moments(got['out.1'], N * T * V53)
        zd = got['out.0'].double()
        torch.testing.assert_close(mean, zd.mean(dim=(0, 2, 3)), rtol=1e-5, atol=1e-6)
        torch.testing.assert_close(var, zd.var(dim=(0, 2, 3), unbiased=False), rtol=1e-4, atol=1e-6)


@pytest.mark.parametrize("offset_bytes", [16, 4])
@pytest.mark.parametrize("N,T", [(3, 33), (3, 48)])
def test_graph_conv_offset_inputs(dev, N, T, offset_bytes):
    """data_ptr() % 32 == 16: the least alignment the fast paths accept -- whole tiles there run the third generation,
    forward (count, mean, M2) statistics and all, and (c) is exact; % 16 == 4: every kernel must fall back (pairs of sums
    from gcn2, the first-generation adjacency gradient with its float atomics: 5e-5 on that gradient only)"""
    from pose2room_amd.p2rnet import gcn_op, math_mode
    A = _graph()
    fast = T % 16 == 0 and offset_bytes % 16 == 0
    seen = []
    real = gcn_op._gen3_able

    def spy(x, z, addend, tables, bwd=None):
        ok = real(x, z, addend, tables, bwd)
        seen.append((x.data_ptr() % 32, ok))
        return ok

    with _switch(gcn_op, _gen3_able=spy), math_mode.use('exact'):     # the exact kernels' dispatcher, whatever the session's mode
        got, ref, _ = _gcn_contract(dev, A, N, T, 7 * N + T, True, offset_bytes=offset_bytes,
                                    tol=None if fast else {'grad:imp': 5e-5})
    # forward and data gradient of each of the four runs asked, on operands at the offset, and were answered as expected
    assert len(seen) == 8 and all(ptr == offset_bytes and ok == fast for ptr, ok in seen), seen
    assert got['out.1'].shape[-1] == (3 if fast else 2)
    _gcn_values(got, ref, torch.tensor(A), key='out.0')


@pytest.mark.parametrize("N,T", [(1, 16), (3, 48), (2, 7)])
def test_graph_conv_second_generation(dev, N, T):
    """USE_GEN3 off: gcn2 and the first-generation gradient kernels at whole tiles too"""
    from pose2room_amd.p2rnet import gcn_op
    A = _graph()
    with _switch(gcn_op, USE_GEN3=False):
        got, ref, _ = _gcn_contract(dev, A, N, T, 3 * N + T, True, tol={'grad:imp': 5e-5})
    _gcn_values(got, ref, torch.tensor(A), key='out.0')


@pytest.mark.parametrize("N,T", [(2, 32), (2, 21)])
def test_graph_conv_extra_link(dev, N, T):
    """the 53-joint adjacency with one more link: no static schedule, gcn2's run-time work stream"""
    A = _graph().copy()
    A[3, 5, 7] = 0.5
    got, ref, tables = _gcn_contract(dev, A, N, T, 4 + T, False, tol={'grad:imp': 5e-5})
    assert tables.gen2 and not tables.gen3
    _gcn_values(got, ref, torch.tensor(A))


@pytest.mark.parametrize("V", [17, 25, 56])
def test_graph_conv_other_skeletons(dev, V):
    """first generation, forward and all four gradients (5e-5 like its own test; (c) to the same: float atomics)"""
    A = cases.ring_adjacency(11, V, V)
    got, ref, tables = _gcn_contract(dev, A, 2, 37, V, True, tol={'grad:imp': 5e-5})
    assert not tables.gen2
    _gcn_values(got, ref, torch.tensor(A), tz=5e-5, key='out.0')


@pytest.mark.parametrize("N,T", [(2, 40), (3, 48), (1, 7)])
def test_chained_blocks_masked_addend_and_bn_link(dev, N, T):
    """two chained st_gcn_blocks: the second block's data-gradient kernel adds the masked identity gradient and emits the
    BatchNorm-backward sums of the first (bn_op.BNLink); values against the same blocks run unchained, 2e-4 as in
    test_gcn_gpu"""
    from pose2room_amd.p2rnet import gcn_op
    from pose2room_amd.p2rnet.modules.stgcn_layers import st_gcn_block
    A = _graph()
    tables = gcn_op.GraphTables(A)
    torch.manual_seed(7 + T)
    blocks = torch.nn.ModuleList([st_gcn_block(64, 64, (3, A.shape[0]), 1) for _ in range(2)])
    for b in blocks:
        for bn in (b.tcn[0], b.tcn[3]):
            bn.weight.data.uniform_(0.5, 1.5); bn.bias.data.uniform_(-0.3, 0.3)
    g = torch.Generator().manual_seed(T)
    x0, w = torch.randn(N, 64, T, V53, generator=g), torch.randn(N, 64, T, V53, generator=g)
    At = torch.tensor(A, dtype=torch.float32)

    def make(chain):
        def fn(x0, w, At, net):
            h = x0 + 0.0
            for i, b in enumerate(net):
                b.gcn.tables = tables
                b.chain_input = chain and i > 0
                h, _ = b(h, At)
            (h * w).sum().backward()
            return h
        return fn

    ins = dict(x0=Input(x0, True), w=w, At=At, net=blocks)
    got = run_contract(make(True), ins, dev)
    ref = run_contract(make(False), ins, dev, fills=())
    for k, v in ref.items():
        if k.endswith('gcn.conv.bias') or k.endswith('tcn.2.bias') or k.startswith('buf:'):
            continue        # zero in exact arithmetic: rounding noise of the summation order on either path
        scale = max(v.abs().max().item(), 1.0)
        assert (got[k] - v).abs().max().item() <= 2e-4 * scale, k


# ---- temporal convolution -------------------------------------------------------------------------------------------
def _tconv_contract(dev, N, T, V, train, taps=3, offset_bytes=0, addend=False, tol=None):
    from pose2room_amd.p2rnet import tconv_op
    bn, conv = cases.bn_conv_pair(taps, N * 10 + T, dims=2 if taps == 3 else 1)
    bn.train(train)
    g = torch.Generator().manual_seed(N * 10 + T + 1)
    z = torch.randn(N, 64, T, V, generator=g) * 1.5 + 0.3
    go = torch.randn(N, 64, T, V, generator=g)
    pe = torch.randn(N, 64, T, generator=g) if addend else None

    def fn(z, go, bn, conv, pe=None):
        u = tconv_op.bn_relu_tconv(z, bn, conv, add_ct=pe)
        u.backward(go)
        return u

    ins = dict(z=Input(z, True), go=go, bn=bn, conv=conv)
    if addend:
        ins['pe'] = Input(pe, True)
    got = run_contract(fn, ins, dev, offset_bytes=offset_bytes, tol=tol)

    # fp64 reference, compared as in test_tconv_gpu (undecided ReLU gates left out of dz, their terms allowed in the sums)
    bn_ref, conv_ref = copy.deepcopy(bn).double().to(dev), copy.deepcopy(conv).double().to(dev)
    zr = z.double().to(dev).requires_grad_(True)
    per = pe.double().to(dev).requires_grad_(True) if addend else None
    if taps == 3:
        pre = bn_ref(zr)
        act = torch.relu(pre)
        act.retain_grad()
        ur = conv_ref(act)
    else:
        pre = bn_ref(zr.view(N, 64, T * V))
        act = torch.relu(pre)
        act.retain_grad()
        ur = conv_ref(act).view(N, 64, T, V)
        pre, = (pre.view(N, 64, T, V),)
        if addend:
            ur = ur + per.unsqueeze(-1)
    ur.backward(go.double().to(dev))
    _close(got['out'], ur.detach(), "u", 3e-5)
    decided = (pre.detach().abs() > 1e-5).double()
    assert decided.mean().item() > 0.999
    _close(got['grad:z'], zr.grad, "dz", 1e-4, where=decided)
    _close(got['grad:conv.weight'], conv_ref.weight.grad.view_as(got['grad:conv.weight']), "dW", 1e-4)
    _close(got['grad:conv.bias'], conv_ref.bias.grad, "dbias", 1e-4)
    if addend:
        _close(got['grad:pe'], per.grad, "dpe", 1e-5)
    und = 1.0 - decided
    shp = (1, -1, 1, 1)
    xhat = (pre.detach() - bn_ref.bias.view(shp)) / bn_ref.weight.view(shp)
    ag = act.grad.view(N, 64, T, V)
    for k, want, term in (('grad:bn.bias', bn_ref.bias.grad, ag.abs()), ('grad:bn.weight', bn_ref.weight.grad, (ag * xhat).abs())):
        slack = (und * term).sum(dim=(0, 2, 3))
        err = (got[k].double() - want).abs()
        assert bool((err <= 1e-4 * want.abs().max() + slack).all()), f"{k}: {err.max().item():.3e}"
    if train:
        _close(got['buf:bn.running_var'], bn_ref.running_var, "running_var", 1e-5)
    return got


@pytest.mark.parametrize("train", [True, False])
@pytest.mark.parametrize("T", [1, 9, 130, 1000, 16, 64])
def test_bn_relu_tconv(dev, T, train):
    """53 joints, 3 taps: ragged tiles (second generation), whole tiles (third), more tiles than workgroups"""
    _tconv_contract(dev, 5 if T == 1000 else 2, T, V53, train)


@pytest.mark.parametrize("fuse_dz,gen3", [(False, True), (True, False), (False, False)])
@pytest.mark.parametrize("T", [9, 64])
def test_bn_relu_tconv_variants(dev, T, fuse_dz, gen3):
    from pose2room_amd.p2rnet import tconv_op
    with _switch(tconv_op, FUSE_DZ=fuse_dz, USE_GEN3=gen3):
        _tconv_contract(dev, 2, T, V53, True)


@pytest.mark.parametrize("offset_bytes", [16, 4])
@pytest.mark.parametrize("T", [9, 64])
def test_bn_relu_tconv_offset_inputs(dev, T, offset_bytes):
    _tconv_contract(dev, 2, T, V53, True, offset_bytes=offset_bytes)


@pytest.mark.parametrize("train", [True, False])
@pytest.mark.parametrize("T,V", [(17, 25), (9, 20)])
def test_bn_relu_tconv_other_skeletons(dev, T, V, train):
    """first generation (csrc/stgcn_tconv.hip sums its per-wave slots in a fixed order: no float atomic, (c) exact)"""
    _tconv_contract(dev, 2, T, V, train)


@pytest.mark.parametrize("train", [True, False])
@pytest.mark.parametrize("T,V,addend", [(40, 53, False), (48, 53, False), (9, 20, False), (48, 53, True), (40, 53, True),
                                        (17, 20, True)])
def test_bn_relu_pointwise(dev, T, V, addend, train):
    """one tap (the embedding MLPs' layers), with and without the broadcast addend"""
    _tconv_contract(dev, 2, T, V, train, taps=1, addend=addend)


# ---- split16 mode ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,T", [(1, 16), (3, 48), (2, 256), (1, 7), (2, 40)])
def test_split16_graph_conv_and_tconv(dev, N, T):
    """graph conv + temporal conv in split16 mode: the split kernels at whole tiles, the exact ones at (1,7) and (2,40).
    Values as in test_split16_gpu: at most 1.5x the exact mode's distance from fp64 plus 2e-7 of range."""
    from pose2room_amd.p2rnet import gcn_op, math_mode, tconv_op
    A = _graph()
    tables = gcn_op.GraphTables(A)
    x, w, b, imp, go = cases.graph_conv_inputs(N, T, A, N * 100 + T)
    At = torch.tensor(A, dtype=torch.float32)
    bn, conv = cases.bn_conv_pair(3, T)
    bn.train(True)

    def fn(x, w, b, imp, go, At, bn, conv):
        z = gcn_op.graph_conv(x, w, b, At * imp, tables)
        u = tconv_op.bn_relu_tconv(z, bn, conv)
        u.backward(go)
        return z, u

    ins = dict(x=Input(x, True), w=Input(w, True), b=Input(b, True), imp=Input(imp, True), go=go, At=At, bn=bn, conv=conv)
    with math_mode.use('split16'):
        got = run_contract(fn, ins, dev, tol=None if T % 16 == 0 else {'grad:imp': 5e-5})
    with math_mode.use('exact'):
        exact = run_contract(fn, ins, dev, fills=())
    math_mode.reset()
    xr, wr, br, ir = (t.double().to(dev).requires_grad_(True) for t in (x, w, b, imp))
    bn64, conv64 = copy.deepcopy(bn).double().to(dev), copy.deepcopy(conv).double().to(dev)
    zr = cases.graph_conv_reference(xr, wr, br, At.double().to(dev) * ir)
    ur = conv64(torch.relu(bn64(zr)))
    ur.backward(go.double().to(dev))
    want = {'out.0': zr.detach(), 'out.1': ur.detach(), 'grad:x': xr.grad, 'grad:w': wr.grad, 'grad:imp': ir.grad,
            'grad:conv.weight': conv64.weight.grad}

    def rel(a, ref):
        return (a.double() - ref).abs().max().item() / (ref.abs().max().item() + 1e-300)
    for k, ref in want.items():
        es, ee = rel(got[k], ref), rel(exact[k], ref)
        assert es <= 1.5 * ee + 2e-7, (k, es, ee)
    if T % 16 == 0:
        assert not torch.equal(got['out.0'], exact['out.0'])        # the split kernels did run
    else:
        assert torch.equal(got['out.0'], exact['out.0'])            # ... and here the exact ones


# ---- BatchNorm + activation, embedding ------------------------------------------------------------------------------
@pytest.mark.parametrize("train", [True, False])
@pytest.mark.parametrize("with_res", [False, True])
@pytest.mark.parametrize("shape", [(3, 8, 7, 5), (2, 64, 40, 53)])
def test_fused_bn_act(dev, shape, with_res, train):
    from pose2room_amd.p2rnet import bn_op
    g = torch.Generator().manual_seed(0)
    bn = torch.nn.BatchNorm2d(shape[1])
    with torch.no_grad():
        for t, lo, hi in ((bn.weight, 0.5, 1.5), (bn.bias, -0.5, 0.5), (bn.running_mean, -0.2, 0.2), (bn.running_var, 0.5, 2.0)):
            t.copy_(torch.rand(t.shape, generator=g) * (hi - lo) + lo)
    bn.train(train)
    x = torch.randn(shape, generator=g) * 2 + 0.5
    res = torch.randn(shape, generator=g) if with_res else None
    go = torch.randn(shape, generator=g)

    def fn(x, go, bn, res=None):
        y = bn_op.fused_bn_act(x, bn, res, relu=True)
        y.backward(go)
        return y

    ins = dict(x=Input(x, True), go=go, bn=bn)
    if with_res:
        ins['res'] = Input(res, True)
    got = run_contract(fn, ins, dev)
    bn_ref = copy.deepcopy(bn).to(dev)
    xr = x.to(dev).requires_grad_(True)
    rr = res.to(dev).requires_grad_(True) if with_res else None
    yr = bn_ref(xr)
    yr = torch.relu(yr + rr if with_res else yr)
    yr.backward(go.to(dev))
    torch.testing.assert_close(got['out'], yr, rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(got['grad:x'], xr.grad, rtol=1e-4, atol=1e-5)
    if with_res:
        torch.testing.assert_close(got['grad:res'], rr.grad, rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(got['grad:bn.weight'], bn_ref.weight.grad, rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(got['grad:bn.bias'], bn_ref.bias.grad, rtol=1e-4, atol=1e-4)
    if train:
        torch.testing.assert_close(got['buf:bn.running_mean'], bn_ref.running_mean, rtol=1e-5, atol=1e-6)
        torch.testing.assert_close(got['buf:bn.running_var'], bn_ref.running_var, rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("want_stats", [False, True])
@pytest.mark.parametrize("B,L", [(1, 7), (3, 20 * 33 + 1), (2, 4096)])
def test_embed3(dev, B, L, want_stats):
    from pose2room_amd.p2rnet import bn_op, tconv_op
    torch.manual_seed(B + L)
    conv = torch.nn.Conv1d(3, 64, 1)
    g = torch.Generator().manual_seed(L)
    x, go = torch.randn(B, 3, L, generator=g), torch.randn(B, 64, L, generator=g)

    def fn(x, go, conv):
        out = tconv_op.embed3(x, conv, want_stats)
        (out[0] if want_stats else out).backward(go)
        return out

    got = run_contract(fn, dict(x=x, go=go, conv=conv), dev)
    ref = copy.deepcopy(conv).double().to(dev)
    want = ref(x.double().to(dev))
    want.backward(go.double().to(dev))
    out = got['out.0' if want_stats else 'out']
    torch.testing.assert_close(out.double(), want, rtol=1e-6, atol=1e-6)
    for k, r in (('grad:conv.weight', ref.weight.grad), ('grad:conv.bias', ref.bias.grad)):
        torch.testing.assert_close(got[k].double(), r, rtol=1e-4, atol=1e-4 * r.abs().max().item())
    if want_stats:
        mean, var, _ = bn_op.moments(got['out.1'], B * L)
        torch.testing.assert_close(mean, out.double().mean(dim=(0, 2)), rtol=1e-5, atol=1e-6)
        torch.testing.assert_close(var, out.double().var(dim=(0, 2), unbiased=False), rtol=1e-4, atol=1e-6)


@pytest.mark.parametrize("train", [True, False])
@pytest.mark.parametrize("B,rows,inner,add", [(2, 64, 53, True), (3, 16, 20, False), (1, 128, 53, False)])
def test_embed_mlp_one_pass_backward(dev, B, rows, inner, add, train):
    """embed_op.embed_mlp against the layer-by-layer functions (tolerances of test_tconv_gpu's test of the same name)"""
    from pose2room_amd.p2rnet import embed_op
    from pose2room_amd.p2rnet.modules.stgcn import _point_mlp, STGCN
    L = rows * inner
    torch.manual_seed(B * 100 + rows + inner)
    seq = _point_mlp(3, 64, 64)
    with torch.no_grad():
        for m in seq.modules():
            if isinstance(m, torch.nn.BatchNorm1d):
                m.weight.uniform_(0.5, 1.5); m.bias.uniform_(-0.5, 0.5)
                m.running_mean.uniform_(-0.2, 0.2); m.running_var.uniform_(0.5, 2.0)
    seq.train(train)
    x = torch.randn(B, 3, L) * torch.tensor([1.0, 0.4, 2.0])[None, :, None]
    pe = torch.randn(B, 64, rows) if add else None
    go = torch.randn(B, 64, L)

    def fused(x, go, seq, pe=None):
        assert embed_op.supported(seq, x, inner, pe)
        out = embed_op.embed_mlp(seq, x, inner, pe)
        out.backward(go)
        return out

    def layered(x, go, seq, pe=None):
        with _switch(embed_op, USE_FUSED=False):
            out = STGCN._mlp(seq, x, inner, add_ct=pe)
            out.backward(go)
        return out

    ins = dict(x=x, go=go, seq=seq)
    if add:
        ins['pe'] = Input(pe, True)
    got = run_contract(fused, ins, dev)
    lay = run_contract(layered, ins, dev, fills=())
    ref64 = copy.deepcopy(seq).double().to(dev)
    with torch.no_grad():
        o64 = ref64(x.double().to(dev))
        if add:
            o64 = (o64.view(B, 64, rows, inner) + pe.double().to(dev).unsqueeze(-1)).view(B, 64, L)
    _close(got['out'], o64, "out vs fp64", 5e-5)
    for k, v in lay.items():
        if k == 'out':
            if inner == 53:
                assert torch.equal(got[k], v)
            else:
                _close(got[k], v, k, 2e-6)
        elif k == 'grad:pe':
            _close(got[k], v, k, 1e-6)
        elif k.startswith('grad:'):
            _close(got[k], v, k, 1e-4)
        else:
            _close(got[k].float(), v.float(), k, 0.0 if inner == 53 else 2e-6)


# ---- pointnet2 ops --------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ext(dev):
    from pose2room_amd.pointnet2_ops import _ext
    return _ext


@pytest.mark.parametrize("b,n,m,kind,seed", [c for c in cases.FPS_CASES if c[4] in (3, 4, 5, 6, 18, 19, 22)])
def test_fps(ext, oracle, dev, b, n, m, kind, seed):
    """n = 1, n = 33, one workgroup per cloud and several (17000 points)"""
    xyz = cases.cloud(b, n, seed, kind)
    got = run_contract(lambda xyz: ext.furthest_point_sampling(xyz, m), dict(xyz=xyz), dev)
    assert torch.equal(got['out'].cpu(), oracle.OracleExt.furthest_point_sampling(xyz, m))


@pytest.mark.parametrize("b,n,m,radius,nsample,kind,seed", [c for c in cases.BALL_CASES if c[6] in (3, 4, 5, 8, 10)])
def test_ball_query(ext, oracle, dev, b, n, m, radius, nsample, kind, seed):
    xyz = cases.cloud(b, n, seed, kind)
    new_xyz = cases.centres_from(xyz, m, seed)
    got = run_contract(lambda new_xyz, xyz: ext.ball_query(new_xyz, xyz, radius, nsample), dict(new_xyz=new_xyz, xyz=xyz), dev)
    assert torch.equal(got['out'].cpu(), oracle.OracleExt.ball_query(new_xyz, xyz, radius, nsample))


@pytest.mark.parametrize("b,c,n,p,s,seed", [(2, 3, 512, 128, 16, 2), (1, 5, 33, 7, 3, 3), (2, 1, 1, 1, 1, 6)])
def test_group_points_and_grad(ext, oracle, dev, b, c, n, p, s, seed):
    g = torch.Generator().manual_seed(seed)
    pts = torch.randn(b, c, n, generator=g)
    idx = torch.randint(0, n, (b, p, s), generator=g, dtype=torch.int32)
    go = torch.randn(b, c, p, s, generator=g)
    got = run_contract(lambda pts, idx, go: (ext.group_points(pts, idx), ext.group_points_grad(go, idx, n)),
                       dict(pts=pts, idx=idx, go=go), dev)
    assert torch.equal(got['out.0'].cpu(), oracle.OracleExt.group_points(pts, idx))
    assert torch.equal(got['out.1'].cpu(), oracle.OracleExt.group_points_grad(go, idx, n))


def test_group_points_grad_scatter_form(ext, oracle, dev):
    """an index list too long for LDS: the order-free scatter form (float atomics: 1e-5 / 1e-4 as in test_ops_gpu)"""
    g = torch.Generator().manual_seed(8)
    b, c, n, p, s = 1, 6, 700, 2500, 16
    idx = torch.randint(0, n, (b, p, s), generator=g, dtype=torch.int32)
    go = torch.randn(b, c, p, s, generator=g)
    got = run_contract(lambda go, idx: ext.group_points_grad(go, idx, n), dict(go=go, idx=idx), dev, tol=1e-5)
    torch.testing.assert_close(got['out'].cpu(), oracle.OracleExt.group_points_grad(go, idx, n), rtol=1e-5, atol=1e-4)


@pytest.mark.parametrize("b,c,n,m,seed", [(1, 7, 100, 100, 2), (2, 256, 64, 9, 3), (1, 3, 33, 1, 4)])
def test_gather_points_and_grad(ext, oracle, dev, b, c, n, m, seed):
    g = torch.Generator().manual_seed(seed)
    pts = torch.randn(b, c, n, generator=g)
    idx = torch.randint(0, n, (b, m), generator=g, dtype=torch.int32)
    go = torch.randn(b, c, m, generator=g)
    got = run_contract(lambda pts, idx, go: (ext.gather_points(pts, idx), ext.gather_points_grad(go, idx, n)),
                       dict(pts=pts, idx=idx, go=go), dev)
    assert torch.equal(got['out.0'].cpu(), oracle.OracleExt.gather_points(pts, idx))
    assert torch.equal(got['out.1'].cpu(), oracle.OracleExt.gather_points_grad(go, idx, n))


@pytest.mark.parametrize("b,n,m,kind,seed", [(2, 100, 2, "uniform", 2), (1, 10, 1, "uniform", 3), (2, 300, 64, "lattice", 4),
                                             (1, 33, 33, "uniform", 7)])
def test_three_nn(ext, oracle, dev, b, n, m, kind, seed):
    unknown, known = cases.cloud(b, n, seed, kind), cases.cloud(b, m, seed + 50, kind)
    got = run_contract(lambda unknown, known: ext.three_nn(unknown, known), dict(unknown=unknown, known=known), dev)
    wd, wi = oracle.OracleExt.three_nn(unknown, known)
    assert torch.equal(got['out.1'].cpu(), wi) and torch.equal(got['out.0'].cpu(), wd)


@pytest.mark.parametrize("b,c,m,n,seed", [(2, 64, 128, 512, 1), (1, 3, 5, 9, 2), (1, 5, 1, 33, 4)])
def test_three_interpolate_and_grad(ext, oracle, dev, b, c, m, n, seed):
    g = torch.Generator().manual_seed(seed)
    pts = torch.randn(b, c, m, generator=g)
    idx = torch.randint(0, m, (b, n, 3), generator=g, dtype=torch.int32)
    w = torch.rand(b, n, 3, generator=g)
    w = (w / w.sum(-1, keepdim=True)).contiguous()
    go = torch.randn(b, c, n, generator=g)
    got = run_contract(lambda pts, idx, w, go: (ext.three_interpolate(pts, idx, w), ext.three_interpolate_grad(go, idx, w, m)),
                       dict(pts=pts, idx=idx, w=w, go=go), dev, tol=1e-5)
    assert torch.equal(got['out.0'].cpu(), oracle.OracleExt.three_interpolate(pts, idx, w))
    torch.testing.assert_close(got['out.1'].cpu(), oracle.OracleExt.three_interpolate_grad(go, idx, w, m), rtol=1e-5, atol=1e-5)


def _sa_module(M):
    from pose2room_amd.pointnet2_ops.pointnet2_modules import PointnetSAModuleVotes
    return PointnetSAModuleVotes(npoint=M, radius=0.3, nsample=16, mlp=[256, 256, 256], use_xyz=False, normalize_xyz=True,
                                 bn=False)


@pytest.mark.parametrize("B,N,M,kind", [(1, 300, 37, "uniform"), (3, 64, 6, "lattice"), (1, 33, 1, "uniform")])
def test_sa_votes_forward(ext, oracle, dev, B, N, M, kind):
    from pose2room_amd.pointnet2_ops import fused
    torch.manual_seed(B * 7 + M)
    mod = _sa_module(M)
    xyz, feats, new_xyz = cases.cloud(B, N, 11, kind), torch.randn(B, 256, N), None
    new_xyz = cases.centres_from(xyz, M, 11)

    def fn(xyz, new_xyz, feats, mod):
        with torch.no_grad():
            return fused.sa_votes(xyz, new_xyz, feats, 0.3, 16, mod.mlp_module, return_idx=True)

    got = run_contract(fn, dict(xyz=xyz, new_xyz=new_xyz, feats=feats, mod=mod), dev)
    assert torch.equal(got['out.1'].cpu(), oracle.OracleExt.ball_query(new_xyz, xyz, 0.3, 16))
    md = copy.deepcopy(mod).to(dev)
    with torch.no_grad():
        want = md.mlp_module(ext.group_points(feats.to(dev), got['out.1'])).max(dim=3).values
    torch.testing.assert_close(got['out.0'], want, rtol=1e-4, atol=1e-4)


@pytest.mark.parametrize("B,N,M,kind", [(1, 300, 37, "uniform"), (3, 64, 6, "lattice")])
def test_sa_votes_backward(dev, B, N, M, kind):
    """fused training path against the unfused HIP chain: indices exact, outputs 1e-4, gradients 1e-3 (test_ops_gpu)"""
    torch.manual_seed(B * 5 + M)
    mod = _sa_module(M)
    xyz, feats, go = cases.cloud(B, N, 21, kind), torch.randn(B, 256, N), torch.randn(B, 256, M)

    def make(fused):
        def fn(xyz, feats, go, mod):
            mod.fused = fused
            nx, nf, inds = mod(xyz, feats)
            nf.backward(go)
            return nx, nf, inds
        return fn

    ins = dict(xyz=xyz, feats=Input(feats, True), go=go, mod=mod)
    got = run_contract(make(True), ins, dev)
    ref = run_contract(make(False), ins, dev, fills=(), tol=1e-5)
    assert torch.equal(got['out.0'], ref['out.0']) and torch.equal(got['out.2'], ref['out.2'])
    torch.testing.assert_close(got['out.1'], ref['out.1'], rtol=1e-4, atol=1e-4)
    for k, v in ref.items():
        if k.startswith('grad:'):
            scale = max(v.abs().max().item(), 1e-6)
            assert (got[k] - v).abs().max().item() <= 1e-3 * scale, k


@pytest.mark.parametrize("kw", [{}, {"l1smooth": True}, {"l1": True}])
@pytest.mark.parametrize("B,N,M,C", [(1, 5, 6, 3), (3, 17, 200, 3), (2, 9, 4, 5), (1, 128, 1, 3)])
def test_nn_distance(oracle, dev, B, N, M, C, kw):
    from pose2room_amd.net_utils.nn_distance import nn_distance
    g = torch.Generator().manual_seed(B * 1000 + N * 10 + M)
    a, q = torch.randn(B, N, C, generator=g), torch.randn(B, M, C, generator=g)
    g1, g2 = torch.randn(B, N, generator=g), torch.randn(B, M, generator=g)

    def fn(a, q, g1, g2):
        out = nn_distance(a, q, **kw)
        (out[0] * g1).sum().add((out[2] * g2).sum()).backward()
        return out

    got = run_contract(fn, dict(a=Input(a, True), q=Input(q, True), g1=g1, g2=g2), dev)
    want = oracle.nn_distance(a, q, **kw)
    for i, w in enumerate(want):
        assert torch.equal(got[f'out.{i}'].cpu(), w)
    wa, wq = oracle.nn_distance_grad(a, q, want[1], want[3], g1, g2, **kw)
    assert torch.equal(got['grad:a'].cpu(), wa) and torch.equal(got['grad:q'].cpu(), wq)


@pytest.mark.parametrize("B,K", [(5, 128), (2, 33), (1, 1)])
def test_nms3d_batched(oracle, dev, B, K):
    from pose2room_amd.net_utils import nms
    allb = np.stack([cases.random_boxes(K, seed=100 + i, stride=7) for i in range(B)])
    valid = np.random.default_rng(0).uniform(size=(B, K)) < 0.7
    if B > 3:
        valid[3] = False
    vt = torch.from_numpy(valid)
    got = run_contract(lambda boxes: nms.nms_3d_batched(boxes, 0.1, valid=vt, return_pick=True),
                       dict(boxes=torch.from_numpy(allb)), dev)
    keep, pick, npick = (got[f'out.{i}'].cpu().numpy() for i in range(3))
    for i in range(B):
        sel = np.where(valid[i])[0]
        want = [int(sel[j]) for j in oracle.nms_3d(allb[i][sel], 0.1)] if len(sel) else []
        assert list(pick[i, :npick[i]]) == want
        mask = np.zeros(K, np.uint8); mask[want] = 1
        assert np.array_equal(keep[i], mask)


# ---- detection loss, batch assembly ---------------------------------------------------------------------------------
@pytest.mark.parametrize("B,S,K,T,case", [(2, 512, 128, 64, 'near'), (2, 64, 128, 32, 'none'), (2, 300, 128, 40, 'ties'),
                                          (2, 300, 257, 40, 'k257'), (3, 255, 361, 8, 'lds')])
def test_fused_detection_loss(dev, B, S, K, T, case):
    """csrc/det_loss.hip against the composed loss: entries 2e-5 / 1e-6, gradients 2e-5 of scale (test_loss_gpu); 'k257'
    and 'lds' are the entries of det_loss_cases.SWEEP with a second trip of the proposal loop, 32 ground-truth slots and
    the dynamic LDS at its limit -- the largest index every output is written at"""
    from pose2room_amd.p2rnet import P2RConfig, default_config
    from pose2room_amd.p2rnet.loss import BoxNetDetectionLoss
    from tests import det_loss_cases
    cfg = P2RConfig(default_config('train', data={'num_frames': T}), device=dev)
    loss_fn = BoxNetDetectionLoss(1, dev, cfg)
    if case in ('k257', 'lds'):
        assert det_loss_cases.BY_ID[case].dims[:4] == (B, S, K, T)
        est, gt = det_loss_cases.sweep_scene(case)
    else:
        est, gt = cases.det_loss_scene(B, S, K, T, seed=B * 1000 + K + T, case=case)
    diff = ['vote_xyz', 'center', 'size', 'heading', 'objectness_scores', 'sem_cls_scores']
    ins = {'e_' + k: Input(v, k in diff) for k, v in est.items()}
    ins.update({'g_' + k: v for k, v in gt.items()})

    def make(fused):
        def fn(**kw):
            e = {k[2:]: v for k, v in kw.items() if k.startswith('e_')}
            g = {k[2:]: v for k, v in kw.items() if k.startswith('g_')}
            out = loss_fn(e, g, None) if fused else loss_fn.composed(e, g, None)
            out['total'].backward()
            return dict(out)
        return fn

    got = run_contract(make(True), ins, dev)
    want = run_contract(make(False), ins, dev, fills=())
    assert list(got) == list(want)
    for k, v in want.items():
        assert got[k].dtype == v.dtype and got[k].shape == v.shape, k
        if k.startswith('out.'):
            np.testing.assert_allclose(got[k].item(), v.item(), rtol=2e-5, atol=1e-6, err_msg=k)
        else:
            scale = max(v.abs().max().item(), 1e-12)
            assert (got[k] - v).abs().max().item() <= 2e-5 * scale, k
    assert (got['out.pos_ratio'].item() == 0) == (case == 'none')


# ---- point-wise stacks (csrc/pw_layers.hip), seams of the backbone (csrc/seed_ops.hip) -----------------------------
def _rel(a, b):
    a, b = a.double(), b.double().to(a.device)
    return ((a - b).abs().max() / (b.abs().max() + 1e-30)).item()


def _stream(t):
    from pose2room_amd import _lib
    return _lib.current_stream(t.device)


@pytest.mark.parametrize("B,L,K,R,x_nlc,out_nlc,tr,bias", [(3, 64, 128, 24, 0, 1, 1, 1), (2, 128, 128, 100, 0, 0, 1, 1),
                                                          (1, 192, 256, 259, 0, 1, 1, 1), (2, 64, 48, 33, 1, 1, 1, 0)])
def test_pw_gemm_forward(dev, B, L, K, R, x_nlc, out_nlc, tr, bias):
    """single forward jobs at ragged R / K, with the statistics epilogue (tolerances of test_pw_gpu)"""
    from pose2room_amd.p2rnet import pw_op
    x, W, bvec, fin = cases.pw_gemm_case(B, L, K, R, x_nlc, bias)

    def fn(x, W, fin, bvec=None):
        out = torch.empty((B, L, R) if out_nlc else (B, R, L), device=dev)
        stats = torch.empty((B * L // 64, R, 3), device=dev)
        job = dict(x=pw_op._at(x), w=pw_op._at(W), bias=pw_op._at(bvec), out=pw_op._at(out), stats=pw_op._at(stats), k=K,
                   rows=R, x_ctot=K, x_nlc=x_nlc, out_ctot=R, out_nlc=out_nlc)
        if tr:
            job.update(tr=pw_op._at(fin, 2 * K), tr_mode=1, tr_ld=K)
        pw_op._gemm([job], B, L, _stream(x))
        return out, stats

    ins = dict(x=x, W=W, fin=fin)
    if bias:
        ins['bvec'] = bvec
    got = run_contract(fn, ins, dev)
    xc = (x.transpose(1, 2) if x_nlc else x).double()
    if tr:
        xc = torch.relu(xc * fin[2].double()[None, :, None] + fin[3].double()[None, :, None])
    ref = torch.einsum('rk,bkl->brl', W.double(), xc)
    if bias:
        ref = ref + bvec.double()[None, :, None]
    out, stats = got['out.0'], got['out.1']
    assert _rel(out.transpose(1, 2) if out_nlc else out, ref) < 2e-6
    cols = ref.permute(1, 0, 2).reshape(R, B * L // 64, 64)
    assert torch.all(stats[..., 0] == 64)
    assert _rel(stats[..., 1].t(), cols.mean(-1)) < 1e-5
    assert _rel(stats[..., 2].t(), ((cols - cols.mean(-1, keepdim=True)) ** 2).sum(-1)) < 1e-5


@pytest.mark.parametrize("B,L,K,R,x_nlc,lazy,out_nlc", [(2, 128, 100, 128, 0, 0, 0), (2, 64, 24, 128, 1, 0, 0),
                                                       (1, 128, 259, 256, 1, 0, 0), (1, 64, 33, 48, 1, 1, 0)])
def test_pw_gemm_data_gradient(dev, B, L, K, R, x_nlc, lazy, out_nlc):
    """single data-gradient jobs at ragged K: transposed weights, lazy input form, mask + BatchNorm-backward sums"""
    from pose2room_amd.p2rnet import pw_op
    g, z, W, coef, mz, mfin = cases.pw_data_gradient_case(B, L, K, R, x_nlc)

    def fn(g, z, W, coef, mz, mfin):
        out = torch.empty((B, L, R) if out_nlc else (B, R, L), device=dev)
        part = torch.empty((B * L // 64, R, 2), device=dev)
        job = dict(x=pw_op._at(g), x_nlc=x_nlc, x_ctot=K, w=pw_op._at(W), w_t=1, out=pw_op._at(out), out_ctot=R,
                   out_nlc=out_nlc, stats=pw_op._at(part), k=K, rows=R, epilogue=1, mz=pw_op._at(mz), mz_ctot=R,
                   mfin=pw_op._at(mfin), mfin_ld=R)
        if lazy:
            job.update(x2=pw_op._at(z), tr=pw_op._at(coef), tr_mode=2, tr_ld=K)
        pw_op._gemm([job], B, L, _stream(g))
        return out, part

    got = run_contract(fn, dict(g=g, z=z, W=W, coef=coef, mz=mz, mfin=mfin), dev)
    gd = (g.transpose(1, 2) if x_nlc else g).double()
    zd = (z.transpose(1, 2) if x_nlc else z).double()
    dz = gd
    if lazy:
        c = coef.double()
        dz = c[0][None, :, None] * gd + c[1][None, :, None] * zd + c[2][None, :, None]
    f = mfin.double()
    mask = (mz.to(dev) * mfin[2].to(dev)[None, :, None] + mfin[3].to(dev)[None, :, None]) > 0     # the kernel's fp32 expression
    ref = torch.einsum('kr,bkl->brl', W.double(), dz).to(dev) * mask
    out, part = got['out.0'], got['out.1']
    assert _rel(out.transpose(1, 2) if out_nlc else out, ref) < 2e-6
    xhat = ((mz.double() - f[0][None, :, None]) * f[1][None, :, None]).to(dev)
    tiles = lambda t: t.permute(1, 0, 2).reshape(R, B * L // 64, 64).sum(-1)
    assert _rel(part[..., 0].t(), tiles(ref)) < 1e-5
    assert _rel(part[..., 1].t(), tiles(ref * xhat)) < 1e-5


@pytest.mark.parametrize("B,L,R,K,x_nlc,y_nlc,lazy,ytr", [(2, 128, 100, 128, 0, 0, 0, 1), (2, 64, 24, 128, 1, 0, 0, 1),
                                                         (1, 256, 259, 256, 1, 0, 0, 1), (1, 64, 33, 20, 1, 1, 0, 1),
                                                         (2, 128, 128, 128, 0, 0, 1, 1)])
def test_pw_wgrad_and_reduce(dev, B, L, R, K, x_nlc, y_nlc, lazy, ytr):
    """single weight-gradient jobs at ragged R / K and every split-K factor, reduced by p2r_pw_reduce"""
    from pose2room_amd.p2rnet import pw_op
    g, z, y, coef, yfin = cases.pw_wgrad_case(B, L, R, K, x_nlc, y_nlc)
    chunks = B * L // 64
    gd = (g.transpose(1, 2) if x_nlc else g).double()
    zd = (z.transpose(1, 2) if x_nlc else z).double()
    yd = (y.transpose(1, 2) if y_nlc else y).double()
    dz = gd
    if lazy:
        c = coef.double()
        dz = c[0][None, :, None] * gd + c[1][None, :, None] * zd + c[2][None, :, None]
    if ytr:
        yd = torch.relu(yd * yfin[0].double()[None, :, None] + yfin[1].double()[None, :, None])
    for split in sorted({1, min(3, chunks), chunks}):
        def fn(g, z, y, coef, yfin):
            pw = torch.empty((split, R, K), device=dev)
            pb = torch.empty((split, R), device=dev)
            job = dict(x=pw_op._at(g), x_nlc=x_nlc, x_ctot=R, rows=R, y=pw_op._at(y), y_nlc=y_nlc, y_ctot=K, k=K,
                       dw_part=pw_op._at(pw), db_part=pw_op._at(pb), split=split)
            if lazy:
                job.update(x2=pw_op._at(z), tr=pw_op._at(coef), tr_mode=2, tr_ld=R)
            if ytr:
                job.update(ytr=pw_op._at(yfin), ytr_ld=K)
            pw_op._wgrad([job], B, L, _stream(g))
            dW, db = torch.empty((R, K), device=dev), torch.empty((R,), device=dev)
            pw_op._reduce([(pw, dW), (pb, db)], _stream(g))
            return dW, db, pw, pb

        got = run_contract(fn, dict(g=g, z=z, y=y, coef=coef, yfin=yfin), dev)
        assert _rel(got['out.0'], torch.einsum('brl,bkl->rk', dz, yd)) < 2e-6, split
        assert _rel(got['out.1'], dz.sum((0, 2))) < 2e-6, split


@pytest.mark.parametrize("train", [True, False])
def test_vote_head_and_vote_finish(dev, train):
    """the vote head (multi-job launches) and the whole voting stage (p2r_vote_finish) against the module chain:
    tolerances of test_pw_gpu"""
    from tests.test_model_cpu import build
    from pose2room_amd.p2rnet import pw_op
    from pose2room_amd.p2rnet.modules import vote_center
    net, _ = build('train', 256)
    mod = net.centervoting
    mod.train(train)
    B, S = 3, 512
    seed_xyz, feats = cases.seeded_randn((B, S, 53, 3), 1), cases.seeded_randn((B, S, 256), 2)
    gx, gf, gft = cases.seeded_randn((B, S, 3), 3), cases.seeded_randn((B, S, 256), 4), cases.seeded_randn((B, 256, S), 4)

    def head(fused):
        def fn(seed_xyz, feats, gx, gf, mod):
            with _switch(vote_center, USE_FUSED_HEAD=fused):
                xyz, f = mod(seed_xyz, feats)
                (xyz * gx).sum().add((f * gf).sum()).backward()
            return xyz, f
        return fn

    ins = dict(seed_xyz=seed_xyz, feats=Input(feats, True), gx=gx, gf=gf, mod=mod)
    got = run_contract(head(True), ins, dev)
    ref = run_contract(head(False), ins, dev, fills=())
    assert _rel(got['out.0'], ref['out.0']) < 1e-5 and _rel(got['out.1'], ref['out.1']) < 1e-5
    for k, v in ref.items():
        if k.startswith('grad:'):
            assert _rel(got[k], v) < 2e-4, k
        elif k.startswith('buf:'):
            assert _rel(got[k].float(), v.float()) < 1e-5, k

    def finish(fused):
        def fn(seed_xyz, feats, gx, gft, mod):
            if fused:
                assert pw_op.votes_normalized_supported(mod, seed_xyz, feats)
                xyz, f = pw_op.votes_normalized(mod, seed_xyz, feats)
            else:
                with _switch(vote_center, USE_FUSED_HEAD=False):
                    xyz, f = mod(seed_xyz, feats)
                    f = f.div(torch.norm(f, p=2, dim=2).unsqueeze(2))
            (xyz * gx).sum().add((f.transpose(1, 2) * gft).sum()).backward()
            return xyz, f
        return fn

    ins = dict(seed_xyz=Input(seed_xyz, True), feats=Input(feats, True), gx=gx, gft=gft, mod=mod)
    got = run_contract(finish(True), ins, dev)
    ref = run_contract(finish(False), ins, dev, fills=())
    assert _rel(got['out.0'], ref['out.0']) < 1e-5 and _rel(got['out.1'], ref['out.1']) < 1e-5
    assert _rel(got['grad:feats'], ref['grad:feats']) < 2e-4 and _rel(got['grad:seed_xyz'], ref['grad:seed_xyz']) < 1e-6
    for k, v in ref.items():
        if k.startswith('grad:mod.'):
            assert _rel(got[k], v) < 2e-4, k


@pytest.mark.parametrize("train", [True, False])
def test_proposal_heads(dev, train):
    """the four proposal heads as multi-job launches with the mixture read-out, against the module chain (test_pw_gpu:
    outputs 2e-5, feature gradient 2e-4, parameter gradients 3e-4, buffers 1e-5)"""
    from tests.test_model_cpu import build
    from pose2room_amd.p2rnet import pw_op
    net, _ = build('train', 256)
    mod = net.detection
    mod.train(train)
    B, K, G = 4, 128, 100
    r = cases.seeded_randn
    feats = r((B, 256, K), 1)
    ins = dict(feats=Input(feats, True), ec=r((B * K, G, 1, 3), 2), es=r((B * K, G, 1, 3), 3), eh=r((B * K, G, 1, 2), 4).double(),
               g0=r((B, 3, K), 5), g1=r((B, 3, K), 6), g2=r((B, 2, K), 7).double(), g3=r((B, 24, K), 8), mod=mod)

    def make(fused):
        def fn(feats, ec, es, eh, g0, g1, g2, g3, mod):
            if fused:
                assert pw_op.proposal_heads_supported(mod, feats)
                outs = pw_op.proposal_heads(mod, feats, {'center': ec, 'size': es, 'heading': eh})
            else:
                outs = [mod.gmm_center.predict(mod.conv_center(feats), eps=ec), mod.gmm_size.predict(mod.conv_size(feats), eps=es),
                        mod.gmm_heading.predict(mod.conv_heading(feats), eps=eh), mod.conv_sem_obj(feats)]
            sum((o * g).sum().double() for o, g in zip(outs, (g0, g1, g2, g3))).backward()
            return tuple(outs)
        return fn

    got = run_contract(make(True), ins, dev)
    ref = run_contract(make(False), ins, dev, fills=())
    for i in range(4):
        o, v = got[f'out.{i}'], ref[f'out.{i}']
        assert o.shape == v.shape and o.dtype == v.dtype and _rel(o, v) < 2e-5, i
    assert _rel(got['grad:feats'], ref['grad:feats']) < 2e-4
    params = [k for k in got if k.startswith('grad:mod.')]
    assert params
    for k in params:
        assert got[k].dtype == ref[k].dtype and _rel(got[k], ref[k]) <= 3e-4, k
    for k, v in ref.items():
        if k.startswith('buf:'):
            assert _rel(got[k].float(), v.float()) < 1e-5, k


def test_proposal_heads_eval_means(dev):
    """evaluation read-out (mixture means and weights) under no_grad, against the modules' generate()"""
    from tests.test_model_cpu import build
    from pose2room_amd.p2rnet import pw_op
    net, _ = build('test', 256)
    mod = net.detection.eval()
    feats = cases.seeded_randn((2, 256, 128), 1)

    def make(fused):
        def fn(feats, mod):
            with torch.no_grad():
                if fused:
                    pc, ps, ph, sem, pis = pw_op.proposal_heads(mod, feats, False, return_pi=True)
                    return pc, ps, ph, sem, pis[0], pis[1], pis[2]
                kw = dict(return_pi=True, multi_modes=False, n_samples=1)
                rc, pic = mod.gmm_center.generate(mod.conv_center(feats), **kw)
                rs, pis_ = mod.gmm_size.generate(mod.conv_size(feats), **kw)
                rh, pih = mod.gmm_heading.generate(mod.conv_heading(feats), **kw)
                return rc, rs, rh, mod.conv_sem_obj(feats), pic, pis_, pih
        return fn

    got = run_contract(make(True), dict(feats=feats, mod=mod), dev)
    ref = run_contract(make(False), dict(feats=feats, mod=mod), dev, fills=())
    for i in range(7):
        a, b = got[f'out.{i}'], ref[f'out.{i}']
        assert a.shape == b.shape and a.dtype == b.dtype and _rel(a, b) < 2e-5, i


@pytest.mark.parametrize("f64", [False, True])
def test_mdn_mix(dev, f64):
    """mixture read-out (sampled and mean) and its gradient against the module's torch expression (test_pw_gpu)"""
    from pose2room_amd.p2rnet import pw_op
    from pose2room_amd.p2rnet.config import Struct
    from pose2room_amd.p2rnet.modules.mdn import MixtureDensityHead
    torch.manual_seed(1)
    B, G, L, D = 3, 100, 128, 2 if f64 else 3
    dt = torch.float64 if f64 else torch.float32
    mu0 = torch.randn(G, D, dtype=dt)
    head = MixtureDensityHead(Struct(input_dim=128, num_gaussian=G, out_dim=D, mu_bias_init=mu0, n_samples=1,
                                     central_tendency='mean'))
    head.log_sigma.data.uniform_(-1.5, 0.0)
    logits_all, eps, dpred = torch.randn(B, 2 * G, L), torch.randn(B * L, G, 1, D, dtype=dt), torch.randn(B, L, D, dtype=dt)

    def fn(logits_all, eps, dpred, head):
        pred, = pw_op._mix_forward(logits_all, [G], G, L, [head], [eps])
        mean, = pw_op._mix_forward(logits_all, [G], G, L, [head], [None])
        dlogit = torch.zeros(B, 2 * G, L, device=dev)
        (dmu,), (dls,) = pw_op._mix_backward(logits_all, dlogit, [G], G, L, [head], [eps], [dpred])
        return pred, mean, dlogit, dmu, dls

    got = run_contract(fn, dict(logits_all=logits_all, eps=eps, dpred=dpred, head=head), dev)
    hd = copy.deepcopy(head).to(dev)
    logit = logits_all[:, G:].clone().to(dev).requires_grad_(True)
    pi = torch.sigmoid(logit)
    ref = hd.generate_point_predictions(pi, eps=eps.to(dev))
    assert got['out.0'].dtype == dt
    assert _rel(got['out.0'].transpose(1, 2), ref) < (1e-12 if f64 else 2e-6)
    assert _rel(got['out.1'].transpose(1, 2), hd.get_mean(pi)) < (1e-12 if f64 else 2e-6)
    gl, gmu, gls = torch.autograd.grad(ref, [logit, hd.mu, hd.log_sigma], dpred.to(dev).transpose(1, 2))
    assert torch.all(got['out.2'][:, :G] == 0) and _rel(got['out.2'][:, G:], gl) < 2e-6
    assert _rel(got['out.3'], gmu) < (1e-12 if f64 else 1e-5) and _rel(got['out.4'], gls) < 1e-5


@pytest.mark.parametrize("B,C,T,J,S,kind", [(2, 64, 128, 53, 64, 'sorted'), (3, 8, 40, 5, 100, 'dup'), (2, 4, 16, 7, 300, 'many')])
def test_seed_rows_gather_and_scatter(dev, B, C, T, J, S, kind):
    from pose2room_amd.p2rnet import seed_op
    inds, x, gout = cases.seed_indices(B, T, S, kind), cases.seeded_randn((B, C, T, J), 1), cases.seeded_randn((B, S, C * J), 2)

    def fn(x, inds, gout):
        rows = seed_op.seed_rows(x, inds)
        rows.backward(gout)
        return rows

    got = run_contract(fn, dict(x=Input(x, True), inds=inds, gout=gout), dev)
    xr = x.clone().requires_grad_(True)
    ref = xr.permute(0, 2, 1, 3)[torch.arange(B)[:, None], inds].reshape(B, S, -1)
    ref.backward(gout)
    assert torch.equal(got['out'].cpu(), ref.detach())
    assert _rel(got['grad:x'], xr.grad) < 1e-6 and torch.equal(got['grad:x'].cpu() == 0, xr.grad == 0)


@pytest.mark.parametrize("shape", [(2, 64, 128, 20), (3, 5, 7, 53), (1, 1, 1, 1), (2, 3, 1000, 64)])
def test_rowsum_short(dev, shape):
    """p2r_rowsum_short through mean_last (forward) and add_broadcast_last (gradient of the broadcast operand)"""
    from pose2room_amd.p2rnet import seed_op
    r = cases.seeded_randn
    x, gm, b, a, gy = r(shape, 1), r(shape[:-1], 2), r(shape[:-1], 3), r(shape, 4), r(shape, 5)

    def fn(x, gm, a, b, gy):
        m = seed_op.mean_last(x)
        m.backward(gm)
        y = seed_op.add_broadcast_last(a, b)
        y.backward(gy)
        return m, y

    got = run_contract(fn, dict(x=Input(x, True), gm=gm, a=Input(a, True), b=Input(b, True), gy=gy), dev)
    assert _rel(got['out.0'], x.mean(-1)) < 1e-6
    assert _rel(got['grad:x'], (gm / shape[-1]).unsqueeze(-1).expand(shape)) < 1e-6
    assert torch.equal(got['out.1'].cpu(), a + b.unsqueeze(-1)) and torch.equal(got['grad:a'].cpu(), gy)
    assert _rel(got['grad:b'], gy.double().sum(-1)) < 2e-6


def test_nearest_prefix(dev):
    from pose2room_amd.p2rnet import seed_op
    g = torch.Generator().manual_seed(9)
    for B, T, S in ((4, 256, 512), (2, 341, 100), (1, 20000, 64)):
        cum = cases.arc_length_case(B, T, S, g)
        target = (cum[:, -1] / (S - 1)).unsqueeze(-1) * torch.arange(S, dtype=torch.float)
        got = run_contract(lambda cum, target: seed_op.nearest_prefix(cum, target), dict(cum=cum, target=target), dev)
        want = torch.argmin(torch.abs(cum.to(dev).unsqueeze(-1) - target.to(dev).unsqueeze(1)), dim=1)
        assert torch.equal(got['out'], want)


# ---- batch assembly on the device (csrc/batch_assemble.hip) ---------------------------------------------------------
_STORE_TENSORS = ('joints', 'votes', 'frame_offset', 'n_frames', 'floor_height', 'box_center', 'box_heading', 'box_size',
                  'box_mask', 'box_cls')


@pytest.mark.parametrize("augment,use_height", [(True, True), (False, False)])
def test_device_sample_store_ragged_batch(dev, augment, use_height):
    """one ragged batch (1 .. 5000 source frames, resampled to 768) from a store whose tables lie in guard bands; bit for
    bit the host loader's batch, as in test_device_loader_gpu"""
    from pose2room_amd.p2rnet import device_loader as dv
    from pose2room_amd.p2rnet.synthetic import make_raw_sample
    from tests.test_device_loader_gpu import KEYS, assert_same_batch, host_batch
    rng = np.random.default_rng(5)
    t0 = [1, 2, 5000] + [int(x) for x in rng.integers(1, 3000, 9)]
    samples = [make_raw_sample(t, n_boxes=int(rng.integers(0, 11)), seed=100 + i) for i, t in enumerate(t0)]
    store = dv.DeviceSampleStore.from_samples(samples, device=dev)
    ids, T = [2, 0, 7, 1, 11, 5, 2], 768
    draws = [(int(rng.integers(0, 2)), dv.ANGLES[int(rng.integers(0, 4))], float(rng.uniform(-1, 1))) for _ in ids] if augment else None

    def fn(**tables):
        s = copy.copy(store)                          # the same store over the guarded copies of its tables
        for k, v in tables.items():
            setattr(s, k, v)
        s._c = dv._Store(n_frames_total=store._c.n_frames_total, n_samples=store._c.n_samples, J=store._c.J, K=store._c.K,
                         **{k: v.data_ptr() for k, v in tables.items()})
        out = s.assemble(ids, T, augment, draws, use_height)
        return {k: out[k] for k in KEYS}

    got = run_contract(fn, {k: getattr(store, k).cpu() for k in _STORE_TENSORS}, dev)
    want = host_batch(samples, ids, T, use_height, draws)
    batch = {k: got[f'out.{k}'] for k in KEYS}
    batch['sample_idx'] = want['sample_idx']
    assert_same_batch({k: batch[k] for k in want}, {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in want.items()})
