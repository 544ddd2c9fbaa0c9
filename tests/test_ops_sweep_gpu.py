"""GPU: the PointNet++ and chamfer kernels (csrc/fps.hip, ball_query.hip, group_gather.hip, interpolate.hip, nn_distance.hip,
nms3d.hip) against the float64 references of tests/ops_cases.py, through `pointnet2_ops._ext`, `net_utils.nn_distance` and
`net_utils.nms`, at the shapes that reach every branch of the three host dispatchers (the mirrors of ops_cases name the
branch of each case; tests/test_ops_reference_cpu.py asserts that they cover all of them) and on inputs with real ties,
zero differences, points exactly on a radius or on Huber's delta, tied scores and suppression chains.

Index outputs are EQUAL to the reference (every case is fully decidable, asserted on the CPU); values lie within the
derived bound of ops_cases per element; the deterministic group-gradient forms are bit-equal to the fp32 ascending-slot
sum and to themselves on a second run; the oracle equalities of tests/test_ops_gpu.py are kept.  The gradient kernels
that claim to overwrite their output are launched on raw pointers into NaN-filled tensors, their input lists followed by
in-range indices and large finite values: a destination nobody hits comes back as an exact zero, no NaN survives, and a
kernel that reads past its lists sums what lies behind them.

`test_report` prints the largest error / bound of the session per op (pytest -s)."""
import numpy as np
import pytest
import torch

from tests import cases
from tests import ops_cases as O

pytestmark = pytest.mark.gpu

RATIOS = {}


def _ids(cs):
    return ["-".join(str(v) for v in c) for c in cs]


def _within(op, got, want, bound):
    ratio, at = O.worst(got.cpu(), want, bound)
    RATIOS[op] = max(RATIOS.get(op, 0.0), ratio)
    print(f"{op}: error / bound {ratio:.4f} at {at}")
    assert ratio <= 1, f"{op}: error / bound {ratio:.4f} at {at}"


@pytest.fixture(scope="module")
def ext(dev):
    from pose2room_amd.pointnet2_ops import _ext
    return _ext


@pytest.mark.parametrize("case", O.FPS_SWEEP, ids=_ids(O.FPS_SWEEP))
def test_fps(ext, oracle, dev, case):
    xyz = cases.cloud(case.b, case.n, case.seed, case.kind)
    got = ext.furthest_point_sampling(xyz.to(dev), case.m).cpu()
    assert got.dtype == torch.int32 and got.shape == (case.b, case.m)
    rounds, undecidable = O.fps_check(xyz, got)
    assert undecidable <= 0.01 * rounds
    assert torch.equal(got, oracle.OracleExt.furthest_point_sampling(xyz, case.m))    # the block-size tie rule


@pytest.mark.parametrize("case", O.BALL_SWEEP, ids=[c.name for c in O.BALL_SWEEP])
def test_ball_query(ext, oracle, dev, case):
    xyz, new_xyz = O.ball_inputs(case.name)
    want, undecidable = O.ball_query_ref(xyz, new_xyz, case.radius, case.nsample)
    assert undecidable == 0
    got = ext.ball_query(new_xyz.to(dev), xyz.to(dev), case.radius, case.nsample).cpu()
    assert torch.equal(got, want), f"first mismatch at {(got != want).nonzero()[:3].tolist()}"
    assert torch.equal(got, oracle.OracleExt.ball_query(new_xyz, xyz, case.radius, case.nsample))


@pytest.mark.parametrize("case", O.THREE_NN_SWEEP, ids=_ids(O.THREE_NN_SWEEP))
def test_three_nn(ext, oracle, dev, case):
    unknown, known = O.three_nn_inputs(case)
    dist, idx, undecidable = O.three_nn_ref(unknown, known)
    assert undecidable == 0
    gd, gi = ext.three_nn(unknown.to(dev), known.to(dev))
    gd, gi = gd.cpu(), gi.cpu()
    assert torch.equal(gi, idx)
    k = min(case.m, 3)
    assert torch.isinf(gd[:, :, k:]).all() and (gd[:, :, k:] > 0).all()
    _within("three_nn", gd[:, :, :k], dist[:, :, :k], O.G5 * dist[:, :, :k])
    if O.exact_cloud(unknown, known):
        assert torch.equal(gd[:, :, :k].double(), dist[:, :, :k])
    wd, wi = oracle.OracleExt.three_nn(unknown, known)
    assert torch.equal(gi, wi) and torch.equal(gd, wd)


@pytest.mark.parametrize("case", O.INTERP_SWEEP, ids=_ids(O.INTERP_SWEEP))
def test_three_interpolate_and_grad(ext, oracle, dev, case):
    pts, idx, w, go = O.interp_inputs(case)
    got = ext.three_interpolate(pts.to(dev), idx.to(dev), w.to(dev))
    want, bound = O.three_interpolate_ref(pts, idx, w)
    _within("three_interpolate", got, want, bound)
    assert torch.equal(got.cpu(), oracle.OracleExt.three_interpolate(pts, idx, w))
    got = ext.three_interpolate_grad(go.to(dev), idx.to(dev), w.to(dev), case.m)
    want, bound, _ = O.three_interpolate_grad_ref(go, idx, w, case.m)
    _within("three_interpolate_grad[%s]" % case.form, got, want, bound)


def _group_call(ext, dev, case, pts, idx, go):
    npoints, nsample = O.group_split(case.S)
    if case.op == "group":
        iv = idx.view(case.b, npoints, nsample).to(dev)
        fwd = ext.group_points(pts.to(dev), iv)
        gov = go.view(case.b, case.c, npoints, nsample).to(dev)
        return fwd.reshape(case.b, case.c, case.S), lambda: ext.group_points_grad(gov, iv, case.n)
    return ext.gather_points(pts.to(dev), idx.to(dev)), lambda: ext.gather_points_grad(go.to(dev), idx.to(dev), case.n)


@pytest.mark.parametrize("case", O.GROUP_SWEEP, ids=_ids(O.GROUP_SWEEP))
def test_group_gather_and_grad(ext, oracle, dev, case):
    pts, idx, go = O.group_inputs(case)
    fwd, grad = _group_call(ext, dev, case, pts, idx, go)
    assert torch.equal(fwd.cpu(), O.group_forward_ref(pts, idx))
    got = grad().cpu()
    want, bound, _ = O.group_grad_ref(go, idx, case.n)
    _within("group_grad[%s]" % case.form, got, want, bound)
    if case.form in O.GROUP_ORDERED:
        assert torch.equal(got, O.group_grad_ordered(go, idx, case.n))       # ascending-slot fp32 sums, bit for bit
        assert torch.equal(grad().cpu(), got)                                # and the same on a second run


def _first_per_form(sweep, extra=()):
    seen, out = set(), []
    for c in sweep:
        if c.form not in seen or c.idx_kind in extra:
            seen.add(c.form)
            out.append(c)
    return out


GROUP_RAW = _first_per_form([c for c in O.GROUP_SWEEP if c.op == "group"], extra=("sparse",))
INTERP_RAW = _first_per_form(O.INTERP_SWEEP, extra=("one",))
BAND = 4096          # elements behind every input list: at least the sort form's 4096 keys


def _banded(t, band, dev):
    """(view of a copy of t on the device, its buffer): the copy is followed by `band` in one allocation"""
    buf = torch.cat([t.reshape(-1), band.to(t.dtype)]).to(dev)
    return buf[:t.numel()].view(t.shape), buf


@pytest.mark.parametrize("case", GROUP_RAW, ids=_ids(GROUP_RAW))
def test_group_points_grad_overwrites(dev, case):
    """p2r_group_points_grad on raw pointers into a NaN-filled output (the header: 'overwritten', no zero-fill pass)"""
    from pose2room_amd import _lib
    _, idx, go = O.group_inputs(case)
    npoints, nsample = O.group_split(case.S)
    idx_d, idx_buf = _banded(idx, torch.arange(BAND) % case.n, dev)             # behind the list: valid destinations
    go_d, go_buf = _banded(go, torch.full((BAND,), 1e30), dev)                  # behind the gradient: large finite values
    out = torch.full((case.b, case.c, case.n), float("nan"), device=dev)
    _lib.launch("p2r_group_points_grad", dev, case.b, case.c, case.n, npoints, nsample, go_d, idx_d, out)
    out = out.cpu()
    want, bound, cnt = O.group_grad_ref(go, idx, case.n)
    assert not torch.isnan(out).any(), "an element of grad_points was left unwritten"
    never = (cnt == 0)[:, None].expand_as(out)
    assert not out[never].any(), "a destination without a slot is not zero"
    _within("group_grad[%s]" % case.form, out, want, bound)
    if case.form in O.GROUP_ORDERED:
        assert torch.equal(out, O.group_grad_ordered(go, idx, case.n))
    assert torch.equal(idx_buf[:idx.numel()].cpu(), idx.reshape(-1)) and torch.equal(go_buf[:go.numel()].cpu(), go.reshape(-1))


@pytest.mark.parametrize("case", INTERP_RAW, ids=_ids(INTERP_RAW))
def test_three_interpolate_grad_overwrites(dev, case):
    """p2r_three_interpolate_grad on raw pointers into a NaN-filled output"""
    from pose2room_amd import _lib
    _, idx, w, go = O.interp_inputs(case)
    out = torch.full((case.b, case.c, case.m), float("nan"), device=dev)
    _lib.launch("p2r_three_interpolate_grad", dev, case.b, case.c, case.n, case.m, go.to(dev), idx.to(dev), w.to(dev), out)
    out = out.cpu()
    want, bound, cnt = O.three_interpolate_grad_ref(go, idx, w, case.m)
    assert not torch.isnan(out).any(), "an element of grad_points was left unwritten"
    assert not out[(cnt == 0)[:, None].expand_as(out)].any(), "a destination without a contribution is not zero"
    _within("three_interpolate_grad[%s]" % case.form, out, want, bound)


@pytest.mark.parametrize("case,mode", O.NND_COMBOS, ids=["%s-%s" % ("-".join(map(str, c)), m) for c, m in O.NND_COMBOS])
def test_nn_distance(oracle, dev, case, mode):
    from pose2room_amd.net_utils.nn_distance import nn_distance
    a, q, g1, g2 = O.nnd_inputs(case, mode)
    kw = O.NND_MODES[mode]
    exact = O.nnd_exact(case, mode)
    d1, i1, d2, i2, b1, b2, undecidable = O.nnd_ref(a, q, mode, exact)
    assert undecidable == 0
    ad = a.to(dev).requires_grad_(True)
    qd = q.to(dev).requires_grad_(True)
    got = nn_distance(ad, qd, **kw)
    gi1, gi2 = got[1].cpu(), got[3].cpu()
    assert gi1.dtype == torch.int64 and torch.equal(gi1, i1) and torch.equal(gi2, i2)      # the FIRST minimal index
    for t, want, bound in ((got[0], d1, b1), (got[2], d2, b2)):
        _within("nn_distance[%s]" % mode, t.detach(), want, bound)
        if exact:
            assert torch.equal(t.detach().cpu().double(), want)
    for t, w in zip(got, oracle.nn_distance(a, q, **kw)):
        assert torch.equal(t.detach().cpu(), w)
    (got[0] * g1.to(dev)).sum().add((got[2] * g2.to(dev)).sum()).backward()
    ga, gq, ba, bq = O.nnd_grad_ref(a, q, gi1, gi2, g1, g2, mode)
    _within("nn_distance_grad[%s]" % mode, ad.grad, ga, ba)
    _within("nn_distance_grad[%s]" % mode, qd.grad, gq, bq)
    wa, wq = oracle.nn_distance_grad(a, q, gi1, gi2, g1, g2, **kw)
    assert torch.equal(ad.grad.cpu(), wa) and torch.equal(qd.grad.cpu(), wq)


@pytest.mark.parametrize("case", O.NMS_SWEEP, ids=[c.name for c in O.NMS_SWEEP])
def test_nms3d(oracle, dev, case):
    from pose2room_amd.net_utils import nms
    boxes, valid = O.nms_inputs(case.name)
    want = list(O.nms_expected(case.name))
    stride = 8 if case.same_cls else 7
    bx = np.ascontiguousarray(boxes[:, :stride])
    if valid is None:
        fn = nms.nms_3d_faster_samecls if case.same_cls else nms.nms_3d_faster
        assert fn(bx, case.thr, case.old_type) == want
        assert want == oracle.nms_3d(bx, case.thr, case.old_type, case.same_cls)
    keep, pick, npick = nms.nms_3d_batched(torch.from_numpy(bx).to(dev)[None], case.thr, case.old_type, case.same_cls,
                                           valid=None if valid is None else torch.from_numpy(valid)[None],
                                           return_pick=True)
    n = int(npick[0])
    assert pick[0, :n].tolist() == want and bool((pick[0, n:] == -1).all())
    mask = np.zeros(case.K, np.uint8)
    mask[want] = 1
    assert np.array_equal(keep[0].cpu().numpy(), mask)


def test_report(dev):
    """the largest error / bound per op over this session (1 would be at the bound)"""
    for op in sorted(RATIOS):
        print(f"worst error / bound  {op}: {RATIOS[op]:.4f}")
