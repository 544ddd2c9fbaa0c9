"""CPU: the float64 references of tests/ops_cases.py against the C oracle (oracle/p2r_oracle.c) on every case of the sweep,
under the bounds and equalities tests/test_ops_sweep_gpu.py then holds the HIP kernels to; the caps on undecidable
comparisons (none for ball_query, three_nn and nn_distance, 1 % of the rounds for FPS: a seed that breaks a cap is changed,
never the bound); the three host-selection mirrors against the branch every case names."""
import numpy as np
import pytest
import torch

from tests import cases
from tests import ops_cases as O


def _ids(cs):
    return ["-".join(str(v) for v in c) for c in cs]


# ---- the mirrors ---------------------------------------------------------------------------------------------------------------
def test_group_mirror_reaches_every_branch():
    got = set()
    for c in O.GROUP_SWEEP:
        form = O.group_grad_form(c.b, c.c, c.n, c.S)
        assert form == c.form, c
        got.add(form)
    assert got == O.GROUP_FORMS
    assert [O.group_sort_np(S)[0] for S in (256, 257, 4093, 4096)] == [256, 512, 4096, 4096]
    # the deterministic forms, each with all slots on one destination
    assert {c.form for c in O.GROUP_SWEEP if c.idx_kind == "one"} == O.GROUP_ORDERED
    # the sort form with padded slots (S % 4 != 0), in both chunk sizes, and with a last chunk of fewer rows
    assert {c.form for c in O.GROUP_SWEEP if c.form.startswith("sort") and c.S % 4} == {"sort8", "sort4"}
    assert any(c.form == "sort8" and c.c % 8 for c in O.GROUP_SWEEP)
    assert O.group_grad_form(0, 3, 5, 7) == O.group_grad_form(2, 3, 0, 7) == "noop"


def test_interp_mirror_reaches_every_branch():
    got = set()
    for c in O.INTERP_SWEEP:
        form = O.interp_grad_form(c.b, c.c, c.n, c.m)
        assert form == c.form, c
        got.add(form)
    assert got == O.INTERP_FORMS


def test_fps_mirror_reaches_every_branch():
    """the sweep adds the upper side of every tiling boundary, the LDS switch, coop<16> and the streaming kernel; the
    cases of tests/cases.py (test_ops_gpu.py) bring coop<4> and coop<8>.  No shape reaches 'coop1'."""
    got = set()
    for c in O.FPS_SWEEP:
        form = O.fps_form(c.b, c.n)
        assert form == c.form, c
        got.add(form)
    got |= {O.fps_form(b, n) for b, n, _, _, _ in cases.FPS_CASES}
    assert got == O.FPS_FORMS
    for b in range(1, 300):                               # S = ceil(n / G) > 1024 whenever the co-operative kernel runs
        for n in (16385, 16400, 20000):
            G = 1
            while G * 2 <= 16 and b * G * 2 <= O.MI355X_CUS:
                G *= 2
            assert G == 1 or -(-n // G) > 1024


# ---- references against the oracle ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", O.FPS_SWEEP, ids=_ids(O.FPS_SWEEP))
def test_fps_oracle_within_reference(oracle, case):
    xyz = cases.cloud(case.b, case.n, case.seed, case.kind)
    picks = oracle.OracleExt.furthest_point_sampling(xyz, case.m)
    rounds, undecidable = O.fps_check(xyz, picks)
    assert rounds == case.b * (case.m - 1)
    assert undecidable <= 0.01 * rounds


def test_fps_check_rejects_wrong_picks():
    xyz = cases.cloud(1, 100, 1)
    picks = torch.zeros(1, 5, dtype=torch.int32)          # point 0 five times: not the furthest after round one
    with pytest.raises(AssertionError):
        O.fps_check(xyz, picks)
    near = cases.cloud(1, 200, 9, "near_origin")
    good = torch.tensor([[0, 0]], dtype=torch.int32)
    mag = (near[0] ** 2).sum(-1)
    good[0, 1] = int(torch.where(mag < 1e-3, torch.full_like(mag, 1e9), torch.zeros_like(mag)).argmax())
    with pytest.raises(AssertionError, match="skip ball"):
        O.fps_check(near, good)


@pytest.mark.parametrize("case", O.BALL_SWEEP, ids=[c.name for c in O.BALL_SWEEP])
def test_ball_query_oracle_equals_reference(oracle, case):
    xyz, new_xyz = O.ball_inputs(case.name)
    want, undecidable = O.ball_query_ref(xyz, new_xyz, case.radius, case.nsample)
    assert undecidable == 0
    assert torch.equal(oracle.OracleExt.ball_query(new_xyz, xyz, case.radius, case.nsample), want)


def test_ball_query_cases_hold_their_edges():
    """what the case names promise: a point exactly on the radius (excluded by the strict <), hits on both sides of point
    2048, balls with more hits than slots and balls with fewer, an empty ball"""
    for name in ("half_r050", "half_r075", "latt_r1"):
        c = O.BALL_BY_NAME[name]
        xyz, new_xyz = O.ball_inputs(name)
        d = O.sqdist64(new_xyz, xyz)
        assert int((d == O.radius2(c.radius)).sum()) > 0, name
    c = O.BALL_BY_NAME["straddle"]
    idx, _ = O.ball_query_ref(*O.ball_inputs("straddle"), c.radius, c.nsample)
    hits = sorted(set(idx[0, 0].tolist()))
    assert set(range(2040, 2056)) <= set(hits) and len(hits) < c.nsample and idx[0, 0, len(hits):].eq(hits[0]).all()
    c = O.BALL_BY_NAME["n4097_m1"]
    d = O.sqdist64(*reversed(O.ball_inputs("n4097_m1")))
    assert int((d < O.radius2(c.radius)).sum()) > c.nsample
    idx, _ = O.ball_query_ref(*O.ball_inputs("empty"), 0.3, 16)
    assert not idx.any()


@pytest.mark.parametrize("case", O.THREE_NN_SWEEP, ids=_ids(O.THREE_NN_SWEEP))
def test_three_nn_oracle_within_reference(oracle, case):
    unknown, known = O.three_nn_inputs(case)
    dist, idx, undecidable = O.three_nn_ref(unknown, known)
    assert undecidable == 0
    gd, gi = oracle.OracleExt.three_nn(unknown, known)
    assert torch.equal(gi, idx)
    k = min(case.m, 3)
    assert torch.isinf(gd[:, :, k:]).all() and (gd[:, :, k:] > 0).all() and not gi[:, :, k:].any()
    ratio, at = O.worst(gd[:, :, :k], dist[:, :, :k], O.G5 * dist[:, :, :k])
    assert ratio <= 1, (ratio, at)
    if O.exact_cloud(unknown, known):
        assert torch.equal(gd[:, :, :k].double(), dist[:, :, :k])


@pytest.mark.parametrize("case", O.INTERP_SWEEP, ids=_ids(O.INTERP_SWEEP))
def test_three_interpolate_oracle_within_reference(oracle, case):
    pts, idx, w, go = O.interp_inputs(case)
    want, bound = O.three_interpolate_ref(pts, idx, w)
    ratio, at = O.worst(oracle.OracleExt.three_interpolate(pts, idx, w), want, bound)
    assert ratio <= 1, (ratio, at)
    want, bound, cnt = O.three_interpolate_grad_ref(go, idx, w, case.m)
    assert float(cnt.sum()) == case.b * case.n * 3
    got = oracle.OracleExt.three_interpolate_grad(go, idx, w, case.m)
    ratio, at = O.worst(got, want, bound)
    assert ratio <= 1, (ratio, at)
    assert not got[(cnt == 0)[:, None].expand_as(got)].any()
    if case.idx_kind == "pair":
        assert bool((idx[:, ::2, 0] == idx[:, ::2, 1]).all())
    if case.idx_kind == "one":
        assert int((cnt > 0).sum()) == case.b and float(cnt.max()) == case.n * 3


@pytest.mark.parametrize("case", O.GROUP_SWEEP, ids=_ids(O.GROUP_SWEEP))
def test_group_oracle_within_reference(oracle, case):
    pts, idx, go = O.group_inputs(case)
    npoints, nsample = O.group_split(case.S)
    assert npoints * nsample == case.S and int(idx.min()) >= 0 and int(idx.max()) < case.n
    want, bound, cnt = O.group_grad_ref(go, idx, case.n)
    if case.op == "group":
        fwd = oracle.OracleExt.group_points(pts, idx.view(case.b, npoints, nsample))
        got = oracle.OracleExt.group_points_grad(go.view(case.b, case.c, npoints, nsample),
                                                 idx.view(case.b, npoints, nsample), case.n)
    else:
        fwd = oracle.OracleExt.gather_points(pts, idx)
        got = oracle.OracleExt.gather_points_grad(go, idx, case.n)
    assert torch.equal(fwd.reshape(case.b, case.c, case.S), O.group_forward_ref(pts, idx))
    ratio, at = O.worst(got, want, bound)
    assert ratio <= 1, (ratio, at)
    if case.form in O.GROUP_ORDERED:
        # the oracle's sequential loop IS the ascending-slot fp32 sum, bit for bit
        assert torch.equal(got, O.group_grad_ordered(go, idx, case.n))
    if case.idx_kind == "one":
        assert float(cnt.max()) == case.S and int((cnt > 0).sum()) == case.b
    if case.idx_kind == "sparse":
        assert int((cnt > 0).sum()) <= 3 * case.b


@pytest.mark.parametrize("case,mode", O.NND_COMBOS, ids=["%s-%s" % ("-".join(map(str, c)), m) for c, m in O.NND_COMBOS])
def test_nn_distance_oracle_within_reference(oracle, case, mode):
    a, q, g1, g2 = O.nnd_inputs(case, mode)
    exact = O.nnd_exact(case, mode)
    d1, i1, d2, i2, b1, b2, undecidable = O.nnd_ref(a, q, mode, exact)
    assert undecidable == 0
    od1, oi1, od2, oi2 = oracle.nn_distance(a, q, **O.NND_MODES[mode])
    assert torch.equal(oi1, i1) and torch.equal(oi2, i2)
    for got, want, bound in ((od1, d1, b1), (od2, d2, b2)):
        ratio, at = O.worst(got, want, bound)
        assert ratio <= 1, (ratio, at)
        if exact:
            assert torch.equal(got.double(), want)
    ga, gq, ba, bq = O.nnd_grad_ref(a, q, oi1, oi2, g1, g2, mode)
    oa, oq = oracle.nn_distance_grad(a, q, oi1, oi2, g1, g2, **O.NND_MODES[mode])
    for got, want, bound in ((oa, ga, ba), (oq, gq, bq)):
        ratio, at = O.worst(got, want, bound)
        assert ratio <= 1, (ratio, at)


def test_nn_distance_cases_hold_their_edges():
    """lattice inputs give arg-min ties and zero differences; the 'ondelta' inputs differences of exactly +-delta"""
    ties = zeros = 0
    for case in O.NND_SWEEP:
        if case.kind not in ("lattice", "halflattice"):
            continue
        a, q, _, _ = O.nnd_inputs(case, "l2")
        D = O.nnd_matrix(a, q, "l2")
        ties += int(((D == D.min(2, keepdim=True).values).sum(2) > 1).sum())
        zeros += int((a[:, :, None, :] == q[:, None, :, :]).sum())
    assert ties > 20 and zeros > 100
    for mode in ("huber1", "huber03"):
        for case in O.NND_SWEEP:
            if case.kind != "ondelta":
                continue
            a, q, _, _ = O.nnd_inputs(case, mode)
            diff = a[:, :, None, :] - q[:, None, :, :]                  # fp32, as the kernel forms it
            assert int((diff.abs() == np.float32(O.nnd_delta(mode))).sum()) >= 8
            assert int((diff == 0).all(-1).sum()) >= 2


@pytest.mark.parametrize("mode", list(O.NND_MODES))
def test_nn_distance_gather_gradient_is_the_autograd_of_the_formula(mode):
    """tie-free inputs: the gather form with the float64 arg-min indices against torch autograd of the reference formula"""
    case = O.NndCase(2, 13, 11, 3, "randn", 899)
    a, q, g1, g2 = O.nnd_inputs(case, mode)
    i1, i2, ga, gq = O.nnd_autograd(a, q, g1, g2, mode)
    _, r1, _, r2, _, _, undecidable = O.nnd_ref(a, q, mode)
    assert undecidable == 0 and torch.equal(r1, i1) and torch.equal(r2, i2)
    wa, wq, _, _ = O.nnd_grad_ref(a, q, i1, i2, g1, g2, mode)
    torch.testing.assert_close(wa, ga, rtol=1e-13, atol=1e-13)
    torch.testing.assert_close(wq, gq, rtol=1e-13, atol=1e-13)


@pytest.mark.parametrize("case", O.NMS_SWEEP, ids=[c.name for c in O.NMS_SWEEP])
def test_nms3d_oracle_equals_reference(oracle, case):
    boxes, valid = O.nms_inputs(case.name)
    want = list(O.nms_expected(case.name))
    sel = np.arange(case.K) if valid is None else np.where(valid)[0]
    stride = 8 if case.same_cls else 7
    got = [int(sel[j]) for j in oracle.nms_3d(boxes[sel][:, :stride], case.thr, case.old_type, case.same_cls)] \
        if len(sel) else []
    assert got == want
    if case.kind.startswith("chain"):                   # every kept box suppressed the next one
        assert len(want) == (case.K + 1) // 2 and all(abs(x - y) == 2 for x, y in zip(want, want[1:]))
    if case.kind in ("ties", "allequal") and valid is None:
        assert len(set(boxes[:, 6])) <= 4 and len(want) > 4
    if case.valid == "one":
        assert len(want) == 1
    if case.valid == "none":
        assert want == []


def test_nms3d_reference_tie_rule():
    """two identical boxes with equal scores: the HIGHER index is picked and suppresses the lower"""
    boxes = np.array([[0, 0, 0, 1, 1, 1, 0.5, 0], [0, 0, 0, 1, 1, 1, 0.5, 0], [5, 5, 5, 6, 6, 6, 0.5, 0]], np.float64)
    assert O.nms3d_ref(boxes, 0.25) == [2, 1]
