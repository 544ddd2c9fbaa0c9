"""CPU: the float64 vote-aggregation reference (tests/sa_votes_cases.py) against a float32 torch chain (conv2d, relu, max)
on the oracle's ball_query indices, and the conditions on the scenes that the GPU sweep (tests/test_sa_votes_sweep_gpu.py)
relies on.

Agreement with the chain ties the reference to the oracle-backed op chain that the golden fixtures pin, and shows that a
correct fp32 implementation stays inside the derived bounds: every stage of the chain is compared on the chain's own
stage input (one-stage bound), the gradients with the reference run on the chain's decisions (cascaded bound).

The scene conditions are asserted here so that the GPU test cannot hide behind them: every branch a scene is there
for is reached, and at most 5e-3 of the decisions of each kind (H > 0, arg-max, out > 0) lie within twice the stage
bound of turning.  A failure of a condition means the scene (its seed) is wrong, not the kernel.
"""
import functools

import pytest
import torch
import torch.nn.functional as F

from tests import sa_votes_cases as V

CAP = 5e-3


@functools.lru_cache(maxsize=None)
def _oracle_idx(name):
    from oracle import cpu_ext
    cpu_ext.build()
    sc = V.scene(name)
    return cpu_ext.OracleExt.ball_query(sc["new_xyz"], sc["xyz"], sc["radius"], V.S)


@functools.lru_cache(maxsize=None)
def _reference(name):
    return V.forward(V.scene(name), _oracle_idx(name))


@functools.lru_cache(maxsize=None)
def _chain(name):
    """the float32 chain with autograd -> (stage tensors, gradients)"""
    sc, idx = V.scene(name), _oracle_idx(name)
    x = {k: sc[k].clone().requires_grad_(True) for k in ("features", "w1", "b1", "w2", "b2")}
    G = V.gather(x["features"], idx)
    z1 = F.conv2d(G, x["w1"].view(V.C, V.C, 1, 1), x["b1"])
    H = torch.relu(z1)
    z2 = F.conv2d(H, x["w2"].view(V.C, V.C, 1, 1), x["b2"])
    out, amax = torch.relu(z2).max(3)
    out.backward(sc["dout"])
    stages = {k: v.detach() for k, v in (("G", G), ("z1", z1), ("H", H), ("z2", z2), ("out", out), ("amax", amax))}
    return stages, {k: v.grad for k, v in x.items()}


@pytest.mark.parametrize("name", V.NAMES)
def test_plain_ball_query_is_the_oracle(oracle, name):
    """the hit counts below come from a plain-torch ball query: it must give the oracle's indices"""
    sc = V.scene(name)
    idx, cnt = V.ball_query(sc["xyz"], sc["new_xyz"], sc["radius"])
    assert idx.dtype == torch.int32 and torch.equal(idx, _oracle_idx(name))
    assert torch.equal(cnt.clamp(max=V.S), (V.first_slot(idx.long()) == torch.arange(V.S)).sum(-1) * (cnt > 0))


@pytest.mark.parametrize("name", V.NAMES)
def test_forward_stages_within_bound(oracle, name):
    sc, idx = V.scene(name), _oracle_idx(name)
    got, _ = _chain(name)
    assert torch.equal(got["G"], V.gather(sc["features"], idx))
    z1, E1 = V.layer(sc["w1"], sc["b1"], got["G"])
    z2, E2 = V.layer(sc["w2"], sc["b2"], got["H"])
    out, _ = V.pool(z2, idx)
    for stage, g, want, bound in (("z1", got["z1"], z1, E1), ("H", got["H"], torch.relu(z1), E1), ("z2", got["z2"], z2, E2),
                                  ("out", got["out"], out, E2.max(-1).values)):
        ratio, at = V.worst(g, want, bound)
        print(f"{name} {stage}: worst error / bound {ratio:.4f} at {at}")
        assert ratio <= 1, (stage, ratio, at)
    # the reference on its own H: the same values up to the first layer's bound pushed through the second
    ref = _reference(name)
    assert torch.equal(ref["G"], got["G"])
    assert ((ref["z1"] - got["z1"].double()).abs() <= ref["E1"]).all()


@pytest.mark.parametrize("name", V.NAMES)
def test_reference_decisions(oracle, name):
    """first index on ties, and the chain's decisions differ from the reference's own only where undecided"""
    idx = _oracle_idx(name).long()
    ref, (got, _) = _reference(name), _chain(name)
    und = V.margins(ref["z1"], ref["E1"], ref["z2"], ref["E2"], idx)
    amax, out = ref["amax"], ref["out"]
    assert (amax[out == 0] == 0).all()                                  # all tie at 0: the lowest sample
    assert torch.equal(V.first_slot(idx)[:, None].expand(-1, V.C, -1, -1).gather(3, amax[..., None])[..., 0], amax)
    point = lambda a: idx[:, None].expand(-1, V.C, -1, -1).gather(3, a[..., None])[..., 0]
    diff = {"h": (got["H"] > 0) != ref["active"], "out": (got["out"] > 0) != (out > 0),
            "arg": (point(got["amax"]) != point(amax)) & (got["out"] > 0) & (out > 0)}
    for k, d in diff.items():
        print(f"{name} {k}: {int(d.sum())} decisions of the fp32 chain differ from the reference's, "
              f"{int(und[k].sum())} of {d.numel()} undecided")
        assert not (d & ~und[k]).any(), k


@pytest.mark.parametrize("name", V.NAMES)
def test_gradients_within_cascaded_bound(oracle, name):
    sc, idx = V.scene(name), _oracle_idx(name)
    got, grads = _chain(name)
    fwd = V.forward(sc, idx, active=got["H"] > 0)
    want = V.backward(sc, fwd, amax=got["amax"], positive=got["out"] > 0, split=1)
    for k, r in (("features", "dfeat"), ("w1", "dw1"), ("b1", "db1"), ("w2", "dw2"), ("b2", "db2")):
        value, bound = want[r]
        assert grads[k].shape == value.shape
        ratio, at = V.worst(grads[k], value, bound)
        print(f"{name} {r}: worst error / bound {ratio:.4f} at {at}")
        assert ratio <= 1, (r, ratio, at)


def test_backward_stages_compose(oracle):
    """the per-stage functions, chained on their own outputs, are the end-to-end backward"""
    sc, ref = V.scene("walk"), _reference("walk")
    want = V.backward(sc, ref, split=64)
    dZ2 = V.dz2_stage(sc["dout"].double(), ref["amax"], ref["out"] > 0)
    dZ1, _ = V.dz1_stage(sc["w2"], dZ2, ref["active"])
    dG, _ = V.dg_stage(sc["w1"], dZ1)
    stages = {"dZ2": dZ2, "dZ1": dZ1, "dG": dG, "dfeat": V.dfeat_stage(dG, ref["idx"], sc["features"].shape[2])[0],
              "dw1": V.dw_stage(dZ1, ref["G"], 64)[0], "dw2": V.dw_stage(dZ2, ref["H"], 64)[0],
              "db1": V.db_stage(dZ1)[0], "db2": V.db_stage(dZ2)[0]}
    for k, v in stages.items():
        assert torch.equal(v, want[k][0]), k
    for k in ("dfeat", "dw1", "dw2", "db1", "db2"):             # a cascaded bound is never below the one-stage bound
        assert (want[k][1] >= 0).all() and torch.isfinite(want[k][1]).all()
    assert (want["dw1"][1] >= V.dw_stage(dZ1, ref["G"], 64)[1]).all()
    # one non-zero per (channel, ball) at most, none where the pooled output is 0
    assert ((dZ2 != 0).sum(-1) <= 1).all() and not dZ2[(ref["out"] == 0)].any()


@pytest.mark.parametrize("name", V.NAMES)
def test_undecided_share(oracle, name):
    ref = _reference(name)
    und = V.margins(ref["z1"], ref["E1"], ref["z2"], ref["E2"], _oracle_idx(name).long())
    for k, u in und.items():
        share = u.double().mean().item()
        print(f"{name} undecided {k}: {share:.2e}")
        assert share <= CAP, (k, share)


def _counts(name):
    sc = V.scene(name)
    return V.ball_query(sc["xyz"], sc["new_xyz"], sc["radius"], sc["xyz"].shape[1])     # every hit, in order


def test_scene_table(oracle):
    for s in V.SCENES:
        full, cnt = _counts(s.name)
        ref = _reference(s.name)
        print(f"{s.name}: B,N,M {s.B},{s.N},{s.M}  counts {int(cnt.min())}..{int(cnt.max())}  "
              f"out == 0: {(ref['out'] == 0).double().mean().item():.3f}  arg-max samples: "
              f"{sorted(set(ref['amax'][ref['out'] > 0].tolist()))}")
        sc = V.scene(s.name)
        assert sc["xyz"].shape == (s.B, s.N, 3) and sc["new_xyz"].shape == (s.B, s.M, 3)
        assert sc["features"].shape == (s.B, V.C, s.N) and sc["dout"].shape == (s.B, V.C, s.M)
        assert sc["w1"].abs().max() <= 2.4 / 16 and sc["w2"].abs().max() <= 2.4 / 16
    assert [(s.B, s.N, s.M) for s in V.SCENES] == [(2, 200, 9), (1, 130, 13), (1, 600, 6), (3, 64, 6), (1, 33, 1),
                                                   (5, 5, 3), (1, 40, 5)]


def test_walk_reaches(oracle):
    full, cnt = _counts("walk")
    ref = _reference("walk")
    assert (cnt >= V.S).sum() >= 16 and cnt.max() > 64                  # full balls, some with more hits than a trip holds
    early = (cnt >= 17) & (full[..., V.S - 1] < 192)                    # the 16th hit before the last of the 4 trips
    assert early.any() and (full[..., V.S - 1] < 64).any() and (full[..., V.S - 1] >= 64).any()
    assert V.BY_NAME["walk"].M % 4 == 1 and V.BY_NAME["walk"].N == 200  # last workgroup: one live wave; 4 trips of 64
    zero, pos = (ref["out"] == 0).double().mean().item(), (ref["out"] > 0).double().mean().item()
    assert zero >= 0.2 and pos >= 0.2, (zero, pos)
    assert len(set(ref["amax"][ref["out"] > 0].tolist())) >= 8


def test_partial_reaches(oracle):
    _, cnt = _counts("partial")
    ref = _reference("partial")
    assert ((cnt >= 2) & (cnt <= 15)).any() and (cnt >= 17).any()
    group = torch.arange(V.BY_NAME["partial"].M) // 4                                      # padded and full balls in one workgroup
    assert any(((cnt[0][group == g] < V.S).any() and (cnt[0][group == g] >= V.S).any()) for g in range(4))
    assert V.BY_NAME["partial"].N % 64 != 0
    zero, pos = (ref["out"] == 0).double().mean().item(), (ref["out"] > 0).double().mean().item()
    assert zero >= 0.2 and pos >= 0.2, (zero, pos)


def test_edge_reaches(oracle):
    sc = V.scene("edge")
    full, cnt = _counts("edge")
    d2 = ((sc["new_xyz"].double()[:, :, None] - sc["xyz"].double()[:, None]) ** 2).sum(-1)   # multiples of 1/16: exact
    on = d2 == sc["radius"] ** 2
    assert sc["radius"] ** 2 == 0.25 and on.any()
    assert not (on & V.ball_hits(sc["xyz"], sc["new_xyz"], sc["radius"])).any()              # strict <: outside
    b, m, n = (t[0].item() for t in on.nonzero(as_tuple=True))
    assert n not in full[b, m, :int(cnt[b, m])].tolist()
    # a point on the radius in front of the 16th hit: `<=` would change the oracle's 16 indices
    assert (on & (torch.arange(V.BY_NAME["edge"].N) <_oracle_idx("edge").long().max(-1).values[..., None]) & (cnt[..., None] > 0)).any()
    pts = sc["xyz"][0]
    assert len(torch.unique(pts, dim=0)) < len(pts)                                          # duplicate points


def test_small_scenes_reach(oracle):
    _, cnt = _counts("dup")
    assert (cnt == 1).any() and V.scene("dup")["xyz"].shape[1] == 64
    one = (cnt == 1)
    assert (_oracle_idx("dup")[one] == _oracle_idx("dup")[one][:, :1]).all()                 # 16 identical columns
    _, cnt = _counts("m3b")
    assert (cnt == 5).all()                                                                  # all points, then padding
    _, cnt = _counts("empty")
    assert (cnt == 0).all() and not _oracle_idx("empty").any()
    assert V.BY_NAME["m1"].M == 1 and V.BY_NAME["m3b"].M < 4


def test_gemm_ranges_tile_the_columns():
    """the ranges of every case cover [0, nb L) once, in order, in whole chunks but for the last"""
    assert V.GEMM_CASES == [(1, 16, 1), (1, 64, 1), (4, 64, 3), (3, 48, 4), (1, 592, 64), (2, 128, 64), (1, 16, 1024)]
    for nb, L, split in V.GEMM_CASES:
        r = V.gemm_ranges(nb, L, split)
        assert len(r) == split and r[0][0] == 0 and max(hi for _, hi in r) == nb * L
        assert all(a[1] == b[0] or b[0] == b[1] == nb * L for a, b in zip(r, r[1:]))
        assert all((hi - lo) % 64 == 0 or hi == nb * L for lo, hi in r)
    assert V.gemm_ranges(4, 64, 3) == [(0, 128), (128, 256), (256, 256)]
    assert V.gemm_ranges(3, 48, 4) == [(0, 64), (64, 128), (128, 144), (144, 144)]
    assert sum(hi > lo for lo, hi in V.gemm_ranges(1, 592, 64)) == 10
    assert sum(hi > lo for lo, hi in V.gemm_ranges(2, 128, 64)) == 4
    assert sum(hi > lo for lo, hi in V.gemm_ranges(1, 16, 1024)) == 1
    A, B = V.gemm_operands(3, 48)
    parts = sum(V.gemm_reference(A, B, lo, hi)[0] for lo, hi in V.gemm_ranges(3, 48, 4))
    full = torch.einsum("bml,bnl->mn", A.double(), B.double())
    assert (parts - full).abs().max() <= 1e-12 * full.abs().max()
