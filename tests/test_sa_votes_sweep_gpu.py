"""GPU: the vote-aggregation kernels (csrc/sa_votes.hip) stage by stage against the float64 reference of
tests/sa_votes_cases.py, over the scenes of that file -- full, padded, one-point and empty balls, distances exactly on
the radius, dead waves, M < 4, N < 16, pooled outputs that are exactly 0 -- then p2r_gemm_nt_256 called directly, the
refused and empty calls, and the wiring of pointnet2_ops/fused.py end to end.

Every stage is evaluated on the kernel's OWN stage input (H on the kernel's G, out on the kernel's H, dZ1 on the kernel's
dZ2, ...), so its bound is the one-stage running-error bound derived in sa_votes_cases.py: nothing here is a measured
tolerance.  Copies and selections (idx, G, dZ2, the zeros of H and dZ1) are compared bit for bit.  The decisions (H > 0,
arg-max, out > 0) may differ from the reference's own only where the reference's margin is below twice its bound;
tests/test_sa_votes_reference_cpu.py caps how many such elements a scene holds.  The end-to-end gradients run the
reference on the kernel's decisions, validated stage by stage before, under the cascaded bound.

Each test prints the worst error / bound of its stages with the element it occurred at, and the number of kernel
decisions that differ from the reference's own.
"""
import pytest
import torch

from tests import sa_votes_cases as V

pytestmark = pytest.mark.gpu

POISON = 3.0e38
POISON_I = -7
POISON_B = 0xAB
EINVAL = "failed with status -22"
_RUNS, _REFS, _E2E = {}, {}, {}


def _full(shape, dev, dtype=torch.float32):
    fill = {torch.float32: POISON, torch.int32: POISON_I, torch.uint8: POISON_B}[dtype]
    return torch.full(shape, fill, dtype=dtype, device=dev)


def _forward_buffers(dev, B, M, train=True):
    o = {"idx": _full((B, M, V.S), dev, torch.int32), "out": _full((B, V.C, M), dev)}
    if train:
        o.update(G=_full((B, V.C, M, V.S), dev), H=_full((B, V.C, M, V.S), dev), amax=_full((B, V.C, M), dev, torch.uint8))
    return o


def _forward(dev, d, radius, train=True, o=None, **over):
    """p2r_sa_votes_forward through the raw ABI on poison-filled outputs -> the output buffers"""
    from pose2room_amd import _lib
    B, N, _ = d["xyz"].shape
    M = d["new_xyz"].shape[1]
    o = _forward_buffers(dev, B, M, train) if o is None else o
    a = dict(b=B, n=N, m=M, nsample=V.S, C0=V.C, C1=V.C, C2=V.C, G=o.get("G"), H=o.get("H"), amax=o.get("amax"))
    a.update(over)
    _lib.launch("p2r_sa_votes_forward", dev, a["b"], a["n"], a["m"], a["nsample"], radius, a["C0"], a["C1"], a["C2"],
                d["xyz"], d["new_xyz"], d["features"], d["w1"], d["b1"], d["w2"], d["b2"], o["idx"], o["out"],
                a["G"], a["H"], a["amax"])
    return o


def _backward(dev, d, f, o=None, **over):
    from pose2room_amd import _lib
    B, _, M = f["out"].shape
    o = {k: _full((B, V.C, M, V.S), dev) for k in ("dZ2", "dZ1", "dG")} if o is None else o
    a = dict(b=B, m=M)
    a.update(over)
    _lib.launch("p2r_sa_votes_backward", dev, a["b"], a["m"], V.S, V.C, d["dout"], f["out"], f["amax"], f["H"], d["w2t"],
                d["w1t"], o["dZ2"], o["dZ1"], o["dG"])
    return o


def _device_inputs(dev, sc):
    d = {k: sc[k].to(dev) for k in V.INPUTS}
    d["w2t"], d["w1t"] = d["w2"].t().contiguous(), d["w1"].t().contiguous()
    return d


def _run(dev, name):
    """one scene through the raw ABI: training forward twice, inference forward, backward twice -> CPU tensors"""
    if name not in _RUNS:
        sc = V.scene(name)
        d = _device_inputs(dev, sc)
        f = _forward(dev, d, sc["radius"])
        f2 = _forward(dev, d, sc["radius"])
        inf = _forward(dev, d, sc["radius"], train=False)
        g = _backward(dev, d, f)
        g2 = _backward(dev, d, f)
        torch.cuda.synchronize()
        cpu = lambda t: {k: v.cpu() for k, v in t.items()}
        _RUNS[name] = {"fwd": cpu(f), "fwd2": cpu(f2), "inf": cpu(inf), "bwd": cpu(g), "bwd2": cpu(g2)}
    return _RUNS[name]


def _ref(dev, name):
    """the reference of each forward stage on the kernel's input of that stage"""
    if name not in _REFS:
        sc, f = V.scene(name), _run(dev, name)["fwd"]
        z1, E1 = V.layer(sc["w1"], sc["b1"], f["G"])
        z2, E2 = V.layer(sc["w2"], sc["b2"], f["H"])
        out, amax = V.pool(z2, f["idx"].long())
        _REFS[name] = {"z1": z1, "E1": E1, "z2": z2, "E2": E2, "out": out, "amax": amax,
                       "undecided": V.margins(z1, E1, z2, E2, f["idx"].long())}
    return _REFS[name]


def _report(name, stage, got, want, bound):
    ratio, at = V.worst(got, want, bound)
    print(f"{name} {stage}: worst error / bound {ratio:.4f} at {at}")
    assert ratio <= 1, (name, stage, ratio, at)


# ---- forward --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", V.NAMES)
def test_indices_and_gather(oracle, dev, name):
    sc, f = V.scene(name), _run(dev, name)["fwd"]
    assert torch.equal(f["idx"], oracle.OracleExt.ball_query(sc["new_xyz"], sc["xyz"], sc["radius"], V.S))
    assert torch.equal(f["G"], V.gather(sc["features"], f["idx"]))


@pytest.mark.parametrize("name", V.NAMES)
def test_hidden_layer(dev, name):
    f, r = _run(dev, name)["fwd"], _ref(dev, name)
    H, z1, E1 = f["H"], r["z1"], r["E1"]
    _report(name, "H", H, torch.relu(z1), E1)
    assert (H[z1 < -E1] == 0).all() and (H[z1 > E1] > 0).all() and (H >= 0).all()
    differ = (H > 0) != (z1 > 0)
    print(f"{name} H > 0: {int(differ.sum())} of {differ.numel()} decisions differ from the reference's")
    assert not (differ & ~r["undecided"]["h"]).any()


@pytest.mark.parametrize("name", V.NAMES)
def test_pooled_output(dev, name):
    f, r = _run(dev, name)["fwd"], _ref(dev, name)
    out, z2, E2 = f["out"], r["z2"], r["E2"]
    _report(name, "out", out, r["out"], E2.max(-1).values)
    assert (out[(z2 < -E2).all(-1)] == 0).all() and (out >= 0).all()
    differ = (out > 0) != (r["out"] > 0)
    print(f"{name} out > 0: {int(differ.sum())} of {differ.numel()} decisions differ from the reference's")
    assert not (differ & ~r["undecided"]["out"]).any()


@pytest.mark.parametrize("name", V.NAMES)
def test_arg_max(dev, name):
    f, r = _run(dev, name)["fwd"], _ref(dev, name)
    amax, idx = f["amax"].long(), f["idx"].long()
    assert (amax < V.S).all()
    # the reference's value at the kernel's sample is within twice the bound of the ball's maximum
    at = torch.relu(r["z2"]).gather(3, amax[..., None])[..., 0]
    assert (r["out"] - at <= 2 * r["E2"].max(-1).values).all()
    # equal columns are bit-equal: of the slots that hold the winning point, the lowest
    first = V.first_slot(idx)[:, None].expand(-1, V.C, -1, -1).gather(3, amax[..., None])[..., 0]
    assert torch.equal(first, amax)
    assert (amax[f["out"] == 0] == 0).all()                           # all tie at 0: the lowest sample wins
    differ = amax != r["amax"]
    print(f"{name} arg-max: {int(differ.sum())} of {differ.numel()} decisions differ from the reference's")
    assert not (differ & ~(r["undecided"]["arg"] | r["undecided"]["out"])).any()


@pytest.mark.parametrize("name", V.NAMES)
def test_inference_mode_and_second_run(dev, name):
    run = _run(dev, name)
    assert sorted(run["inf"]) == ["idx", "out"]
    for k in ("idx", "out"):
        assert torch.equal(run["inf"][k], run["fwd"][k]), k
    for k in run["fwd"]:
        assert torch.equal(run["fwd2"][k], run["fwd"][k]), k
    for k in run["bwd"]:
        assert torch.equal(run["bwd2"][k], run["bwd"][k]), k


# ---- backward, on the kernel's own out, amax, H ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", V.NAMES)
def test_backward_stages(dev, name):
    sc, run = V.scene(name), _run(dev, name)
    f, g = run["fwd"], run["bwd"]
    assert torch.equal(g["dZ2"], V.dz2_stage(sc["dout"], f["amax"], f["out"] > 0))
    active = f["H"] > 0
    dZ1, E = V.dz1_stage(sc["w2"], g["dZ2"], active)
    _report(name, "dZ1", g["dZ1"], dZ1, E)
    assert (g["dZ1"][~active] == 0).all()
    dG, E = V.dg_stage(sc["w1"], g["dZ1"])
    _report(name, "dG", g["dG"], dG, E)


# ---- p2r_gemm_nt_256 ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nb,L,split", V.GEMM_CASES)
def test_gemm_nt_partials(dev, nb, L, split):
    from pose2room_amd import _lib
    A, B = V.gemm_operands(nb, L)
    Ad, Bd = A.to(dev), B.to(dev)
    part, again = (_full((split, V.C, V.C), dev) for _ in range(2))
    _lib.launch("p2r_gemm_nt_256", dev, nb, L, split, Ad, Bd, part)
    _lib.launch("p2r_gemm_nt_256", dev, nb, L, split, Ad, Bd, again)
    assert torch.equal(part, again)
    ranges = V.gemm_ranges(nb, L, split)
    live = sum(hi > lo for lo, hi in ranges)
    assert all(hi > lo for lo, hi in ranges[:live])
    assert (part[live:] == 0).all()                                     # an empty range: exact zeros
    got = part[:live].cpu()
    for p, (lo, hi) in enumerate(ranges[:live]):
        want, E = V.gemm_reference(A, B, lo, hi)
        _report(f"gemm_nt {nb},{L},{split}", f"part {p} [{lo},{hi})", got[p], want, E)
    want, E = V.gemm_reference(A, B, 0, nb * L)
    _report(f"gemm_nt {nb},{L},{split}", "sum of parts", got.double().sum(0), want,
            E * (V.gamma(nb * L + split) / V.gamma(nb * L + 1)))


# ---- refused and empty calls: nothing is written -------------------------------------------------------------------------------
def _untouched(o):
    for k, t in o.items():
        fill = {torch.float32: POISON, torch.int32: POISON_I, torch.uint8: POISON_B}[t.dtype]
        assert (t == fill).all(), k


@pytest.mark.parametrize("over", [{"nsample": 8}, {"C0": 128}, {"H": None}, {"n": 0}], ids=["nsample8", "C0_128", "G_without_H", "n0"])
def test_forward_refusals(dev, over):
    sc = V.scene("walk")
    d = _device_inputs(dev, sc)
    o = _forward_buffers(dev, 2, 9)
    with pytest.raises(RuntimeError, match="p2r_sa_votes_forward " + EINVAL):
        _forward(dev, d, sc["radius"], o=o, **over)
    torch.cuda.synchronize()
    _untouched(o)


@pytest.mark.parametrize("over", [{"b": 0}, {"m": 0}], ids=["b0", "m0"])
def test_empty_calls_write_nothing(dev, over):
    sc = V.scene("walk")
    d = _device_inputs(dev, sc)
    o = _forward_buffers(dev, 2, 9)
    _forward(dev, d, sc["radius"], o=o, **over)
    oi = _forward_buffers(dev, 2, 9, train=False)
    _forward(dev, d, sc["radius"], train=False, o=oi, **over)
    f = {k: v.to(dev) for k, v in _run(dev, "walk")["fwd"].items()}
    g = {k: _full((2, V.C, 9, V.S), dev) for k in ("dZ2", "dZ1", "dG")}
    _backward(dev, d, f, o=g, **over)
    torch.cuda.synchronize()
    _untouched(o), _untouched(oi), _untouched(g)


def test_gemm_nt_refusals_and_empty(dev):
    from pose2room_amd import _lib
    A, B = (t.to(dev) for t in V.gemm_operands(1, 16))
    part = _full((1, V.C, V.C), dev)
    for split in (0, 1025):
        with pytest.raises(RuntimeError, match="p2r_gemm_nt_256 " + EINVAL):
            _lib.launch("p2r_gemm_nt_256", dev, 1, 16, split, A, B, part)
    _lib.launch("p2r_gemm_nt_256", dev, 0, 16, 1, A, B, part)           # nb = 0: OK, nothing to do
    torch.cuda.synchronize()
    _untouched({"partial": part})


# ---- end to end through fused.sa_votes / _SAVotes --------------------------------------------------------------------------------
E2E = ("walk", "partial", "m3b")
PARAMS = ("features", "w1", "b1", "w2", "b2")
REF_OF = {"features": "dfeat", "w1": "dw1", "b1": "db1", "w2": "dw2", "b2": "db2"}


def _fused(dev, name, trainable=PARAMS, summed=False):
    """fused.sa_votes on the scene with `trainable` requiring gradients; backward of sum(out * dout), or of out.sum(), whose
    gradient reaches the op expanded (stride 0) -> (out, idx, {name: grad or None}) on the CPU"""
    from pose2room_amd.pointnet2_ops import fused
    sc = V.scene(name)
    c1, c2 = (torch.nn.Conv2d(V.C, V.C, 1) for _ in range(2))
    with torch.no_grad():
        for conv, w, b in ((c1, "w1", "b1"), (c2, "w2", "b2")):
            conv.weight.copy_(sc[w].view(V.C, V.C, 1, 1))
            conv.bias.copy_(sc[b])
    mod = torch.nn.Sequential(c1, torch.nn.ReLU(), c2, torch.nn.ReLU()).to(dev)
    assert fused.supports(mod, V.S)
    leaves = {"features": sc["features"].clone().to(dev), "w1": c1.weight, "b1": c1.bias, "w2": c2.weight, "b2": c2.bias}
    for k, t in leaves.items():
        t.requires_grad_(k in trainable)
    out, idx = fused.sa_votes(sc["xyz"].to(dev), sc["new_xyz"].to(dev), leaves["features"], sc["radius"], V.S, mod,
                              return_idx=True)
    if summed:
        out.sum().backward()
    else:
        out.backward(sc["dout"].to(dev))
    grads = {k: None if t.grad is None else t.grad.detach().reshape(sc[k].shape).cpu() for k, t in leaves.items()}
    return out.detach().cpu(), idx.cpu(), grads


def _all_gradients(dev, name):
    if name not in _E2E:
        _E2E[name] = _fused(dev, name)
    return _E2E[name]


def _check_gradients(dev, name, grads, sc):
    f = _run(dev, name)["fwd"]
    fwd = V.forward(sc, f["idx"], active=f["H"] > 0)
    want = V.backward(sc, fwd, amax=f["amax"], positive=f["out"] > 0, split=64)
    for k in PARAMS:
        value, bound = want[REF_OF[k]]
        assert grads[k].dtype == torch.float32 and grads[k].shape == value.shape, k
        _report(name, "end to end " + REF_OF[k], grads[k], value, bound)


@pytest.mark.parametrize("name", E2E)
def test_end_to_end(dev, name):
    out, idx, grads = _all_gradients(dev, name)
    f = _run(dev, name)["fwd"]
    assert torch.equal(out, f["out"]) and torch.equal(idx, f["idx"])
    _check_gradients(dev, name, grads, V.scene(name))


def test_end_to_end_expanded_cotangent(dev):
    """d(out.sum()) arrives as an expanded scalar: the op must make it contiguous before the kernel reads it"""
    _, _, grads = _fused(dev, "walk", summed=True)
    sc = dict(V.scene("walk"))
    sc["dout"] = torch.ones_like(sc["dout"])
    _check_gradients(dev, "walk", grads, sc)


@pytest.mark.parametrize("trainable", [("features",), ("w1", "w2"), ("b1", "b2"), ("w1", "b2")],
                         ids=["features", "weights", "biases", "w1_b2"])
@pytest.mark.parametrize("name", E2E)
def test_requires_grad_subsets(dev, name, trainable):
    """what is asked for is bit-equal to the all-gradients run, the rest is None"""
    out_all, _, want = _all_gradients(dev, name)
    out, _, got = _fused(dev, name, trainable)
    assert torch.equal(out, out_all)
    for k in PARAMS:
        if k in trainable:
            assert got[k] is not None and torch.equal(got[k], want[k]), k
        else:
            assert got[k] is None, k
