"""GPU: the recording repair on the device (csrc/recording_repair.hip: p2r_joint_valid_bits, p2r_gap_fill,
p2r_smooth_frames; net_utils/recording_repair.py; build_samples(repair=...); repair_batch) against the definition
`repair_reference` -- on np.interp's own outputs (G19), over the sweep of tests/recording_repair_cases.py, under the
memory contract of tests/memguard.py, in front of the sample build and in front of the synthetic model.

Everything is compared for equality, bit for bit: the kernels evaluate the definition's expressions in its order with
contraction off, a measured item is copied, and the NaN the fill writes is one fixed pattern.  Only where the smoothing
meets values that are not finite is the comparison by `isnan` mask: the payload of a computed NaN is not part of the
contract."""
import ctypes

import numpy as np
import pytest
import torch

from pose2room_amd.net_utils import recording_repair as rr
from pose2room_amd.net_utils import sample_build as sb
from pose2room_amd.p2rnet import device_loader as dv
from tests import memguard
from tests import recording_repair_cases as rc
from tests.memguard import run_contract

pytestmark = pytest.mark.gpu

EINVAL = -22
SWEEP = rc.sweep()


def _np(t):
    return t.cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _device(joints, spec, dev):
    """-> (out, how, stats, bits) of the entry points as host arrays, and the Recordings"""
    rec = sb.Recordings(joints, dev)
    bits = rr.valid_bits(rec)
    out, how, stats = rr.gap_fill(rec, bits, spec.max_gap, spec.hold_ends)
    assert out.is_cuda and how.dtype == torch.uint8 and stats.dtype == torch.int32
    return (_np(out), _np(how), _np(stats), _np(bits).view(np.uint64)), rec


def _check(got, want):
    for name, g, w in zip(('out', 'how', 'stats', 'bits'), got, want):
        assert g.shape == w.shape and g.dtype == w.dtype, name
        if name == 'out':
            g, w = _bits(g), _bits(w)
        assert np.array_equal(g, w), (name, int((g != w).sum()), np.argwhere(g != w)[:4].tolist())


# ---- 1. G19 and the sweep against the definition -------------------------------------------------------------------------
def test_g19(dev):
    z = rc.g19()
    spec = rr.RepairSpec(rr.MAX_GAP, True, 0)
    for r in range(int(z['n_recordings'])):
        x = z[f'r{r}_joints']
        (out, how, stats, bits), _ = _device([x], spec, dev)
        assert np.array_equal(_bits(out), _bits(z[f'r{r}_filled']))                 # np.interp, bit for bit
        assert np.array_equal(how == 0, np.isfinite(x).all(-1)) and stats[0, 2] == 0
    # and all four packed into one call
    xs = [z[f'r{r}_joints'][:, :1] for r in range(int(z['n_recordings']))]
    (out, _, _, _), _ = _device(xs, spec, dev)
    assert np.array_equal(_bits(out), _bits(np.concatenate([z[f'r{r}_filled'][:, :1] for r in range(len(xs))])))


@pytest.mark.parametrize("i", range(len(SWEEP)), ids=[c.name for c in SWEEP])
def test_sweep(dev, i):
    c = SWEEP[i]
    got, _ = _device(c.joints, c.spec, dev)
    _check(got, rc.reference(c.name))


@pytest.mark.parametrize("h", [1, 3, 8])
def test_smoothing_equals_mirror(dev, h):
    c = rc.by_name('F129-65-1_J53_gap63_hold1')
    want_fill = rc.reference(c.name)[0]
    fixed, how, stats = rr.repair_packed(sb.Recordings(c.joints, dev), c.spec._replace(smooth=h))
    assert isinstance(fixed, sb.Recordings) and np.array_equal(_np(how), rc.reference(c.name)[1])
    parts = np.split(want_fill, np.cumsum([len(x) for x in c.joints])[:-1])
    want = np.concatenate([rr.smooth_reference(p, h) for p in parts])
    got = _np(fixed.joints)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan)                                       # what is not finite propagates
    assert np.array_equal(_bits(got[~nan]), _bits(want[~nan]))
    # repaired, all-finite data: every bit
    full = [np.where(np.isnan(p), 1.5, p) for p in parts]
    assert nan.any() and all(np.isfinite(p).all() for p in full)
    got = _np(rr.smooth_frames(sb.Recordings(full, dev), h))
    assert np.array_equal(_bits(got), _bits(np.concatenate([rr.smooth_reference(p, h) for p in full])))


def test_smoothing_tiles(dev):
    """more than one tile of 112 frames and of 32 columns, recordings that end inside a tile, J * 3 no multiple of 32"""
    rng = np.random.default_rng(5)
    xs = [rng.uniform(-1e3, 1e3, (F, 23, 3)) for F in (1, 111, 112, 113, 7, 230, 2)]
    for h in (2, 8):
        got = _np(rr.smooth_frames(sb.Recordings(xs, dev), h))
        assert np.array_equal(_bits(got), _bits(np.concatenate([rr.smooth_reference(x, h) for x in xs])))


# ---- 2. properties ---------------------------------------------------------------------------------------------------------
def test_permuting_the_recordings_permutes_the_results(dev):
    c = rc.by_name('F129-65-1_J53_gap63_hold1')
    order = [2, 0, 1]
    a, _ = _device(c.joints, c.spec, dev)
    b, _ = _device([c.joints[k] for k in order], c.spec, dev)
    cut = lambda x, js: np.split(x, np.cumsum([len(j) for j in js])[:-1])            # noqa: E731
    for k in (0, 1):
        pa, pb = cut(a[k], c.joints), cut(b[k], [c.joints[o] for o in order])
        for n, o in enumerate(order):
            assert np.array_equal(_bits(pb[n]) if k == 0 else pb[n], _bits(pa[o]) if k == 0 else pa[o])
    assert np.array_equal(b[2], a[2][order])
    words = [(len(x) + 63) // 64 for x in c.joints]
    wa, wb = np.split(a[3], np.cumsum(words)[:-1]), np.split(b[3], np.cumsum([words[o] for o in order])[:-1])
    assert all(np.array_equal(wb[n], wa[o]) for n, o in enumerate(order))


def test_frames_of_no_recording_get_zeros(dev):
    """a packed axis with more frames than the recordings own, and a recording outside its limits"""
    rng = np.random.default_rng(3)
    J = 5
    x = rng.uniform(-1e3, 1e3, (40, J, 3))
    x[3:6, 1] = np.nan
    packed = torch.from_numpy(x).to(dev)
    offs = torch.tensor([0, 20], dtype=torch.int64, device=dev)
    n = torch.tensor([10, 12], dtype=torch.int32, device=dev)
    rec = sb.Recordings.from_packed(packed, offs, n, [10, 12])
    out, how, stats = rr.gap_fill(rec, rr.valid_bits(rec), 5, True)
    want = rr.repair_reference([x[:10], x[20:32]], rr.RepairSpec(5, True, 0))
    got = _np(out)
    assert np.array_equal(_bits(np.concatenate([got[:10], got[20:32]])), _bits(want[0]))
    assert not got[10:20].any() and not got[32:].any() and not _np(how)[10:20].any() and not _np(how)[32:].any()
    assert np.array_equal(_np(stats), want[2])
    sm = _np(rr.smooth_frames(rec, 2))
    assert not sm[10:20].any() and not sm[32:].any()
    assert np.array_equal(_bits(sm[20:32]), _bits(rr.smooth_reference(x[20:32], 2)))


# ---- 3. the memory contract ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lengths,J", [((65,), 65), ((193, 64, 129), 53)], ids=['F65-J65', 'R3-F193-J53'])
def test_memory_contract(dev, lengths, J):
    """inputs and outputs in poisoned, guard-banded buffers: every output element is overwritten (the words' padding
    bits, `how` and the statistics of a recording without a hole included), no halo is damaged, the inputs are
    bit-identical afterwards, and four runs over different surroundings give identical bits"""
    joints = rc.contract_case(lengths, J)
    spec = rr.RepairSpec(5, True, 2)
    off = np.zeros(len(lengths), np.int64)
    off[1:] = np.cumsum(lengths)[:-1]

    def fn(packed, frame_offset, n_frames):
        rec = sb.Recordings.from_packed(packed, frame_offset, n_frames, lengths)
        bits = rr.valid_bits(rec)
        out, how, stats = rr.gap_fill(rec, bits, spec.max_gap, spec.hold_ends)
        fixed = sb.Recordings.from_packed(out, frame_offset, n_frames, lengths)
        return bits, out, how, stats, rr.smooth_frames(fixed, spec.smooth)

    got = run_contract(fn, dict(packed=torch.from_numpy(np.concatenate(joints)), frame_offset=torch.from_numpy(off),
                                n_frames=torch.from_numpy(np.asarray(lengths, np.int32))), dev)
    want = rr.repair_reference(joints, spec._replace(smooth=0))
    _check((_np(got['out.1']), _np(got['out.2']), _np(got['out.3']), _np(got['out.0']).view(np.uint64)), want)
    smooth = rr.repair_reference(joints, spec)[0]
    nan = np.isnan(smooth)
    assert np.array_equal(np.isnan(_np(got['out.4'])), nan)
    assert np.array_equal(_bits(_np(got['out.4'])[~nan]), _bits(smooth[~nan]))


def test_refused_calls_leave_their_outputs_untouched(dev):
    joints = rc.contract_case((65, 7), 3)
    rec = sb.Recordings(joints, dev)
    word_offset, n_words = rr._words(rec)
    bits_in = rr.valid_bits(rec)
    outs = {k: memguard.guarded(shape, dtype, dev) for k, shape, dtype in (
        ('bits', (n_words, 3), torch.int64), ('out', (72, 3, 3), torch.float64), ('how', (72, 3), torch.uint8),
        ('stats', (2, 4), torch.int32), ('smooth', (72, 3, 3), torch.float64))}
    p = {k: v.data_ptr() for k, (_, v) in outs.items()}
    stream = torch.cuda.current_stream(dev).cuda_stream
    l, r, wo = rr.lib(), ctypes.byref(rec.c), word_offset.data_ptr()
    refused = [
        l.p2r_gap_fill(r, wo, n_words, bits_in.data_ptr(), -1, 1, p['out'], p['how'], p['stats'], stream),
        l.p2r_gap_fill(r, wo, n_words, bits_in.data_ptr(), rr.MAX_GAP + 1, 1, p['out'], p['how'], p['stats'], stream),
        l.p2r_gap_fill(r, wo, n_words, None, 5, 1, p['out'], p['how'], p['stats'], stream),
        l.p2r_gap_fill(r, None, n_words, bits_in.data_ptr(), 5, 1, p['out'], p['how'], p['stats'], stream),
        l.p2r_gap_fill(None, wo, n_words, bits_in.data_ptr(), 5, 1, p['out'], p['how'], p['stats'], stream),
        l.p2r_gap_fill(r, wo, n_words, bits_in.data_ptr(), 5, 1, rec.joints.data_ptr(), p['how'], p['stats'], stream),
        l.p2r_smooth_frames(r, 0, p['smooth'], stream),
        l.p2r_smooth_frames(r, rr.MAX_HALF + 1, p['smooth'], stream),
        l.p2r_smooth_frames(None, 2, p['smooth'], stream),
        l.p2r_joint_valid_bits(r, None, n_words, p['bits'], stream),
        l.p2r_joint_valid_bits(None, wo, n_words, p['bits'], stream),
        l.p2r_joint_valid_bits(r, wo, 0, p['bits'], stream),
    ]
    assert refused == [EINVAL] * 12
    torch.cuda.synchronize(dev)
    for name, (buf, view) in outs.items():
        assert int(memguard.poison_count(view)) == view.numel(), name
        assert int(memguard.halo_damage(buf, view, 'poison')) == 0, name
    with pytest.raises(ValueError, match="max_gap"):
        rr.gap_fill(rec, bits_in, rr.MAX_GAP + 1, True)
    with pytest.raises(ValueError, match="half_width"):
        rr.smooth_frames(rec, 9)
    with pytest.raises(RuntimeError, match="bits"):
        rr.gap_fill(rec, bits_in.cpu(), 5, True)


# ---- 4. repair_packed: library calls and synchronisation --------------------------------------------------------------------
class _Counted(object):
    """an entry point of the library that counts its calls"""

    def __init__(self, fn, calls, name):
        self.fn, self.calls, self.name, self.argtypes = fn, calls, name, fn.argtypes

    def __call__(self, *args):
        self.calls.append(self.name)
        return self.fn(*args)


@pytest.mark.parametrize("smooth", [0, 3])
def test_repair_packed_is_two_or_three_calls_without_a_synchronisation(dev, monkeypatch, smooth):
    c = rc.by_name('F129-65-1_J53_gap63_hold1')
    spec = c.spec._replace(smooth=smooth)
    rec = sb.Recordings(c.joints, dev)
    rr.repair_packed(rec, spec)                                                     # library loaded, allocator warm
    torch.cuda.synchronize(dev)
    calls = []
    for name in ('p2r_joint_valid_bits', 'p2r_gap_fill', 'p2r_smooth_frames'):
        monkeypatch.setattr(rr.lib(), name, _Counted(getattr(rr.lib(), name), calls, name), raising=True)
    torch.cuda.set_sync_debug_mode("error")
    try:
        fixed, how, stats = rr.repair_packed(rec, spec)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert calls == ['p2r_joint_valid_bits', 'p2r_gap_fill'] + ['p2r_smooth_frames'] * (smooth > 0)
    assert fixed.joints.is_cuda and how.is_cuda and stats.is_cuda and fixed.joints.data_ptr() != rec.joints.data_ptr()
    assert fixed.frame_offset is rec.frame_offset and fixed.R == rec.R and fixed.c.max_frames == rec.c.max_frames
    want = rr.repair_reference(c.joints, spec)
    assert np.array_equal(_np(how), want[1]) and np.array_equal(_np(stats), want[2])
    nan = np.isnan(want[0])
    assert np.array_equal(np.isnan(_np(fixed.joints)), nan)
    assert np.array_equal(_bits(_np(fixed.joints)[~nan]), _bits(want[0][~nan]))


# ---- 5. in front of the sample build -----------------------------------------------------------------------------------------
def _same_store(a, b):
    for f in ('joints', 'votes', 'frame_offset', 'n_frames', 'floors'):
        x, y = getattr(a, f), getattr(b, f)
        assert x.dtype == y.dtype and torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x,
                                                  y.view(torch.int32) if y.dtype == torch.float32 else y), f
    assert a.names == b.names and a.kept == b.kept and a.first == b.first and a.rejected == b.rejected


@pytest.mark.parametrize("smooth", [0, 2])
def test_build_samples_with_repair_equals_build_of_the_mirrors_recordings(dev, smooth):
    recs = rc.scene_recordings([None, 'short', 'short'])
    spec = rr.RepairSpec(30, True, smooth)
    with pytest.raises(ValueError, match="holes_1_short has a coordinate that is not finite"):
        sb.build_samples(recs, device=dev)                                           # as before without the argument
    got = sb.build_samples(recs, (0, 5), device=dev, repair=spec)
    fixed, how, stats, _ = rr.repair_reference([r['joints'] for r in recs], spec)
    parts = np.split(fixed, np.cumsum([len(r['joints']) for r in recs])[:-1])
    want = sb.build_samples([dict(r, joints=p) for r, p in zip(recs, parts)], (0, 5), device=dev)
    assert type(want) is sb.BuiltSamples and isinstance(got, rr.RepairedSamples) and isinstance(got, sb.BuiltSamples)
    assert len(got) == len(want) == 11 and got.kept == [0, 1, 2] and got.rejected == []
    _same_store(got, want)
    assert got.repair.dtype == np.int32 and np.array_equal(got.repair, stats)
    assert stats[0].tolist() == [0, 0, 0, 0] and stats[1, 0] > 20 and stats[1, 2] == 0 and (how == 2).any()
    store = dv.DeviceSampleStore.from_recordings(recs, (0, 5), device=dev, repair=spec)
    assert torch.equal(store.joints, want.joints) and np.array_equal(store.repair, stats)
    assert dv.DeviceSampleStore.from_recordings([recs[0]], (0,), device=dev).repair is None


def test_skip_rejects_exactly_the_recordings_with_a_gap_too_long(dev):
    recs = rc.scene_recordings(['short', 'long', None, 'long'], seed=10)
    spec = rr.RepairSpec(5, True, 0)
    with pytest.raises(ValueError, match=r"holes_1_long has a coordinate that is not finite \(and 1 more"):
        sb.build_samples(recs, (0,), device=dev, repair=spec)
    with pytest.raises(ValueError, match="holes_0_short"):
        sb.build_samples(recs, (0,), device=dev, repair=None, on_unrepairable='skip')
    got = sb.build_samples(recs, (0,), device=dev, repair=spec, on_unrepairable='skip')
    assert got.kept == [0, 2] and got.names == ['holes_0_short_0', 'holes_2_None_0']
    assert got.rejected == [('holes_1_long', sb.UNREPAIRABLE), ('holes_3_long', rr.UNREPAIRABLE)]
    assert got.repair[:, 3].tolist() == [4, 6, 0, 6] and (got.repair[:, 2] > 0).tolist() == [False, True, False, True]
    fixed = rr.repair_reference([recs[0]['joints'], recs[2]['joints']], spec)[0]
    parts = [fixed[:len(recs[0]['joints'])], fixed[len(recs[0]['joints']):]]
    want = sb.build_samples([dict(recs[0], joints=parts[0]), dict(recs[2], joints=parts[1])], (0,), device=dev)
    assert torch.equal(got.joints, want.joints) and torch.equal(got.votes, want.votes)
    assert bool(torch.isfinite(got.joints).all())
    # with max_gap = 12 the long gap is filled as well
    assert sb.build_samples(recs, (0,), device=dev, repair=rr.RepairSpec(12, True, 0)).kept == [0, 1, 2, 3]
    none = sb.build_samples([recs[1]], (0,), device=dev, repair=spec, on_unrepairable='skip')
    assert none.names == [] and none.rejected == [('holes_1_long', sb.UNREPAIRABLE)] and none.repair.shape == (1, 4)


# ---- 6. in front of the model ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_repair_batch_equals_mirror(dev, dtype):
    rng = np.random.default_rng(8)
    x = torch.from_numpy(rng.uniform(-3, 3, (3, 70, 53, 3))).to(dtype)
    x[0, 10:14, 7] = float('nan')
    x[1, :2, 0, 1] = float('inf')
    x[2, 60:, 52] = float('nan')
    x[2, 5:50, 3] = float('nan')
    spec = rr.RepairSpec(30, True, 1)
    before = x.clone()
    joints, how, stats = rr.repair_batch(x.to(dev), spec)
    assert joints.dtype == dtype and joints.shape == x.shape and how.shape == (3, 70, 53) and stats.shape == (3, 4)
    want = rr.repair_reference(list(x.double().numpy()), spec)
    assert np.array_equal(_np(how).reshape(-1, 53), want[1]) and np.array_equal(_np(stats), want[2])
    w = torch.from_numpy(want[0]).to(dtype).reshape(x.shape)
    assert torch.equal(torch.isnan(joints.cpu()), torch.isnan(w)) and torch.equal(joints.cpu().nan_to_num(7.0), w.nan_to_num(7.0))
    assert stats[2].tolist() == [55, 10, 45, 31] and torch.equal(x.isnan(), before.isnan())
    with pytest.raises(RuntimeError, match="GPU"):
        rr.repair_batch(x, spec)
    with pytest.raises(ValueError, match="input_joints"):
        rr.repair_batch(x.to(dev)[0], spec)


@pytest.fixture(scope="module")
def model(dev):
    from pose2room_amd.p2rnet.synthetic import make_batch
    from tests.test_model_cpu import build
    # the fixture of tests/test_scene_gpu.py: the far-box filter is off, as wherever `generate` runs on these weights
    net, cfg = build('test', 64, device=dev, remove_far_box=False)
    return net.to(dev).eval(), cfg, make_batch(2, 64, seed=77, device=dev)


def test_repair_batch_makes_predict_scenes_finite(model):
    net, cfg, data = model
    joints = data['input_joints']
    holes = joints.clone()
    holes[0, 20:23, 0, :3] = float('nan')            # the origin joint: its NaN reaches the votes and the boxes
    holes[1, 0:2, 30, 1] = float('nan')
    with torch.no_grad():
        bad = net.predict_scenes(dict(data, input_joints=holes), contact=False, unique=False)
        assert not bool(torch.isfinite(bad.node_obbs).all())                          # what the user gets today
        fixed, how, stats = rr.repair_batch(holes[..., :3], rr.RepairSpec())
        assert stats.cpu().tolist() == [[3, 3, 0, 3], [2, 2, 0, 2]] and bool(torch.isfinite(fixed).all())
        repaired = holes.clone()
        repaired[..., :3] = fixed
        measured = how == 0
        assert torch.equal(repaired[..., :3][measured], joints[..., :3][measured])
        good = net.predict_scenes(dict(data, input_joints=repaired), contact=False, unique=False)
    assert bool(torch.isfinite(good.node_obbs).all()) and bool(torch.isfinite(good.node_score).all())
    assert int(good.count.sum()) > 0
