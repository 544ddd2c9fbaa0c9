"""GPU: the sample build on the device (csrc/sample_build.hip through net_utils/sample_build.py and
DeviceSampleStore.from_recordings) against what the reference's own stage 3 made of the G16 recordings, against the NumPy
mirror on seeded edge cases, against `floor_heights`, and against the host-built store; and the memory contract of the
three entry points (tests/memguard.py).  Every comparison is exact.  G16 and seeded data only."""
import ctypes
import functools
import warnings

import numpy as np
import pytest
import torch

from pose2room_amd.net_utils import sample_build as sb
from pose2room_amd.net_utils import vote_labels as vl
from pose2room_amd.p2rnet import device_loader as dv
from tests import memguard
from tests import sample_build_cases as cases

pytestmark = pytest.mark.gpu

KEPT = [0, 1, 2, 6]                     # the G16 recordings that give samples


def _scan_inputs(recs, dev, contact):
    rec = sb.Recordings([r['joints'] for r in recs], dev)
    K = max(len(r['object_nodes']) for r in recs)
    objects = vl.ContactBoxes([vl.contact_tables(sb.enlarged_nodes(r['object_nodes'], contact), K, 0.0) for r in recs],
                              dev)
    room = torch.from_numpy(np.stack([sb.room_row(r['room_bbox']) for r in recs])).to(dev)
    return rec, room, objects


def _scan(recs, dev, origin=0, contact=1.0):
    first, status = sb.recording_scan(*_scan_inputs(recs, dev, contact), origin)
    return first.cpu().tolist(), status.cpu().tolist()


# ---- 1. the scan -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("J,origin", [(53, 0), (2, 1)])
def test_scan_edges_equal_mirror(dev, J, origin):
    mk = functools.partial(cases.seeded_recording, J=J, origin=origin)
    recs = [mk(1, 0), mk(7, 6), mk(64, None), mk(65, 64), mk(300, 257), mk(300, 0, seed=1), mk(7, None, seed=2),
            mk(64, 5, near=False), dict(mk(7, 2, seed=3), object_nodes=[]), mk(9, 4, seed=4), mk(300, 299, seed=5)]
    recs[9]['joints'][1, 1 - origin if J == 2 else 17, 2] = np.nan      # a non-origin joint of a trimmed frame
    want = [sb.scan_reference(r['joints'], r['room_bbox'], r['object_nodes'], 1.0, origin) for r in recs]
    assert want == [(0, 0), (6, 0), (-1, 3), (64, 0), (257, 0), (0, 0), (-1, 3), (5, 2), (2, 2), (4, 4), (299, 0)]
    first, status = _scan(recs, dev, origin)
    assert list(zip(first, status)) == want
    with pytest.raises(ValueError, match="seeded_9_4_4.*not finite"):
        sb.build_samples(recs, device=dev, origin_joint=origin)


def test_scan_beyond_one_trip_of_the_workgroup(dev):
    """Recordings longer than the 1024 lanes of a workgroup: a lane keeps its first frame in the room across its trips
    and overwrites its last frame near an object; and frames near an object that all lie before `first` do not count."""
    mk = cases.seeded_recording
    recs = [mk(2100, 1500), mk(2100, 1023, seed=1), mk(2100, 1024, seed=2), mk(2100, 1500, seed=3, near='before'),
            mk(1100, 40, seed=4, near='before'), mk(2049, 2048, seed=5), mk(2100, None, seed=6)]
    want = [sb.scan_reference(r['joints'], r['room_bbox'], r['object_nodes'], 1.0, 0) for r in recs]
    assert want == [(1500, 0), (1023, 0), (1024, 0), (1500, 2), (40, 2), (2048, 0), (-1, 3)]
    first, status = _scan(recs, dev)
    assert list(zip(first, status)) == want


def test_scan_equals_g16(dev):
    g16, contact, origin = cases.g16()
    first, status = _scan([c.recording for c in g16], dev, origin, contact)
    assert first == [c.first for c in g16]
    assert [s & 4 for s in status] == [0] * 7
    reason = lambda s: sb.NEVER_IN_ROOM if s & 1 else sb.NEAR_NO_OBJECT if s & 2 else None       # noqa: E731
    assert [reason(s) for s in status] == [c.reason for c in g16]


# ---- 2. the build ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variants", [(0,), (5,), tuple(range(8))])
@pytest.mark.parametrize("votes", [True, False])
def test_build_equals_g16(dev, variants, votes):
    g16, contact, origin = cases.g16()
    built = sb.build_samples([c.recording for c in g16], variants, contact_dist=contact, device=dev, votes=votes)
    assert built.kept == KEPT and built.first == [g16[i].first for i in KEPT]
    assert built.rejected == [(c.recording['name'], c.reason) for c in g16 if c.reason is not None]
    want = [(g16[i], a) for i in KEPT for a in variants]
    assert built.names == [c.recording['name'] + '_%d' % a for c, a in want]
    lengths = [c.variants[a][0].shape[0] for c, a in want]
    assert sorted(set(lengths)) == [1, 5, 37]
    assert built.n_frames.cpu().tolist() == lengths
    assert built.frame_offset.cpu().tolist() == [int(x) for x in np.cumsum([0] + lengths[:-1])]
    assert (built.votes is None) == (not votes)
    joints = built.joints.cpu().numpy()
    got_votes = built.votes.cpu().numpy() if votes else None
    assert joints.shape == (sum(lengths), 53, 3) and joints.shape[0] * 53 % 256 != 0
    off = 0
    for (c, a), n, nodes in zip(want, lengths, built.instances):
        rj, rv, rn = c.variants[a]                                  # the reference's own output
        assert np.array_equal(joints[off:off + n], rj), (c.recording['name'], a)
        if votes:
            assert np.array_equal(got_votes[off:off + n], rv), (c.recording['name'], a)
        for x, y in zip(nodes, rn):
            assert np.array_equal(x['centroid'], y['centroid']) and np.array_equal(x['R_mat'], y['R_mat'])
        off += n
    fh = np.array([dv.floor_heights(c.variants[a][0]) for c, a in want])
    assert np.array_equal(built.floors.cpu().numpy(), fh)


# ---- 3. the floors ---------------------------------------------------------------------------------------------------------
def _floors(dev, columns, J):
    """columns: one (frames * J,) float32 height array per sample -> (device floors (N, 2), floor_heights (N, 2))"""
    rng = np.random.default_rng(5)
    joints, t0 = [], []
    for y in columns:
        j = rng.normal(0.0, 1.0, (y.size // J, J, 3)).astype(np.float32)
        j[..., 1] = y.reshape(-1, J)
        joints.append(j)
        t0.append(j.shape[0])
    off = np.zeros(len(t0), np.int64)
    off[1:] = np.cumsum(t0)[:-1]
    got = sb.floor_percentile(torch.from_numpy(np.concatenate(joints)).to(dev), torch.from_numpy(off).to(dev),
                              torch.tensor(t0, dtype=torch.int32, device=dev), max_frames=max(t0))
    return got.cpu().numpy(), np.array([dv.floor_heights(j) for j in joints])


def test_floors_equal_numpy(dev):
    rng = np.random.default_rng(6)
    draw = lambda n: rng.normal(0.9, 0.5, n).astype(np.float32)                                   # noqa: E731
    f = np.float32
    # J = 1: n = 1, 2, 52 (the first n on the g >= 0.5 branch), an all-equal column, two-valued columns (n = 300, k = 2)
    # whose tie ends below, at and above rank k, and both zeros among both signs with the ranks inside the zeros
    two = lambda lo: np.concatenate([np.full(lo, 0.25, f), np.full(300 - lo, 0.75, f)])[rng.permutation(300)]  # noqa: E731
    zeros = np.concatenate([f([-1.5, -0.25]), np.full(3, -0.0, f), np.full(3, 0.0, f), draw(392) ** 2 + f(0.01)])
    edge = np.concatenate([f([-1.5, -0.25, -0.125, -0.0625]), np.full(2, -0.0, f), np.full(2, 0.0, f),
                           draw(392) ** 2 + f(0.01)])       # y[k] is negative, y[k + 1] a zero
    cols = [draw(1), draw(2), draw(52), np.full(300, 0.75, f), two(2), two(3), two(4), zeros[rng.permutation(400)],
            edge[rng.permutation(400)], -draw(777) ** 2]
    got, want = _floors(dev, cols, 1)
    assert (got == want).all(), (got, want)
    # J = 53: n = 53, 106 (the first n with k = 1), 37 * 53, 1200 * 53
    got, want = _floors(dev, [draw(53), draw(106), draw(37 * 53), draw(1200 * 53)], 53)
    assert (got == want).all(), (got, want)
    # n = 10001 = 137 * 73 is the smallest n at which the float32 form asks for another rank (k = 99) than the float64
    # form (k = 98); found by a search over all n <= 65535 * 53, which has 2308 such n
    n = 137 * 73
    assert int(np.floor((n - 1) * (0.99 / 100.0))) == 98 and int(np.floor(f(n - 1) * (f(0.99) / f(100)))) == 99
    got, want = _floors(dev, [draw(n), draw(73)], 73)
    assert (got == want).all(), (got, want)
    # a NaN height gives NaN, as np.percentile does
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        got, want = _floors(dev, [np.concatenate([draw(99), f([np.nan])]), draw(100)], 1)
    assert np.isnan(got[0]).all() and np.isnan(want[0]).all() and (got[1] == want[1]).all()


# ---- 4. the store ----------------------------------------------------------------------------------------------------------
TABLES = ('box_center', 'box_heading', 'box_size', 'box_mask', 'box_cls')


@pytest.fixture(scope="module")
def host_samples():
    g16, contact, origin = cases.g16()
    return [s for c in g16 if c.reason is None for s in sb.build_reference(c.recording, range(8), contact).samples]


@pytest.mark.parametrize("mode", ['store', 'derive'])
def test_store_from_recordings_equals_host_store(dev, host_samples, mode, monkeypatch):
    g16, contact, origin = cases.g16()
    want = dv.DeviceSampleStore(host_samples, device=dev, votes=mode)
    monkeypatch.setattr(dv, 'floor_heights', None)                  # from_recordings has no use for it
    got = dv.DeviceSampleStore.from_recordings([c.recording for c in g16], votes=mode, device=dev)
    assert got.names == want.names and len(got) == 32 and got.kept == KEPT
    assert got.rejected == [(c.recording['name'], c.reason) for c in g16 if c.reason is not None]
    for k in ('joints', 'frame_offset', 'n_frames', 'floor_height') + TABLES:
        a, b = getattr(got, k), getattr(want, k)
        assert a.dtype == b.dtype and torch.equal(a, b), k
    assert np.array_equal(got.T0, want.T0) and got.nbytes == want.nbytes and got.lean == want.lean
    if mode == 'derive':
        assert got.votes is None and want.votes is None
        for k in ('centroid', 'R_mat', 'half', 'n_boxes'):
            assert torch.equal(getattr(got.contact, k), getattr(want.contact, k)), k
    else:
        assert got.contact is None and torch.equal(got.votes, want.votes)
    ids = [0, 9, 17, 31, 12]
    draws = [(1, dv.ANGLES[1], 0.3), (0, dv.ANGLES[0], -0.7), (1, dv.ANGLES[3], 0.0), (0, dv.ANGLES[2], 0.55),
             (1, dv.ANGLES[0], -0.1)]
    for augment in (True, False):
        a = got.assemble(ids, 16, augment, draws if augment else None, use_height=True)
        b = want.assemble(ids, 16, augment, draws if augment else None, use_height=True)
        assert a.keys() == b.keys() and a['sample_idx'] == b['sample_idx']
        for k in a:
            if k != 'sample_idx':
                assert torch.equal(a[k], b[k]), (augment, k)


def test_store_with_every_recording_rejected(dev):
    g16, contact, origin = cases.g16()
    with pytest.raises(ValueError, match="no samples.*never in the room"):
        dv.DeviceSampleStore.from_recordings([g16[3].recording, g16[4].recording], device=dev)
    built = sb.build_samples([g16[5].recording], device=dev)
    assert built.names == [] and built.joints.shape == (0, 53, 3) and built.rejected == [('no_objects', sb.NEAR_NO_OBJECT)]


# ---- 5. the memory contract ------------------------------------------------------------------------------------------------
def _guarded_out(shape, dtype, dev, offset_bytes):
    """an output poison-filled inside poisoned guard bands, its start not 16-byte aligned"""
    buf, view = memguard.guarded(shape, dtype, dev, fill='poison', halo='poison', offset_bytes=offset_bytes)
    assert view.data_ptr() % 16 == offset_bytes
    return buf, view


def _check_outputs(outs):
    torch.cuda.synchronize()
    for name, (buf, view) in outs.items():
        assert int(memguard.halo_damage(buf, view, 'poison')) == 0, f"{name}: written outside"
        assert int(memguard.poison_count(view)) == 0, f"{name}: an element never written"


def _check_inputs(inputs, before, call):
    for k, v in inputs.items():
        assert memguard.same_bits(v, before[k]), f"{call} wrote to its input {k}"


def test_memory_contract_of_the_three_entry_points(dev):
    g16, contact, origin = cases.g16()
    recs = [c.recording for c in g16]
    rec, room, objects = _scan_inputs(recs, dev, contact)
    inputs = {'rec.joints': rec.joints, 'rec.frame_offset': rec.frame_offset, 'rec.n_frames': rec.n_frames,
              'room': room, 'objects.centroid': objects.centroid, 'objects.R_mat': objects.R_mat,
              'objects.half': objects.half, 'objects.n_boxes': objects.n_boxes}
    before = {k: v.clone() for k, v in inputs.items()}              # taken before the first launch
    # scan
    outs = {'first': _guarded_out((rec.R,), torch.int32, dev, 4), 'status': _guarded_out((rec.R,), torch.int32, dev, 4)}
    sb._launch("p2r_recording_scan", dev, ctypes.byref(rec.c), origin, room, ctypes.byref(objects.c), outs['first'][1],
               outs['status'][1])
    _check_outputs(outs)
    _check_inputs(inputs, before, "p2r_recording_scan")
    first = outs['first'][1].cpu().tolist()
    assert first == [c.first for c in g16]
    # build: all eight variants of the kept recordings, with and without votes
    plan_rows = [(i, first[i], a, recs[i]['joints'].shape[0] - first[i]) for i in KEPT for a in range(8)]
    S, F = len(plan_rows), sum(p[3] for p in plan_rows)
    col = lambda k: torch.tensor([p[k] for p in plan_rows], dtype=torch.int32, device=dev)        # noqa: E731
    out_offset = torch.tensor(np.cumsum([0] + [p[3] for p in plan_rows[:-1]]), dtype=torch.int64, device=dev)
    shift = torch.from_numpy(np.stack([sb.floor_shift(recs[p[0]]['room_bbox']) for p in plan_rows])).to(dev)
    nodes = [sb.variant_nodes(recs[p[0]]['object_nodes'], sb.floor_shift(recs[p[0]]['room_bbox']), p[2])
             for p in plan_rows]
    boxes = vl.ContactBoxes([vl.contact_tables(n, 10, contact) for n in nodes], dev)
    cols = [col(0), col(1), col(2)]
    build_inputs = {'plan.recording': cols[0], 'plan.first': cols[1], 'plan.variant': cols[2],
                    'plan.out_offset': out_offset, 'plan.shift': shift, 'boxes.centroid': boxes.centroid,
                    'boxes.R_mat': boxes.R_mat, 'boxes.half': boxes.half, 'boxes.n_boxes': boxes.n_boxes}
    before.update({k: v.clone() for k, v in build_inputs.items()})
    inputs.update(build_inputs)
    plan = sb._Plan(recording=cols[0].data_ptr(), first=cols[1].data_ptr(), variant=cols[2].data_ptr(),
                    out_offset=out_offset.data_ptr(), shift=shift.data_ptr(), n_frames_out=F, S=S)
    results = []
    for with_votes in (True, False):
        outs = {'joints': _guarded_out((F, 53, 3), torch.float32, dev, 4)}
        if with_votes:
            outs['votes'] = _guarded_out((F, 53, 10), torch.float32, dev, 4)
        sb._launch("p2r_build_samples", dev, ctypes.byref(rec.c), ctypes.byref(plan),
                   ctypes.byref(boxes.c) if with_votes else None, outs['joints'][1],
                   outs['votes'][1] if with_votes else None)
        _check_outputs(outs)
        _check_inputs(inputs, before, "p2r_build_samples")
        results.append(outs['joints'][1].clone())
    assert torch.equal(results[0], results[1])
    want = np.concatenate([g16[p[0]].variants[p[2]][0] for p in plan_rows])
    assert np.array_equal(results[0].cpu().numpy(), want)
    # floors of the samples just built
    joints = results[0]
    n_frames = torch.tensor([p[3] for p in plan_rows], dtype=torch.int32, device=dev)
    before.update({'joints': joints.clone(), 'n_frames': n_frames.clone()})
    inputs.update({'joints': joints, 'n_frames': n_frames})
    outs = {'floors': _guarded_out((S, 2), torch.float64, dev, 8)}
    sb._launch("p2r_floor_percentile", dev, joints, out_offset, n_frames, S, 53, 37, F, outs['floors'][1])
    _check_outputs(outs)
    assert np.array_equal(outs['floors'][1].cpu().numpy(),
                          np.array([dv.floor_heights(g16[p[0]].variants[p[2]][0]) for p in plan_rows]))
    _check_inputs(inputs, before, "p2r_floor_percentile")
