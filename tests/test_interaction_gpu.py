"""GPU: the interaction timeline on the device (csrc/interaction.hip: p2r_contact_bits, p2r_contact_intervals,
p2r_frame_labels; net_utils/interaction_device.py; SceneBatch.interactions; P2RNet.predict_interactions) against the
definition `interaction_reference` -- on the inside masks recorded from the reference's hull test (G20), over the designed
cases of tests/interaction_cases.py, under the memory contract of tests/memguard.py, and end to end on the synthetic model.

Everything is compared for equality: all results are integers, the kernels evaluate the definition's expressions in its
order with contraction off, and every case keeps every joint 1e-9 away from every enlarged face or exactly on it (asserted
when the case is built and again in tests/test_interaction_cpu.py)."""
import numpy as np
import pytest
import torch

from pose2room_amd.net_utils import interaction_device as idv
from pose2room_amd.net_utils import scene_device as sd
from tests import interaction_cases as ic
from tests import memguard
from tests.memguard import run_contract

pytestmark = pytest.mark.gpu

EINVAL = -22
SWEEP = ic.sweep()


def _np(t):
    return None if t is None else t.cpu().numpy()


def _scene_batch(c, dev):
    """the node arrays of case c as a SceneBatch on the device"""
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)               # noqa: E731
    N, K = c.node_obbs.shape[:2]
    return sd.SceneBatch(c.H, N // c.H, K, t(c.count), torch.zeros(N, K, dtype=torch.int32, device=dev), t(c.node_obbs),
                         t(c.node_rmat), torch.zeros(N, K, dtype=torch.int64, device=dev),
                         torch.zeros(N, K, dtype=torch.float32, device=dev))


def _batch(c, dev, **kw):
    kw = {**dict(merge_gap=c.merge_gap, min_len=c.min_len, max_intervals=c.M), **kw}
    return _scene_batch(c, dev).interactions(torch.from_numpy(c.joints).to(dev), contact_thresh=c.thresh, **kw)


def _device(c, dev, **kw):
    b = _batch(c, dev, **kw)
    assert all(t is None or t.is_cuda for t in b.tensors())
    return idv.Interaction(*map(_np, b.tensors()))


def _popcount(words):
    return idv.unpack_bits(words, 64 * words.shape[-1]).sum(-1)


# ---- 1. G20 and the designed cases against the definition ---------------------------------------------------------------------
def test_g20(dev):
    z = ic.g20()
    t = lambda k: torch.from_numpy(z[k]).to(dev)                                  # noqa: E731
    bits, njoint, joint_mask, n_raw = idv.contact_bits(t('joints'), t('node_obbs'), t('node_rmat'), t('count'),
                                                       float(z['contact_thresh']))
    for name, got in (('bits', bits), ('njoint', njoint), ('joint_mask', joint_mask)):        # the reference's hull test
        assert np.array_equal(_np(got), z[name]) and _np(got).dtype == z[name].dtype, name
    assert np.array_equal(_np(n_raw), _popcount(z['bits']))


@pytest.mark.parametrize("i", range(len(SWEEP)), ids=[c.name for c in SWEEP])
def test_sweep(dev, i):
    c = SWEEP[i]
    got, want = _device(c, dev), ic.reference(c.name)
    ic.check_interaction(got, want)
    T = c.joints.shape[1]
    assert np.array_equal(got.n_raw, _popcount(got.bits)) and np.array_equal(got.n_frames, _popcount(got.clean))
    # n_labelled is the popcount of the OR over the slots
    union = idv.unpack_bits(got.clean, T).any(1) if got.clean.shape[1] else np.zeros((len(c.count), T), bool)
    assert np.array_equal(got.n_labelled, union.sum(1)) and np.array_equal(got.label >= 0, union)
    plain = _device(c, dev, labels=False)                     # two launches: the same bits and runs, no njoint
    assert plain.njoint is None and plain.label is None and plain.n_active is None and plain.n_labelled is None
    ic.check_interaction(plain, want._replace(njoint=None, label=None, n_active=None, n_labelled=None))


# ---- 2. properties ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ['T-130-2x2', 'T-64', 'patterns-4097'])
def test_no_merging_no_filter_gives_the_bits(dev, name):
    got = _device(ic.by_name(name), dev, merge_gap=0, min_len=1)
    assert np.array_equal(got.clean, got.bits) and got.bits.any() and np.array_equal(got.n_frames, got.n_raw)


def test_copies_of_one_scene_give_equal_timelines(dev):
    one = ic.by_name('patterns-130')
    H = 3
    a, b = _device(one, dev), _batch(ic.copies(one, H), dev)
    got = idv.Interaction(*map(_np, b.tensors()))
    for f in idv.Interaction._fields:
        assert np.array_equal(getattr(got, f), np.concatenate([getattr(a, f)] * H, 0)), f
    assert b.timeline(0, 0) == b.timeline(0, 1) == b.timeline(0, 2) and len(b.timeline(0)) == one.count[0]
    assert np.array_equal(b.labels(0, 0), b.labels(0, 2))


@pytest.mark.parametrize("name", ['T-130-2x2', 'T-64'])
def test_permuting_the_samples_permutes_the_results(dev, name):
    c = ic.by_name(name)
    B = len(c.count) // c.H
    assert B == 2
    swap = lambda a: a.reshape(c.H, B, *a.shape[1:])[:, ::-1].reshape(a.shape).copy()     # noqa: E731
    a = _device(c, dev)
    b = _device(c._replace(count=swap(c.count), node_obbs=swap(c.node_obbs), node_rmat=swap(c.node_rmat),
                           joints=c.joints[::-1].copy()), dev)
    assert not np.array_equal(a.bits, b.bits)
    for f in idv.Interaction._fields:
        assert np.array_equal(getattr(a, f), swap(getattr(b, f))), f


def test_empty_problems(dev):
    z = lambda *shape, dtype: torch.zeros(*shape, dtype=dtype, device=dev)        # noqa: E731
    joints = z(2, 70, 7, 3, dtype=torch.float32)
    for N, K in ((0, 5), (0, 0), (2, 0)):
        count = z(N, dtype=torch.int32)
        bits, njoint, joint_mask, n_raw = idv.contact_bits(joints, z(N, K, 7, dtype=torch.float64),
                                                           z(N, K, 3, 3, dtype=torch.float64), count, 0.1)
        assert bits.shape == (N, K, 2) and njoint.shape == (N, K, 70) and joint_mask.shape == n_raw.shape == (N, K)
        clean, n_intervals, intervals, n_frames, first, last = idv.contact_intervals(bits, count, 70, 1, 2, 4)
        assert clean.shape == (N, K, 2) and intervals.shape == (N, K, 4, 2) and first.shape == (N, K)
        with memguard.poisoned_allocations('cuda'):
            label, n_active, n_labelled = idv.frame_labels(clean, njoint, count)
            torch.cuda.synchronize(dev)
        assert label.shape == n_active.shape == (N, 70) and n_labelled.shape == (N,)
        assert bool((label == -1).all()) and not bool(n_active.any()) and not bool(n_labelled.any())
    # all counts 0: zeros and -1 over buffers that held something else
    with memguard.poisoned_allocations('cuda'):
        count = z(2, dtype=torch.int32)
        bits, njoint, joint_mask, n_raw = idv.contact_bits(joints, torch.ones(2, 5, 7, dtype=torch.float64, device=dev),
                                                           torch.ones(2, 5, 3, 3, dtype=torch.float64, device=dev), count, 9.0)
        clean, n_intervals, intervals, n_frames, first, last = idv.contact_intervals(bits, count, 70)
        torch.cuda.synchronize(dev)
    for t in (bits, njoint, joint_mask, n_raw, clean, n_intervals, n_frames):
        assert not bool(t.any())
    for t in (intervals, first, last):
        assert bool((t == -1).all())


# ---- 3. the memory contract ------------------------------------------------------------------------------------------------
def _all_stages(c):
    def fn(joints, node_obbs, node_rmat, count):
        bits, njoint, joint_mask, n_raw = idv.contact_bits(joints, node_obbs, node_rmat, count, c.thresh)
        runs = idv.contact_intervals(bits, count, c.joints.shape[1], c.merge_gap, c.min_len, c.M)
        return (bits, njoint, joint_mask, n_raw) + tuple(runs) + tuple(idv.frame_labels(runs[0], njoint, count))
    return fn


@pytest.mark.parametrize("name", ['T-65', 'patterns-4097'])
def test_memory_contract(dev, name):
    """inputs and outputs in poisoned, guard-banded buffers: every output element is overwritten (the padding bits, the
    empty slots and the -1 of the unused intervals included), no halo is damaged, the inputs are bit-identical
    afterwards, and four runs over different surroundings give identical bits"""
    c = ic.by_name(name)
    t = torch.from_numpy
    ins = dict(joints=t(c.joints), node_obbs=t(c.node_obbs), node_rmat=t(c.node_rmat), count=t(c.count))
    got = run_contract(_all_stages(c), ins, dev)
    ic.check_interaction(idv.Interaction(*[_np(got[f'out.{i}']) for i in range(13)]), ic.reference(name))


def test_refused_calls_leave_their_outputs_untouched(dev):
    from tests.test_interaction_cpu import BAD_BITS, BAD_INTERVALS, BAD_LABELS
    B, T, J, C, N, K, M = 2, 70, 7, 3, 4, 5, 16               # the shapes the lists of bad arguments are written against
    W = idv.words_of(T)
    joints = torch.zeros(B, T, J, C, device=dev)
    count = torch.full((N,), K, dtype=torch.int32, device=dev)
    obbs = torch.ones(N, K, 7, dtype=torch.float64, device=dev)
    rmat = torch.ones(N, K, 3, 3, dtype=torch.float64, device=dev)
    bits_in = torch.zeros(N, K, W, dtype=torch.int64, device=dev)
    njoint_in = torch.zeros(N, K, T, dtype=torch.uint8, device=dev)
    i32, i64, u8 = torch.int32, torch.int64, torch.uint8
    outs = {k: memguard.guarded(shape, dtype, dev) for k, shape, dtype in (
        ('bits', (N, K, W), i64), ('njoint', (N, K, T), u8), ('joint_mask', (N, K), i64), ('n_raw', (N, K), i32),
        ('clean', (N, K, W), i64), ('n_intervals', (N, K), i32), ('intervals', (N, K, M, 2), i32), ('n_frames', (N, K), i32),
        ('first', (N, K), i32), ('last', (N, K), i32), ('label', (N, T), i32), ('n_active', (N, T), u8),
        ('n_labelled', (N,), i32))}
    p = {k: v.data_ptr() for k, (_, v) in outs.items()}
    stream = torch.cuda.current_stream(dev).cuda_stream
    l = idv.lib()
    good = {
        'p2r_contact_bits': dict(joints=joints.data_ptr(), B=B, T=T, J=J, C=C, N=N, K=K, node_obbs=obbs.data_ptr(),
                                 node_rmat=rmat.data_ptr(), count=count.data_ptr(), contact_thresh=0.1, bits=p['bits'],
                                 njoint=p['njoint'], joint_mask=p['joint_mask'], n_raw=p['n_raw']),
        'p2r_contact_intervals': dict(bits=bits_in.data_ptr(), count=count.data_ptr(), N=N, K=K, T=T, merge_gap=1, min_len=2,
                                      M=M, clean=p['clean'], n_intervals=p['n_intervals'], intervals=p['intervals'],
                                      n_frames=p['n_frames'], first=p['first'], last=p['last']),
        'p2r_frame_labels': dict(clean=bits_in.data_ptr(), njoint=njoint_in.data_ptr(), count=count.data_ptr(), N=N, K=K, T=T,
                                 label=p['label'], n_active=p['n_active'], n_labelled=p['n_labelled']),
    }
    refused = []
    for name, bads in (('p2r_contact_bits', BAD_BITS), ('p2r_contact_intervals', BAD_INTERVALS),
                       ('p2r_frame_labels', BAD_LABELS)):
        for bad in bads:
            refused.append(getattr(l, name)(*{**good[name], **bad}.values(), stream))
    assert refused == [EINVAL] * len(refused) and len(refused) > 50
    torch.cuda.synchronize(dev)
    for name, (buf, view) in outs.items():
        assert int(memguard.poison_count(view)) == view.numel(), name
        assert int(memguard.halo_damage(buf, view, 'poison')) == 0, name


# ---- 4. SceneBatch.interactions: launches and synchronisation -----------------------------------------------------------------
class _Counted(object):
    """an entry point of the library that counts its calls"""

    def __init__(self, fn, calls, name):
        self.fn, self.calls, self.name, self.argtypes = fn, calls, name, fn.argtypes

    def __call__(self, *args):
        self.calls.append(self.name)
        return self.fn(*args)


def test_scene_batch_interactions_is_three_launches_without_a_synchronisation(dev, monkeypatch):
    c = ic.by_name('T-130-2x2')
    scenes, joints = _scene_batch(c, dev), torch.from_numpy(c.joints).to(dev)
    kw = dict(contact_thresh=c.thresh, merge_gap=c.merge_gap, min_len=c.min_len, max_intervals=c.M)
    scenes.interactions(joints, **kw)                          # library loaded, allocator warm
    torch.cuda.synchronize(dev)
    calls = []
    names = ('p2r_contact_bits', 'p2r_contact_intervals', 'p2r_frame_labels')
    for name in names:
        monkeypatch.setattr(idv.lib(), name, _Counted(getattr(idv.lib(), name), calls, name), raising=True)
    torch.cuda.set_sync_debug_mode("error")
    try:
        batch = scenes.interactions(joints, **kw)
        bare = scenes.interactions(joints, labels=False, **kw)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert calls == list(names) + list(names[:2])              # one launch each, as include/p2r_interaction.h states
    assert isinstance(batch, idv.InteractionBatch) and batch.scenes is scenes and (batch.H, batch.B, batch.T) == (2, 2, 130)
    assert batch._host_arrays is None and scenes._host_arrays is None and batch.bits.is_cuda and batch.label.is_cuda
    assert bare.njoint is None and bare.label is None and torch.equal(bare.clean, batch.clean)
    h = batch.host()
    ic.check_interaction(idv.Interaction(*[h.get(f) for f in idv.Interaction._fields]), ic.reference(c.name))
    assert batch.host() is h
    want = ic.reference(c.name)
    tl = batch.timeline(1, h=1)
    assert [n['intervals'] for n in tl] == [[tuple(r) for r in want.intervals[3, s, :min(want.n_intervals[3, s], c.M)].tolist()]
                                            for s in range(3)]
    assert np.array_equal(batch.labels(1, h=1), want.label[3])


# ---- 5. predict_interactions on the synthetic model -----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model(dev):
    from pose2room_amd.p2rnet.synthetic import make_batch
    from tests.test_model_cpu import build
    # the fixture of tests/test_scene_gpu.py: the far-box filter is off, as wherever `generate` runs on these weights
    net, cfg = build('test', 64, device=dev, remove_far_box=False)
    return net.to(dev).eval(), cfg, make_batch(2, 64, seed=77, device=dev)


@pytest.mark.parametrize("kw", [dict(num_hypotheses=None), dict(num_hypotheses=3, n_samples=[5, 40, 20], seed=322)],
                         ids=['deterministic', 'H3'])
def test_predict_interactions_is_the_definition_on_predict_scenes(model, kw):
    net, cfg, data = model
    H = kw['num_hypotheses'] or 1
    run = dict(contact_thresh=0.3, merge_gap=2, min_len=3, max_intervals=4)
    batch = net.predict_interactions(data, **kw, **run)
    joints = data['input_joints']
    T = joints.shape[1]
    assert isinstance(batch, idv.InteractionBatch) and (batch.H, batch.B, batch.T) == (H, 2, T)
    assert batch._host_arrays is None and batch.bits.is_cuda and batch.label.shape == (2 * H, T)
    scenes = net.predict_scenes(data, contact=True, unique=False, **kw)
    for f in ('count', 'node_obbs', 'node_rmat', 'node_score', 'contact_frame'):   # the same scenes
        assert torch.equal(getattr(batch.scenes, f), getattr(scenes, f)), f
    z = batch.scenes.host()
    want = idv.interaction_reference(_np(joints), z['count'], z['node_obbs'], z['node_rmat'], 0.3, 2, 3, 4)
    h = batch.host()
    ic.check_interaction(idv.Interaction(*[h.get(f) for f in idv.Interaction._fields]), want)
    print('predict_interactions:', kw, 'nodes', z['count'].tolist(), 'contact frames', want.n_raw.sum(1).tolist(),
          'intervals', want.n_intervals.sum(1).tolist(), 'labelled', want.n_labelled.tolist())
    assert z['count'].max() > 0 and (H == 1 or (want.n_raw.sum() > 0 and want.n_intervals.sum() > 0))
    for n in range(2 * H):
        tl = batch.timeline(n % 2, n // 2)
        assert len(tl) == z['count'][n] and [node['inst_idx'] for node in tl] == z['inst_idx'][n, :len(tl)].tolist()
        assert np.array_equal(batch.labels(n % 2, n // 2), want.label[n])
    if H == 1:                                                 # the ground-truth scene of the same batch, its stored nodes
        from pose2room_amd.net_utils.occupancy_device import scenes_from_labels
        gt = scenes_from_labels(data, cfg)
        gi, g = gt.interactions(joints, **run), gt.host()
        want = idv.interaction_reference(_np(joints), g['count'], g['node_obbs'], g['node_rmat'], 0.3, 2, 3, 4)
        ic.check_interaction(idv.Interaction(*[gi.host().get(f) for f in idv.Interaction._fields]), want)
        print('ground truth: nodes', g['count'].tolist(), 'contact frames', want.n_raw.sum(1).tolist())
        assert g['count'].max() > 0 and [len(gi.timeline(b)) for b in range(2)] == g['count'].tolist()
    default = net.predict_interactions(data, **kw)             # the distance of the training labels, no merging
    from pose2room_amd.net_utils.vote_labels import default_contact_dist
    assert default.contact_thresh == default_contact_dist() and (default.merge_gap, default.min_len, default.max_intervals) == (0, 1, 16)
    assert torch.equal(default.clean, default.bits)
