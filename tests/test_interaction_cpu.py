"""CPU: the contract of the interaction timeline (csrc/interaction.hip, net_utils/interaction_device.py) before any kernel
is involved: the definition `interaction_reference` against the inside masks recorded from the reference's own hull test
(G20) and against a case written out by hand, the order of merging and filtering, the ABI of include/p2r_interaction.h /
libp2r_interaction.so, the argument checks of the entry points and of the Python wrappers -- all of which return before
any launch --, the cases the GPU test sweeps, and the teeth of those cases: each of five wrong definitions must change a
designed case.  All results are integers: every comparison is for equality."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

from pose2room_amd import _lib
from pose2room_amd.net_utils import interaction_device as idv
from pose2room_amd.net_utils import scene_device as sd
from tests import interaction_cases as ic

EINVAL = -22
built = pytest.mark.skipif(not os.path.exists(idv.LIB_PATH), reason="libp2r_interaction.so is not built")


def _word(*frames):
    return np.array(sum(1 << f for f in frames), np.uint64).astype(np.int64)


# ---- 1. the definition -----------------------------------------------------------------------------------------------------
def test_definition_reproduces_g20():
    z = ic.g20()
    joints, count, obbs, rmat = ic.g20_design(int(z['seed']))                      # the fixture is the design, bit for bit
    for k, a in zip(('joints', 'count', 'node_obbs', 'node_rmat'), (joints, count, obbs, rmat)):
        assert np.array_equal(a, z[k]) and a.dtype == z[k].dtype, k
    assert z['joints'].shape == (1, 130, 53, 3) and z['joints'].dtype == np.float32 and z['node_obbs'].shape == (1, 6, 7)
    assert z['margin'] >= ic.MARGIN and float(z['contact_thresh']) == ic.G20_THRESH
    assert len({round(float(h), 3) for h in z['node_obbs'][0, :, 6]}) == 6 and np.abs(np.sin(2 * z['node_obbs'][0, :, 6])).min() > 0.01
    inside = np.unpackbits(z['inside'], axis=3, bitorder='little')[..., :53].astype(bool)
    assert inside.shape == (1, 6, 130, 53) and inside.any() and not inside.all()
    thr = float(z['contact_thresh'])
    assert np.array_equal(idv.reference_inside(z['joints'], z['count'], z['node_obbs'], z['node_rmat'], thr), inside)
    ref = idv.interaction_reference(z['joints'], z['count'], z['node_obbs'], z['node_rmat'], thr)
    for f in ('bits', 'njoint', 'joint_mask'):                                     # the hull test, everything it decides
        assert np.array_equal(getattr(ref, f), z[f]) and getattr(ref, f).dtype == z[f].dtype, f
    assert np.array_equal(z['njoint'], inside.sum(3)) and np.array_equal(idv.unpack_bits(z['bits'], 130), inside.any(3))
    assert np.array_equal(ref.n_raw, inside.any(3).sum(2)) and np.array_equal(ref.clean, ref.bits)


def test_definition_by_hand():
    """T = 70, two nodes, three joints; the expected words, intervals and labels written out"""
    T = 70
    obbs, rmat = np.zeros((1, 3, 7)), np.zeros((1, 3, 3, 3))
    obbs[0, 0], obbs[0, 1] = [0, 0, 0, 2, 2, 2, 0], [10, 0, 0, 2, 2, 2, 0]
    rmat[0, 0] = rmat[0, 1] = np.eye(3)
    joints = np.full((1, T, 3, 3), 50.0, np.float32)
    for t in (3, 4, 6, 62, 63, 64, 69):
        joints[0, t, 0] = [0.5, 0.5, 0.5]                      # joint 0 in node 0
    for t in (4, 62):
        joints[0, t, 2] = [-0.5, 0.0, 1.25]                    # joint 2 in node 0 too, on the enlarged face
    for t in (4, 5, 40):
        joints[0, t, 1] = [10.5, 0.0, 0.0]                     # joint 1 in node 1
    joints[0, 62, 1] = [11.26, 0.0, 0.0]                       # ... just outside
    count = np.array([2], np.int32)
    raw = idv.interaction_reference(joints, count, obbs, rmat, 0.25)
    assert raw.bits.shape == (1, 3, 2) and raw.bits.dtype == np.int64
    assert raw.bits[0, 0].tolist() == [_word(3, 4, 6, 62, 63), _word(0, 5)] and raw.bits[0, 1].tolist() == [_word(4, 5, 40), 0]
    assert not raw.bits[0, 2].any() and raw.n_raw[0].tolist() == [7, 3, 0] and raw.joint_mask[0].tolist() == [0b101, 0b010, 0]
    assert raw.njoint[0, 0, [3, 4, 5, 62]].tolist() == [1, 2, 0, 2] and raw.njoint.dtype == np.uint8
    assert np.array_equal(raw.clean, raw.bits) and raw.n_intervals[0].tolist() == [4, 2, 0]
    assert raw.intervals[0, 0, :5].tolist() == [[3, 5], [6, 7], [62, 65], [69, 70], [-1, -1]] and raw.intervals.shape == (1, 3, 16, 2)
    assert raw.label[0, [3, 4, 5, 6, 40, 62, 69, 0]].tolist() == [0, 0, 1, 0, 1, 0, 0, -1]       # frame 4: 2 joints against 1
    assert raw.n_active[0, [3, 4, 5, 0]].tolist() == [1, 2, 1, 0] and raw.n_labelled.tolist() == [9]
    got = idv.interaction_reference(joints, count, obbs, rmat, 0.25, merge_gap=1, min_len=2, max_intervals=2)
    assert got.clean[0, 0].tolist() == [_word(3, 4, 5, 6, 62, 63), _word(0)] and got.clean[0, 1].tolist() == [_word(4, 5), 0]
    assert got.n_intervals[0].tolist() == [2, 1, 0] and got.intervals[0].tolist() == [[[3, 7], [62, 65]], [[4, 6], [-1, -1]],
                                                                                    [[-1, -1], [-1, -1]]]
    assert got.n_frames[0].tolist() == [7, 2, 0] and got.first[0].tolist() == [3, 4, -1] and got.last[0].tolist() == [64, 5, -1]
    # frame 5: node 0 has the merged bit and no joint, node 1 one joint; frame 4: 2 against 1
    assert got.label[0, [3, 4, 5, 6, 40, 69]].tolist() == [0, 0, 1, 0, -1, -1] and got.n_labelled.tolist() == [7]
    assert np.array_equal(got.bits, raw.bits) and np.array_equal(got.njoint, raw.njoint)
    one = idv.interaction_reference(joints, count, obbs, rmat, 0.25, merge_gap=4, min_len=1, max_intervals=1)
    assert one.n_intervals[0].tolist() == [2, 2, 0] and one.intervals[0, :, 0].tolist() == [[3, 7], [4, 6], [-1, -1]]
    assert one.intervals[0, 0, 0].tolist() == [3, 7] and one.last[0, 0] == 69 and one.clean[0, 0, 1] == _word(0, 1, 2, 3, 4, 5)


def test_merge_comes_before_filter():
    runs = [[10, 12], [13, 15]]                                # two runs of 2 frames, 1 apart
    assert idv.clean_runs(runs, 1, 4) == [[10, 15]]
    assert idv.clean_runs(runs, 1, 4, filter_first=True) == []
    assert idv.clean_runs(runs, 0, 4) == [] and idv.clean_runs(runs, 0, 2) == runs and runs == [[10, 12], [13, 15]]
    assert idv.runs_of(np.array([1, 1, 0, 1, 0, 0, 1], bool)) == [[0, 2], [3, 4], [6, 7]] and idv.runs_of(np.zeros(5, bool)) == []
    dense = np.zeros((1, 1, 20), bool)
    dense[0, 0, [10, 11, 13, 14]] = True
    clean, n, iv, nf, first, last = idv.reference_intervals(dense, [1], 1, 4, 2)
    assert clean[0, 0, 10:15].all() and clean.sum() == 5 and n[0, 0] == 1 and iv[0, 0].tolist() == [[10, 15], [-1, -1]]
    assert (nf[0, 0], first[0, 0], last[0, 0]) == (5, 10, 14)
    assert idv.reference_intervals(dense, [1], 1, 4, 2, filter_first=True)[1][0, 0] == 0
    assert idv.reference_intervals(dense, [0], 1, 4, 2)[1][0, 0] == 0             # the slot is not counted


def test_interaction_batch_host_side():
    """InteractionBatch's host methods on CPU tensors"""
    c, ref = ic.by_name('T-130-2x2'), ic.reference('T-130-2x2')
    t = torch.from_numpy
    N, K = c.node_obbs.shape[:2]
    T = c.joints.shape[1]
    scenes = sd.SceneBatch(c.H, 2, K, t(c.count), torch.arange(N * K, dtype=torch.int32).reshape(N, K), t(c.node_obbs),
                           t(c.node_rmat), torch.full((N, K), 7, dtype=torch.int64), torch.full((N, K), 0.5))
    batch = idv.InteractionBatch(scenes, T, [t(a) for a in ref], c.thresh, c.merge_gap, c.min_len, c.M)
    assert len(batch) == 4 and (batch.H, batch.B, batch.K, batch.T) == (2, 2, 5, 130) and batch._host_arrays is None
    tl = batch.timeline(1, h=1)                                # sample 3: three nodes
    assert len(tl) == 3 and batch.timeline(0, h=1) == [] and len(batch.timeline(0)) == 5
    for s, node in enumerate(tl):
        assert node['inst_idx'] == 3 * K + s and node['class_id'] == 7 and node['score'] == 0.5
        m = min(int(ref.n_intervals[3, s]), c.M)
        assert node['intervals'] == [tuple(r) for r in ref.intervals[3, s, :m].tolist()] and node['n_intervals'] == ref.n_intervals[3, s]
        assert all(b - a >= c.min_len for a, b in node['intervals'])
        assert (node['n_frames'], node['first'], node['last']) == (ref.n_frames[3, s], ref.first[3, s], ref.last[3, s])
        assert sum(1 << j for j in node['joints']) == int(ref.joint_mask[3, s]) and node['joints'] == sorted(node['joints'])
        dense = batch.dense(3)[s]
        assert dense.sum() == node['n_frames'] and all(dense[a:b].all() for a, b in node['intervals'])
    assert any(node['intervals'] for node in tl)
    assert np.array_equal(batch.labels(1, h=1), ref.label[3]) and batch.labels(0).shape == (130,)
    assert np.array_equal(batch.dense(0, clean=False), idv.unpack_bits(ref.bits[0], T))
    with pytest.raises(IndexError):
        batch.timeline(2)
    with pytest.raises(IndexError):
        batch.dense(4)
    bare = idv.InteractionBatch(scenes, T, [t(a) for a in ref[:10]] + [None] * 3, c.thresh, c.merge_gap, c.min_len, c.M)
    assert 'label' not in bare.host() and len(bare.timeline(0)) == 5
    with pytest.raises(RuntimeError, match="labels=False"):
        bare.labels(0)
    with pytest.raises(ValueError, match="bits"):
        idv.InteractionBatch(scenes, T + 64, [t(a) for a in ref], c.thresh, c.merge_gap, c.min_len, c.M)


# ---- 2. the ABI ------------------------------------------------------------------------------------------------------------------
NAMES = ['p2r_contact_bits', 'p2r_contact_intervals', 'p2r_frame_labels']


def test_header_parses():
    from pose2room_amd.net_utils import occupancy_device, recording_repair
    protos = _lib.prototypes(idv.HEADER_PATH)
    assert sorted(protos) == _lib.declared_symbols(idv.HEADER_PATH) == NAMES
    p = protos['p2r_contact_bits']
    assert p.kinds == 'p' + 'iiiiii' + 'ppp' + 'f' + 'pppp' and p.has_stream and p.restype is ctypes.c_int
    assert p.argtypes[10] is ctypes.c_double
    assert protos['p2r_contact_intervals'].kinds == 'pp' + 'iiiiii' + 'pppppp' and protos['p2r_contact_intervals'].has_stream
    assert protos['p2r_frame_labels'].kinds == 'ppp' + 'iii' + 'ppp' and protos['p2r_frame_labels'].has_stream
    for other in (None, sd.HEADER_PATH, occupancy_device.HEADER_PATH, recording_repair.HEADER_PATH):
        assert not set(protos) & set(_lib.declared_symbols(*([other] if other else [])))
    with open(idv.HEADER_PATH) as f:
        text = f.read()
    for name, value in (('P2R_INTERACTION_MAX_K', idv.MAX_K), ('P2R_INTERACTION_MAX_T', idv.MAX_T),
                        ('P2R_INTERACTION_MAX_J', idv.MAX_J), ('P2R_INTERACTION_MAX_M', idv.MAX_M)):
        assert f"#define {name} {value} " in text
    assert (idv.MAX_K, idv.MAX_T, idv.MAX_J, idv.MAX_M) == (sd.MAX_K, sd.MAX_T, sd.MAX_J, 64)
    assert 'size_t' not in _lib._code(idv.HEADER_PATH) and len(idv.Interaction._fields) == 13


@built
def test_every_prototype_binds_and_library_exports_exactly_them():
    protos = _lib.prototypes(idv.HEADER_PATH)
    out = subprocess.run(["nm", "-D", "--defined-only", idv.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if " T " in ln and ln.split()[-1].startswith("p2r_")}
    assert exported == set(protos)
    for name, p in protos.items():
        fn = getattr(idv.lib(), name)
        assert fn.argtypes == p.argtypes and fn.restype is p.restype
    assert os.path.basename(idv.LIB_PATH) == 'libp2r_interaction.so'
    for other in (_lib.LIB_PATH, sd.LIB_PATH):
        out = subprocess.run(["nm", "-D", "--defined-only", other], capture_output=True, text=True, check=True).stdout
        assert not any(n in out for n in ('p2r_contact_bits', 'p2r_contact_intervals', 'p2r_frame_labels'))


# ---- 3. argument checks: on the host, before any launch ---------------------------------------------------------------------
_BUF = ctypes.create_string_buffer(64)          # a non-NULL address; never read, every call is refused first
_P = ctypes.addressof(_BUF)


def bits_args(**over):
    a = dict(joints=_P, B=2, T=70, J=7, C=3, N=4, K=5, node_obbs=_P, node_rmat=_P, count=_P, contact_thresh=0.1, bits=_P,
             njoint=_P, joint_mask=_P, n_raw=_P)
    a.update(over)
    return list(a.values()) + [None]


def intervals_args(**over):
    a = dict(bits=_P, count=_P, N=4, K=5, T=70, merge_gap=1, min_len=2, M=16, clean=_P, n_intervals=_P, intervals=_P,
             n_frames=_P, first=_P, last=_P)
    a.update(over)
    return list(a.values()) + [None]


def labels_args(**over):
    a = dict(clean=_P, njoint=_P, count=_P, N=4, K=5, T=70, label=_P, n_active=_P, n_labelled=_P)
    a.update(over)
    return list(a.values()) + [None]


BAD_BITS = [dict(T=0), dict(T=-1), dict(T=65536), dict(J=0), dict(J=65), dict(C=2), dict(C=5), dict(B=0), dict(B=3),
            dict(N=-1), dict(K=-1), dict(K=1025), dict(N=1 << 16, B=1, K=1024, T=65535), dict(N=1 << 22, B=1, K=1024, T=1),
            dict(joints=None), dict(node_obbs=None), dict(node_rmat=None), dict(count=None), dict(bits=None),
            dict(joint_mask=None), dict(n_raw=None)]
BAD_INTERVALS = [dict(T=0), dict(T=65536), dict(N=-1), dict(K=-1), dict(K=1025), dict(M=0), dict(M=65), dict(min_len=0),
                 dict(min_len=71), dict(merge_gap=-1), dict(merge_gap=71), dict(N=1 << 16, K=1024, T=65535),
                 dict(N=1 << 15, K=1024, T=1, M=64), dict(bits=None), dict(count=None), dict(clean=None),
                 dict(n_intervals=None), dict(intervals=None), dict(n_frames=None), dict(first=None), dict(last=None)]
BAD_LABELS = [dict(T=0), dict(T=65536), dict(N=-1), dict(K=-1), dict(K=1025), dict(N=1 << 16, K=1024, T=65535),
              dict(clean=None), dict(njoint=None), dict(count=None), dict(label=None), dict(n_active=None),
              dict(n_labelled=None)]


@built
def test_entry_points_refuse_bad_arguments():
    l = idv.lib()
    for fn, args, bads in ((l.p2r_contact_bits, bits_args, BAD_BITS), (l.p2r_contact_intervals, intervals_args, BAD_INTERVALS),
                           (l.p2r_frame_labels, labels_args, BAD_LABELS)):
        for bad in bads:
            assert fn(*args(**bad)) == EINVAL, (fn.__name__, bad)
    # problems without an output element: 0, and nothing launched (there is no device here to launch on); a NULL njoint
    # is no reason to refuse the bits call
    for empty in (dict(N=0), dict(K=0)):
        none = dict(joints=None, node_obbs=None, node_rmat=None, count=None, bits=None, njoint=None, joint_mask=None, n_raw=None)
        assert l.p2r_contact_bits(*bits_args(**empty, **none)) == 0
        none = dict(bits=None, count=None, clean=None, n_intervals=None, intervals=None, n_frames=None, first=None, last=None)
        assert l.p2r_contact_intervals(*intervals_args(**empty, **none)) == 0
    assert l.p2r_frame_labels(*labels_args(N=0, clean=None, njoint=None, count=None, label=None, n_active=None,
                                           n_labelled=None)) == 0
    assert l.p2r_contact_bits(*bits_args(njoint=None, T=0)) == EINVAL             # still refused for its own reasons


def _cpu_inputs(N=4, K=5, B=2, T=70, J=7):
    return dict(joints=torch.zeros(B, T, J, 3), node_obbs=torch.zeros(N, K, 7, dtype=torch.float64),
                node_rmat=torch.zeros(N, K, 3, 3, dtype=torch.float64), count=torch.zeros(N, dtype=torch.int32))


def test_wrappers_refuse_cpu_tensors_and_bad_shapes():
    ok = _cpu_inputs()
    with pytest.raises(RuntimeError, match="GPU tensor"):
        idv.contact_bits(**ok, contact_thresh=0.1)
    for name, bad in (('joints', ok['joints'].double()), ('joints', ok['joints'][..., :2]), ('joints', ok['joints'][0]),
                      ('joints', torch.zeros(2, 70, 65, 3)), ('node_obbs', ok['node_obbs'].float()),
                      ('node_obbs', ok['node_obbs'][..., :6]), ('node_obbs', 'x'), ('node_rmat', ok['node_rmat'].float()),
                      ('node_rmat', ok['node_rmat'][:, :, :2]), ('count', ok['count'].long()), ('count', ok['count'][:3])):
        with pytest.raises(ValueError, match=name):
            idv.contact_bits(**{**ok, name: bad}, contact_thresh=0.1)
    with pytest.raises(ValueError, match="multiple of"):
        idv.contact_bits(**{**ok, 'joints': torch.zeros(3, 70, 7, 3)}, contact_thresh=0.1)
    with pytest.raises(ValueError, match="at most 1024"):
        idv.contact_bits(**_cpu_inputs(2, 1025), contact_thresh=0.1)
    bits, count = torch.zeros(4, 5, 2, dtype=torch.int64), ok['count']
    with pytest.raises(RuntimeError, match="GPU tensor"):
        idv.contact_intervals(bits, count, 70)
    for bad in (bits.int(), bits[..., :1], bits[0], 'x'):
        with pytest.raises(ValueError, match="bits"):
            idv.contact_intervals(bad, count, 70)
    with pytest.raises(ValueError, match="bits"):
        idv.contact_intervals(bits, count, 129)                # three words
    with pytest.raises(ValueError, match="count"):
        idv.contact_intervals(bits, count[:3], 70)
    for kw, what in ((dict(merge_gap=-1), "merge_gap"), (dict(merge_gap=71), "merge_gap"), (dict(min_len=0), "min_len"),
                     (dict(min_len=71), "min_len"), (dict(max_intervals=0), "max_intervals"),
                     (dict(max_intervals=65), "max_intervals")):
        with pytest.raises(ValueError, match=what):
            idv.contact_intervals(bits, count, 70, **kw)
    for T in (0, 65536):
        with pytest.raises(ValueError, match="frames"):
            idv.contact_intervals(bits, count, T)
    njoint = torch.zeros(4, 5, 70, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        idv.frame_labels(bits, njoint, count)
    for bad in (None, njoint.int(), njoint[0]):
        with pytest.raises(ValueError, match="njoint"):
            idv.frame_labels(bits, bad, count)
    with pytest.raises(ValueError, match="clean"):
        idv.frame_labels(bits[..., :1], njoint, count)
    with pytest.raises(ValueError, match="count"):
        idv.frame_labels(bits, njoint, count.long())
    with pytest.raises(TypeError, match="SceneBatch"):
        idv.interactions_of(ok, ok['joints'])
    scenes = sd.SceneBatch(2, 2, 5, ok['count'], torch.zeros(4, 5, dtype=torch.int32), ok['node_obbs'], ok['node_rmat'],
                           torch.zeros(4, 5, dtype=torch.int64), torch.zeros(4, 5))
    with pytest.raises(RuntimeError, match="GPU tensor"):
        scenes.interactions(ok['joints'])
    with pytest.raises(ValueError, match="joints"):
        scenes.interactions(torch.zeros(3, 70, 7, 3))
    with pytest.raises(ValueError, match="min_len"):
        scenes.interactions(ok['joints'], min_len=0)
    with pytest.raises(ValueError, match="max_intervals"):
        scenes.interactions(ok['joints'], max_intervals=65)


def test_default_contact_thresh_is_the_training_labels_distance(monkeypatch):
    from pose2room_amd.net_utils import vote_labels
    ok, seen = _cpu_inputs(), []
    scenes = sd.SceneBatch(2, 2, 5, ok['count'], torch.zeros(4, 5, dtype=torch.int32), ok['node_obbs'], ok['node_rmat'],
                           torch.zeros(4, 5, dtype=torch.int64), torch.zeros(4, 5))

    class Stop(Exception):
        pass

    def stop(joints, node_obbs, node_rmat, count, contact_thresh, njoint=True):
        seen.append((contact_thresh, njoint))
        raise Stop

    monkeypatch.setattr(idv, 'contact_bits', stop)
    for kw in (dict(), dict(contact_thresh=0.3, labels=False)):
        with pytest.raises(Stop):
            scenes.interactions(ok['joints'], **kw)
    assert seen == [(vote_labels.default_contact_dist(), True), (0.3, False)]


def test_a_missing_library_is_an_error(monkeypatch):
    monkeypatch.setattr(idv._library, 'lib_path', os.path.join(os.path.dirname(idv.LIB_PATH), 'libp2r_interaction_absent.so'))
    monkeypatch.setattr(idv._library, '_handle', None)
    with pytest.raises(_lib.P2RLibraryError, match="libp2r_interaction_absent.so is missing"):
        idv.lib()


# ---- 4. the cases and their teeth ----------------------------------------------------------------------------------------------
def test_sweep_covers_what_it_claims():
    cases = ic.sweep()
    assert {c.situation for c in cases} == {'T', 'K = 0', 'count = 0', 'patterns', 'dyadic', 'ties', 'bad count', 'saturate'}
    for c in cases:
        worst, zeros = ic.assert_margin(c)                    # every case, no joint excused
        assert worst >= ic.MARGIN and (zeros > 0) == c.dyadic
        ref = ic.reference(c.name)
        ic.check_interaction(ref, ref)
        assert c.joints.dtype == np.float32 and c.joints.size <= 80000, c.name                # a third of a megabyte at most
    shape = lambda c: (c.joints.shape[1], c.joints.shape[2], c.joints.shape[3], c.node_obbs.shape[1])     # noqa: E731
    assert sorted(shape(c)[0] for c in cases if c.situation == 'T') == [1, 63, 64, 65, 130, 4097]
    assert {shape(c)[1] for c in cases} >= {1, 53, 64} and {shape(c)[2] for c in cases} == {3, 4}
    assert {shape(c)[3] for c in cases} >= {0, 1, 4, 5}
    for c in (c for c in cases if c.situation == 'T'):
        assert ic.reference(c.name).n_raw.max() > 0, c.name
    assert {(c.H, c.joints.shape[0]) for c in cases} >= {(2, 2), (3, 1), (1, 2), (1, 1)}
    counts = {(int(n), c.node_obbs.shape[1]) for c in cases for n in c.count}
    assert any(n == 0 and K > 0 for n, K in counts) and any(n == 1 and K > 1 for n, K in counts) and any(n == K > 1 for n, K in counts)
    c, ref = ic.by_name('T-4097-3x1'), ic.reference('T-4097-3x1')
    assert ref.bits.shape[2] == 65 and ref.clean[:, :, :64].any()                 # two chunks of words; the last frame is
    assert ic.reference('patterns-4097').bits[0, :, 64].any()                    # in contact in the constructed case
    assert (ref.clean != ref.bits).any() and ref.n_intervals.max() > 1
    assert not ic.reference('K-0').bits.size and ic.reference('K-0').label.shape == (2, 10) and (ic.reference('K-0').label == -1).all()
    assert not ic.reference('none-kept').bits.any() and (ic.reference('none-kept').intervals == -1).all()
    # the constructed patterns
    c, ref = ic.by_name('patterns-130'), ic.reference('patterns-130')
    names = list(ic.PATTERNS_130)
    assert c.node_obbs.shape[1] == len(names) + 1 and c.count[0] == len(names) and (c.merge_gap, c.min_len, c.M) == (3, 4, 3)
    for s, runs in enumerate(ic.PATTERNS_130.values()):
        assert np.array_equal(idv.unpack_bits(ref.bits[0, s], 130), ic.spans(130, *runs)), names[s]
    row = lambda name: names.index(name)                                            # noqa: E731
    iv = lambda name: ref.intervals[0, row(name), :ref.n_intervals[0, row(name)]].tolist()      # noqa: E731
    assert iv('ends at bit 63') == [[60, 64]] and ref.clean[0, row('ends at bit 63')].tolist() == [_word(60, 61, 62, 63), 0, 0]
    assert iv('starts at bit 0 of the next word') == [[64, 70]] and iv('over three words') == [[30, 129]]
    assert iv('ends at T-1') == [[120, 130]] and ref.last[0, row('ends at T-1')] == 129
    assert iv('all frames') == [[0, 130]] and ref.clean[0, row('all frames')].tolist() == [-1, -1, 3]
    assert iv('none') == [] and ref.first[0, row('none')] == -1
    assert iv('gap of merge_gap across a word boundary') == [[55, 70]]
    assert iv('gap of merge_gap + 1 across a word boundary') == [[55, 62], [66, 70]]
    assert iv('runs of min_len and min_len - 1') == [[10, 14]]
    s = row('more than M intervals')
    assert ref.n_intervals[0, s] == 6 > c.M and ref.intervals[0, s].tolist() == [[0, 4], [10, 14], [20, 24]] and ref.last[0, s] == 129
    assert iv('merged, then long enough') == [[10, 17]] and iv('single frames at the word edges') == []
    assert ref.n_raw[0, row('single frames at the word edges')] == 5 and not ref.bits[0, len(names)].any()
    ref = ic.reference('patterns-4097')
    assert ref.n_intervals[0].tolist() == [1, 2, 1, 0, 2, 58] and ref.intervals[0, 0, 0].tolist() == [4000, 4097]
    assert ref.intervals[0, 1, :2].tolist() == [[5, 9], [4090, 4097]] and ref.intervals[0, 2, 0].tolist() == [0, 4096]
    assert ref.intervals[0, 4, :2].tolist() == [[100, 2000], [2003, 4000]] and (ref.intervals[0, 5, :58] >= 0).all()
    # exact faces, NaN, ties
    c, ref = ic.by_name('dyadic'), ic.reference('dyadic')
    assert np.isnan(c.joints).any() and np.isinf(c.joints).any()
    assert ref.njoint[0, :, 0].tolist() == [1, 1, 1, 1] and ref.njoint[0, :, 1].tolist() == [0, 0, 0, 1]       # on / beyond the face
    assert ref.njoint[0, :3, 2].tolist() == [2, 2, 2] and ref.njoint[0, :, 3].tolist() == [1, 1, 1, 1]         # edge, corner; NaN
    assert ref.njoint[0, :, 4].tolist() == [0, 0, 0, 0] and ref.label[0].tolist() == [0, 3, 0, 0, -1, 0]
    assert ref.njoint[0, :, 5].tolist() == [3, 3, 3, 3] and ref.njoint[1, 0].tolist() == [1, 0, 0, 0, 0, 0]
    ref = ic.reference('ties')
    both = idv.unpack_bits(ref.clean[0, 0], 70) & idv.unpack_bits(ref.clean[0, 2], 70)
    assert np.array_equal(ref.njoint[0, 0], ref.njoint[0, 1]) and both.any() and (ref.label != 1).all() and (ref.label == 0).any()
    c, ref = ic.by_name('bad-count'), ic.reference('bad-count')
    assert c.count.tolist() == [-2, 6] and c.node_obbs.shape[1] == 3 and not ref.bits[0].any() and ref.bits[1].any()
    ref = ic.reference('saturate-K260')
    assert ref.n_active[0].tolist() == [255, 0, 255] and ref.label[0].tolist() == [0, -1, 0]


MUTATIONS = {
    'lt-for-le': (dict(strict=True), 'dyadic'),
    'threshold-on-the-size': (dict(thresh_on_size=True), 'dyadic'),
    'filter-before-merge': (dict(filter_first=True), 'patterns-130'),
    'tie-to-higher-slot': (dict(tie='high'), 'ties'),
    'end-inclusive': (dict(end_inclusive=True), 'patterns-130'),
}
SMALL_CASES = [c.name for c in ic.sweep() if c.joints.shape[1] <= 130]


@pytest.mark.parametrize("mutation", sorted(MUTATIONS))
def test_wrong_definitions_are_caught(mutation):
    kw, designed = MUTATIONS[mutation]
    caught = []
    for name in SMALL_CASES:
        c = ic.by_name(name)
        wrong = idv.interaction_reference(*ic.inputs(c), *ic.run_args(c), **kw)
        try:
            ic.check_interaction(wrong, ic.reference(name))
        except AssertionError:
            caught.append(name)
    assert designed in caught, (mutation, caught)
    if mutation == 'threshold-on-the-size':                    # random scenes tell it too, not the constructed one alone
        assert 'T-130-2x2' in caught


def test_a_single_bit_is_caught():
    want = ic.reference('T-65')
    for f in ('bits', 'clean'):
        a = getattr(want, f).copy()
        a[1, 0, 1] ^= np.int64(1) << np.int64(63)             # a padding bit
        with pytest.raises(AssertionError):
            ic.check_interaction(want._replace(**{f: a}), want)
    a = want.joint_mask.copy()
    a[1, 4] ^= np.int64(1) << np.int64(63)
    with pytest.raises(AssertionError):
        ic.check_interaction(want._replace(joint_mask=a), want)
    for f in ('njoint', 'n_raw', 'n_intervals', 'intervals', 'n_frames', 'first', 'last', 'label', 'n_active', 'n_labelled'):
        a = getattr(want, f).copy()
        a[(-1,) * a.ndim] += 1
        with pytest.raises(AssertionError):
            ic.check_interaction(want._replace(**{f: a}), want)
