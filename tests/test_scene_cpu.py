"""CPU: the contract of the scene read-out on the device (csrc/scene.hip, net_utils/scene_device.py) before any kernel is
involved: the float64 definitions of tests/scene_cases.py against the reference's own results (G15), the record layout
against `multi_modal_eval.confident_boxes`, the ABI of include/p2r_scene.h / libp2r_scene.so, the argument checks of the
entry points and of the Python wrappers -- all of which return before any launch -- and the teeth of the comparison
functions that the GPU test shares: each of four wrong definitions must be caught by them."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

from pose2room_amd import _lib
from pose2room_amd.net_utils import multi_modal_eval as mm
from pose2room_amd.net_utils import scene_device as sd
from tests import scene_cases as sc

EINVAL = -22
built = pytest.mark.skipif(not os.path.exists(sd.LIB_PATH), reason="libp2r_scene.so is not built")


def _g15_nodes(z, **kw):
    return sc.nodes_def(z['box_params'], z['obj_prob'], z['pred_mask'], z['pred_sem_cls'], float(z['dump_threshold']), **kw)


# ---- 1. the definitions against the reference -----------------------------------------------------------------------------
def test_definitions_reproduce_g15():
    z = sc.g15()
    N, K = z['obj_prob'].shape
    assert (N, K) == (3, 24) and z['input_joints'].shape == (3, 40, 53, 3)
    # the box parameters the nodes are made of: the repository's host restatement against the reference's
    np.testing.assert_allclose(mm.corners_to_params(z['pred_corners_3d']).reshape(N, K, 7), z['box_params'], rtol=0,
                               atol=1e-12)
    nd = _g15_nodes(z)
    un = sc.unique_def(z['input_joints'])
    ct = sc.contact_def(z['input_joints'], nd.node_obbs, nd.node_rmat, nd.count)
    assert sc.assert_contact_margins(z['input_joints'], ct, nd.count) >= sc.CONTACT_MARGIN
    assert np.array_equal(un.count, z['unique_count']) and np.array_equal(un.index, z['unique_index'])
    assert (un.count < 40).all()                                   # the fixture has duplicates, adjacent and distant
    for b in range(N):
        kept = np.nonzero(z['keep'][b])[0]
        m = len(kept)
        assert m >= 1 and nd.count[b] == m and np.array_equal(nd.inst_idx[b, :m], kept)
        assert np.array_equal(nd.node_rmat[b, :m], z['rmat'][b, kept])          # head2rot of the reference, bit for bit
        assert np.array_equal(un.rank[b][ct.frame[b, :m]], z['contact_unique'][b, kept])
    # the de-duplication matters to the index: some contact frame lies behind a removed frame
    assert any((un.rank[b][ct.frame[b, :nd.count[b]]] != ct.frame[b, :nd.count[b]]).any() for b in range(N))


def test_records_layout_is_confident_boxes():
    z = sc.g15()
    thr = float(z['dump_threshold'])
    want = mm.confident_boxes(None, {'pred_mask': z['pred_mask']},
                              {'pred_corners_3d': z['pred_corners_3d'], 'obj_prob': z['obj_prob'],
                               'pred_sem_cls': z['pred_sem_cls']}, thr)
    N, K = z['obj_prob'].shape
    obbs = mm.corners_to_params(z['pred_corners_3d']).reshape(N, K, 7)
    nd = sc.nodes_def(obbs, z['obj_prob'], z['pred_mask'], z['pred_sem_cls'], thr)
    got = sd.records_from_nodes(nd.count, nd.inst_idx, nd.node_obbs, nd.node_cls)
    assert len(got) == len(want) == N
    for g, w in zip(got, want):
        assert list(g) == list(w) == ['obbs', 'cls', 'inst_idx']
        for k in g:
            assert g[k].dtype == w[k].dtype and g[k].shape == w[k].shape and np.array_equal(g[k], w[k]), k
    # a sample without a confident box: a record without instances, and no file
    empty = sd.records_from_nodes(np.zeros(1, np.int32), np.full((1, K), -1, np.int32), np.zeros((1, K, 7)),
                                  np.zeros((1, K), np.int64))[0]
    assert empty['obbs'].shape == (0, 7) and empty['cls'].shape == (0,) and empty['inst_idx'].shape == (K,)
    assert not empty['inst_idx'].any()


def test_scene_batch_host_side(tmp_path):
    """SceneBatch's host methods on CPU tensors (`host()` takes whatever device the tensors are on): node dicts as
    demo.py builds them, the npz layout of the reference's dump, and no file for a sample without nodes"""
    z = sc.g15()
    nd = _g15_nodes(z)
    un = sc.unique_def(z['input_joints'])
    ct = sc.contact_def(z['input_joints'], nd.node_obbs, nd.node_rmat, nd.count)
    nd.count[1] = 0                                                 # sample 1 without nodes
    t = torch.from_numpy
    batch = sd.SceneBatch(1, 3, 24, *[t(a) for a in nd], t(ct.frame), t(ct.dist), *[t(a) for a in un])
    nodes = batch.nodes(2)
    kept = np.nonzero(z['keep'][2])[0]
    assert len(batch) == 3 and len(nodes) == len(kept) and batch.nodes(1) == []
    for node, k in zip(nodes, kept):
        assert set(node) == {'centroid', 'R_mat', 'size', 'class_id', 'score', 'inst_idx', 'contact_frame',
                             'contact_dist', 'contact_frame_unique'}
        assert np.array_equal(node['centroid'], z['box_params'][2, k, 0:3])
        assert np.array_equal(node['size'], z['box_params'][2, k, 3:6]) and np.array_equal(node['R_mat'], z['rmat'][2, k])
        assert node['class_id'] == [z['pred_sem_cls'][2, k]] and node['inst_idx'] == k
        assert node['contact_frame_unique'] == z['contact_unique'][2, k]
    assert np.array_equal(batch.unique(0), z['unique_index'][0, :z['unique_count'][0]])
    path = str(tmp_path / '000000_pred_confident_nms_bbox.npz')
    assert batch.save_npz(path, 2) is True
    with np.load(path) as f:
        assert sorted(f.files) == ['cls', 'inst_idx', 'obbs']
        assert np.array_equal(f['obbs'], z['box_params'][2, kept]) and np.array_equal(f['inst_idx'], z['keep'][2])
        assert np.array_equal(f['cls'], z['pred_sem_cls'][2, kept])
    other = str(tmp_path / 'none.npz')
    assert batch.save_npz(other, 1) is False and not os.path.exists(other)


# ---- 2. the ABI -------------------------------------------------------------------------------------------------------------
NAMES = ['p2r_contact_frames', 'p2r_scene_nodes', 'p2r_unique_frames']


def test_header_parses():
    from pose2room_amd.net_utils import ap_device, mm_device, parse_device, vote_labels
    protos = _lib.prototypes(sd.HEADER_PATH)
    assert sorted(protos) == _lib.declared_symbols(sd.HEADER_PATH) == NAMES
    assert protos['p2r_scene_nodes'].kinds == 'ii' + 'pppp' + 'f' + 'pppppp'
    assert protos['p2r_contact_frames'].kinds == 'p' + 'iiiiii' + 'ppppp'
    assert protos['p2r_unique_frames'].kinds == 'p' + 'iiii' + 'ppp'
    assert all(p.has_stream and p.restype is ctypes.c_int for p in protos.values())
    for other in (None, ap_device.HEADER_PATH, mm_device.HEADER_PATH, vote_labels.HEADER_PATH, parse_device.HEADER_PATH):
        assert not set(protos) & set(_lib.declared_symbols(*([other] if other else [])))
    with open(sd.HEADER_PATH) as f:
        text = f.read()
    for name, value in (('P2R_SCENE_MAX_K', sd.MAX_K), ('P2R_SCENE_MAX_T', sd.MAX_T), ('P2R_SCENE_MAX_J', sd.MAX_J),
                        ('P2R_UNIQUE_MAX_T', sd.UNIQUE_MAX_T)):
        assert f"#define {name} {value} " in text
    assert sd.UNIQUE_MAX_T >= 4096


@built
def test_every_prototype_binds_and_library_exports_exactly_them():
    protos = _lib.prototypes(sd.HEADER_PATH)
    out = subprocess.run(["nm", "-D", "--defined-only", sd.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if " T " in ln and ln.split()[-1].startswith("p2r_")}
    assert exported == set(protos)
    for name, p in protos.items():
        fn = getattr(sd.lib(), name)
        assert fn.argtypes == p.argtypes and fn.restype is ctypes.c_int
    assert os.path.basename(sd.LIB_PATH) == 'libp2r_scene.so'
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert not any(name in out for name in NAMES)


# ---- 3. argument checks: on the host, before any launch ---------------------------------------------------------------------
_BUF = ctypes.create_string_buffer(64)          # a non-NULL address; never read, every call below is refused first
_P = ctypes.addressof(_BUF)


@built
def test_entry_points_refuse_bad_arguments():
    l = sd.lib()
    good = dict(N=2, K=5, obbs=_P, obj_prob=_P, pred_mask=_P, pred_cls=_P, thr=0.5, count=_P, inst_idx=_P, node_obbs=_P,
                node_rmat=_P, node_cls=_P, node_score=_P)
    for bad in [dict(N=-1), dict(K=-1), dict(K=1025), dict(N=1 << 22, K=1 << 10)] + [{k: None} for k in good if good[k] == _P]:
        assert l.p2r_scene_nodes(*{**good, **bad}.values(), None) == EINVAL, bad
    good = dict(joints=_P, B=2, T=8, J=53, C=3, N=4, K=5, node_obbs=_P, node_rmat=_P, count=_P, frame=_P, dist=_P)
    for bad in [dict(N=-2), dict(B=0), dict(N=3), dict(T=0), dict(T=65536), dict(J=0), dict(J=65), dict(C=2), dict(C=5),
                dict(K=-1), dict(K=1025), dict(N=1 << 22, K=1 << 10)] + [{k: None} for k in good if good[k] == _P]:
        assert l.p2r_contact_frames(*{**good, **bad}.values(), None) == EINVAL, bad
    good = dict(joints=_P, B=2, T=8, J=53, C=4, count=_P, index=_P, rank=_P)
    for bad in [dict(B=-1), dict(T=0), dict(T=4097), dict(J=0), dict(J=65), dict(C=2), dict(C=5)] + \
            [{k: None} for k in good if good[k] == _P]:
        assert l.p2r_unique_frames(*{**good, **bad}.values(), None) == EINVAL, bad
    # problems without an output element: 0, and nothing launched (there is no device here to launch on)
    assert l.p2r_scene_nodes(0, 5, *[None] * 4, 0.5, *[None] * 6, None) == 0
    assert l.p2r_contact_frames(None, 1, 8, 53, 3, 0, 5, *[None] * 5, None) == 0
    assert l.p2r_contact_frames(None, 2, 8, 53, 3, 4, 0, *[None] * 5, None) == 0
    assert l.p2r_unique_frames(None, 0, 8, 53, 3, None, None, None, None) == 0


def test_wrappers_refuse_cpu_tensors_and_bad_shapes():
    N, K, B, T, J = 4, 5, 2, 8, 3
    nodes = dict(obbs=torch.zeros(N, K, 7, dtype=torch.float64), obj_prob=torch.zeros(N, K),
                 pred_mask=torch.zeros(N, K, dtype=torch.uint8), pred_cls=torch.zeros(N, K, dtype=torch.int64))
    with pytest.raises(RuntimeError, match="GPU tensor"):
        sd.scene_nodes(**nodes, dump_threshold=0.5)
    for name, bad in (('obbs', nodes['obbs'].float()), ('obj_prob', nodes['obj_prob'].double()),
                      ('pred_mask', nodes['pred_mask'].bool()), ('pred_cls', nodes['pred_cls'].int()),
                      ('obj_prob', nodes['obj_prob'][:, :4])):
        with pytest.raises(ValueError, match=name):
            sd.scene_nodes(**{**nodes, name: bad}, dump_threshold=0.5)
    with pytest.raises(ValueError, match="at most 1024"):
        sd.scene_nodes(torch.zeros(1, 1025, 7, dtype=torch.float64), torch.zeros(1, 1025),
                       torch.zeros(1, 1025, dtype=torch.uint8), torch.zeros(1, 1025, dtype=torch.int64), 0.5)

    joints = torch.zeros(B, T, J, 3)
    contact = dict(joints=joints, node_obbs=torch.zeros(N, K, 7, dtype=torch.float64),
                   node_rmat=torch.zeros(N, K, 3, 3, dtype=torch.float64), count=torch.zeros(N, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="GPU tensor"):
        sd.contact_frames(**contact)
    with pytest.raises(ValueError, match="multiple of B"):
        sd.contact_frames(**{**contact, 'joints': torch.zeros(3, T, J, 3)})
    for name, bad, match in (('joints', joints.double(), 'joints must be float32'),
                             ('joints', torch.zeros(B, T, J, 2), 'joints must be float32'),
                             ('joints', torch.zeros(B, T, 65, 3), 'joints'), ('joints', torch.zeros(B, 0, J, 3), 'frames'),
                             ('joints', torch.zeros(1, 65536, 1, 3), 'frames'),
                             ('node_rmat', contact['node_rmat'].float(), 'node_rmat'),
                             ('node_rmat', torch.zeros(N, K, 9, dtype=torch.float64), 'node_rmat'),
                             ('count', contact['count'].long(), 'count'),
                             ('node_obbs', torch.zeros(N, 1025, 7, dtype=torch.float64), 'at most 1024')):
        with pytest.raises(ValueError, match=match):
            sd.contact_frames(**{**contact, name: bad})

    with pytest.raises(RuntimeError, match="GPU tensor"):
        sd.unique_frames(joints)
    for bad in (joints.double(), torch.zeros(B, 4097, 1, 3), torch.zeros(B, T, 65, 4), torch.zeros(B, T, J)):
        with pytest.raises(ValueError, match="joints|frames"):
            sd.unique_frames(bad)
    with pytest.raises(ValueError, match="stack of 3 hypotheses"):
        sd.scenes_from_parsed(torch.zeros(N, K, 8, 3, dtype=torch.float64), nodes['obj_prob'], nodes['pred_mask'],
                              nodes['pred_cls'], joints, num_hypotheses=3)


def test_a_missing_library_is_an_error(monkeypatch):
    monkeypatch.setattr(sd._library, 'lib_path', os.path.join(os.path.dirname(sd.LIB_PATH), 'libp2r_scene_absent.so'))
    monkeypatch.setattr(sd._library, '_handle', None)
    with pytest.raises(_lib.P2RLibraryError, match="libp2r_scene_absent.so is missing"):
        sd.lib()


# ---- 4. the cases and the teeth of the comparison functions ---------------------------------------------------------------------
def test_sweep_covers_what_it_claims():
    cases = sc.sweep()
    dims = lambda c: (c.obbs.shape[1], *c.joints.shape[1:], c.obbs.shape[0] // c.joints.shape[0])   # noqa: E731  K,T,J,C,H
    assert {dims(c)[0] for c in cases} == {1, 24, 65, 128} and {dims(c)[1] for c in cases} == {1, 40, 257}
    assert {dims(c)[2] for c in cases} == {1, 53} and {dims(c)[3] for c in cases} == {3, 4}
    assert {dims(c)[4] for c in cases} == {1, 2}
    for K in (1, 24, 65, 128):
        assert {(dims(c)[1]) for c in cases if dims(c)[0] == K} == {1, 40, 257}
    kept = set()
    for c in cases:
        nd = sc.nodes_def(c.obbs, c.obj_prob, c.pred_mask, c.pred_cls, c.threshold)
        ct = sc.contact_def(c.joints, nd.node_obbs, nd.node_rmat, nd.count)
        sc.assert_contact_margins(c.joints, ct, nd.count, c.mirror, c.skip_rows)
        K, T = dims(c)[:2]
        kept.add('none' if not nd.count.any() else 'all' if (nd.count == K).all() else 'mixed')
        if T >= 32:
            un = sc.unique_def(c.joints)
            eq = sc.rows_equal_matrix(c.joints[1])
            assert eq[6, 7] and eq[3, T - 2] and eq[11, 12] and not eq[16, 16] and not eq[16, 17]
            assert np.signbit(c.joints[1, 12]).sum() == np.signbit(c.joints[1, 11]).sum() + 1       # the -0.0
            assert un.rank[1, 16] != un.rank[1, 17] and un.rank[1, 12] == un.rank[1, 11] and (un.count < T).all()
        if c.mirror is not None:
            b, lo, hi = c.mirror
            assert lo < hi and not sc.rows_equal_matrix(c.joints[b])[lo, hi]
            assert ct.frame[0, 0] == lo and ct.d[(0, 0)][lo] == ct.d[(0, 0)][hi] == ct.dist[0, 0]
    assert kept == {'none', 'all', 'mixed'}
    assert sum(c.mirror is not None for c in cases) >= 4


def _tie_case():
    return next(c for c in sc.sweep() if c.mirror is not None and c.joints.shape[2] == 53 and c.obbs.shape[1] >= 24)


def test_last_minimum_instead_of_first_is_caught():
    c = _tie_case()
    nd = sc.nodes_def(c.obbs, c.obj_prob, c.pred_mask, c.pred_cls, c.threshold)
    want = sc.contact_def(c.joints, nd.node_obbs, nd.node_rmat, nd.count)
    sc.check_contact(want.frame, want.dist, want, c.joints, nd.node_obbs, nd.count, c.skip_rows)
    wrong = sc.contact_def(c.joints, nd.node_obbs, nd.node_rmat, nd.count, pick='last')
    assert wrong.frame[0, 0] == c.mirror[2] and wrong.dist[0, 0] == want.dist[0, 0]      # the same distance, the later frame
    with pytest.raises(AssertionError):
        sc.check_contact(wrong.frame, wrong.dist, want, c.joints, nd.node_obbs, nd.count, c.skip_rows)
    # and in G15, where equal rows tie
    z = sc.g15()
    nd = _g15_nodes(z)
    want = sc.contact_def(z['input_joints'], nd.node_obbs, nd.node_rmat, nd.count)
    wrong = sc.contact_def(z['input_joints'], nd.node_obbs, nd.node_rmat, nd.count, pick='last')
    un = sc.unique_def(z['input_joints'])
    if not np.array_equal(wrong.frame, want.frame):
        assert np.array_equal(un.rank[0][wrong.frame[0, :nd.count[0]]], un.rank[0][want.frame[0, :nd.count[0]]])
        with pytest.raises(AssertionError):
            sc.check_contact(wrong.frame, wrong.dist, want, z['input_joints'], nd.node_obbs, nd.count)


def test_a_distance_outside_the_bound_is_caught():
    c = _tie_case()
    nd = sc.nodes_def(c.obbs, c.obj_prob, c.pred_mask, c.pred_cls, c.threshold)
    want = sc.contact_def(c.joints, nd.node_obbs, nd.node_rmat, nd.count)
    dist = want.dist.copy()
    dist[0, 1] += 1e-13                                             # the bound is a few 1e-15 at room scale
    bound = sc.dist_bound(c.joints[0, want.frame[0, 1], want.joint[0, 1]], nd.node_obbs[0, 1])
    assert 0 < bound < 1e-13
    with pytest.raises(AssertionError):
        sc.check_contact(want.frame, dist, want, c.joints, nd.node_obbs, nd.count, c.skip_rows)
    frame = want.frame.copy()
    frame[0, nd.count[0]:] = 0                                      # a slot beyond count must hold -1
    if nd.count[0] < frame.shape[1]:
        with pytest.raises(AssertionError):
            sc.check_contact(frame, want.dist, want, c.joints, nd.node_obbs, nd.count, c.skip_rows)


def test_adjacent_only_dedupe_is_caught():
    c = _tie_case()
    want = sc.unique_def(c.joints)
    sc.check_unique(want, want)
    wrong = sc.unique_def(c.joints, adjacent_only=True)
    assert (wrong.count > want.count).all()                         # the distant duplicates stay
    with pytest.raises(AssertionError):
        sc.check_unique(wrong, want)
    z = sc.g15()
    with pytest.raises(AssertionError):
        sc.check_unique(sc.unique_def(z['input_joints'], adjacent_only=True), sc.unique_def(z['input_joints']))


@pytest.mark.parametrize("mutation", [dict(use_mask=False), dict(strict=False)], ids=['no-pred-mask', 'ge-for-gt'])
def test_wrong_keep_rules_are_caught(mutation):
    c = next(c for c in sc.sweep() if c.name.endswith('mixed') and c.obbs.shape[1] >= 24)
    want = sc.nodes_def(c.obbs, c.obj_prob, c.pred_mask, c.pred_cls, c.threshold)
    sc.check_nodes(want, want)
    sc.check_nodes(want, want, sc.RMAT_TOL)
    wrong = sc.nodes_def(c.obbs, c.obj_prob, c.pred_mask, c.pred_cls, c.threshold, **mutation)
    with pytest.raises(AssertionError):
        sc.check_nodes(wrong, want, sc.RMAT_TOL)
    if 'use_mask' in mutation:                                      # G15 has boxes over the threshold that the NMS removed
        z = sc.g15()
        with pytest.raises(AssertionError):
            sc.check_nodes(_g15_nodes(z, use_mask=False), _g15_nodes(z), sc.RMAT_TOL)
