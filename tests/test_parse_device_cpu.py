"""CPU: the contract of prediction parsing on the device (csrc/parse_boxes.hip, net_utils/parse_device.py) before any
kernel is involved: the ABI of include/p2r_parse.h / libp2r_parse.so, the float64 restatement (tests/parse_cases.py)
against the reference's own results (G14 with the Delaunay far-box test, G3), the margins of every generated case, the
argument checks of the entry point, which return on the host before any launch, and the `parse_impl` switch."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from pose2room_amd import _lib
from pose2room_amd.net_utils import parse_device as pd
from tests import parse_cases as pc
from tests.test_model_cpu import G

EINVAL = -22


# ---- 1. the ABI ----------------------------------------------------------------------------------------------------------
def test_header_binds_and_library_exports_exactly_it():
    from pose2room_amd.net_utils import ap_device, mm_device, vote_labels
    protos = _lib.prototypes(pd.HEADER_PATH)
    assert sorted(protos) == _lib.declared_symbols(pd.HEADER_PATH) == ['p2r_parse_boxes']
    p = protos['p2r_parse_boxes']
    assert p.has_stream and p.kinds == 'ppppppp' + 'iiiiiii' + 'f' + 'ii' + 'ppppp'
    assert p.argtypes[14] is ctypes.c_double and p.restype is ctypes.c_int
    for other in (None, ap_device.HEADER_PATH, mm_device.HEADER_PATH, vote_labels.HEADER_PATH):
        assert not set(protos) & set(_lib.declared_symbols(*([other] if other else [])))
    out = subprocess.run(["nm", "-D", "--defined-only", pd.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if " T " in ln and ln.split()[-1].startswith("p2r_")}
    assert exported == set(protos)
    fn = pd.lib().p2r_parse_boxes
    assert fn.argtypes == p.argtypes and fn.restype is ctypes.c_int
    assert os.path.basename(pd.LIB_PATH) == 'libp2r_parse.so'


def test_libp2r_hip_still_exports_exactly_its_header():
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if " T " in ln and ln.split()[-1].startswith("p2r_")}
    assert exported == set(_lib.declared_symbols()) and 'p2r_parse_boxes' not in exported
    assert _lib.lib().p2r_abi_version() == 3


# ---- 2. the restatement against the reference ----------------------------------------------------------------------------
def test_restatement_reproduces_g14():
    case, z = pc.g14()
    assert case.center.shape == (3, 24, 3) and case.joints.shape[1] == 40
    r = pc.restate_case(case)
    assert np.array_equal(r.nonempty, z['nonempty'])                        # the Delaunay hull test, bit for bit
    assert r.nonempty.sum(1).min() >= 1 and (r.nonempty == 0).sum(1).min() >= 1          # near and far boxes everywhere
    np.testing.assert_allclose(r.corners, z['pred_corners_3d'], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(r.obj_prob, z['obj_prob'], rtol=1e-6, atol=1e-7)
    assert np.array_equal(r.pred_cls, z['pred_sem_cls'])
    # rotated boxes: headings off the axes in every sample
    theta = np.arctan2(case.heading_sc[..., 0], case.heading_sc[..., 1])
    assert (np.abs(np.sin(2 * theta)) > 0.1).sum(1).min() >= 8


@pytest.mark.parametrize("key,mode", [('pred_mask', 0), ('pred_mask_cls', 1), ('pred_mask_2d', 2)])
def test_g14_keep_masks_replay_with_clear_decisions(oracle, key, mode):
    """the reference's keep mask is the oracle's NMS on the restated rows of the restated near boxes, and every decision
    it is made of is at least MARGIN from flipping"""
    case, z = pc.g14()
    thr = float(z['nms_iou'])
    r = pc.restate_case(case._replace(nms_mode=mode))
    gap, over = pc.nms_margins(r.boxes, r.nonempty, thr, mode == 1)
    assert min(r.far_margin.min(), r.size_margin.min(), gap, over) >= pc.MARGIN
    assert np.array_equal(replay_keep(oracle, r.boxes, r.nonempty, thr, mode == 1), z[key])
    assert (z[key].sum(1) >= 1).all() and z['pred_mask'].sum() < z['nonempty'].sum()     # the NMS did suppress something


def replay_keep(oracle, boxes, nonempty, thr, same_cls=False):
    """the reference's mask construction (ap_helper.py:216-251) on rows of p2r_nms3d: the oracle's NMS (pinned bit for
    bit to net_utils/nms.py by G2) among the near boxes; with same_cls only boxes of one class suppress each other,
    which is the NMS of every class by itself"""
    keep = np.zeros(nonempty.shape, np.uint8)
    for i, (b, ne) in enumerate(zip(boxes, nonempty)):
        inds = np.nonzero(ne)[0]
        groups = [inds] if not same_cls else [inds[b[inds, 7] == c] for c in np.unique(b[inds, 7])]
        for g in groups:
            pick = oracle.nms_3d(np.ascontiguousarray(b[g, :7]), thr, False)
            keep[i, g[pick]] = 1
    return keep


@pytest.mark.parametrize("tag", ['g3u', 'g3f'])
def test_restatement_reproduces_g3(tag):
    z = np.load(G)
    r = pc.restate(z[f'{tag}_center'], z[f'{tag}_size'], z[f'{tag}_heading'], z[f'{tag}_objectness_scores'],
                   z[f'{tag}_sem_cls_scores'], remove_far_box=False)
    np.testing.assert_allclose(r.corners, z[f'{tag}_pred_corners_3d'], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(r.obj_prob, z[f'{tag}_obj_prob'], rtol=1e-6, atol=1e-7)
    assert np.array_equal(r.pred_cls, z[f'{tag}_pred_sem_cls'])
    assert r.nonempty.all() and r.boxes.shape[-1] == 7


def test_restatement_rows_and_first_maximum():
    case = pc.sweep()[1]
    rows = {m: pc.restate_case(case._replace(nms_mode=m)) for m in (0, 1, 2)}
    mins, maxs = rows[0].corners.min(2), rows[0].corners.max(2)
    score = rows[0].obj_prob.astype(np.float64)
    assert np.array_equal(rows[0].boxes, np.concatenate([mins, maxs, score[..., None]], -1))
    assert np.array_equal(rows[1].boxes[..., :7], rows[0].boxes) and np.array_equal(rows[1].boxes[..., 7], rows[1].pred_cls)
    assert np.array_equal(rows[2].boxes[..., [0, 2, 3, 5, 6]], rows[0].boxes[..., [0, 2, 3, 5, 6]])
    assert (rows[2].boxes[..., 1] == 0).all() and (rows[2].boxes[..., 4] == 1).all()
    assert (rows[0].pred_cls[:, 0] == 1).all() and (rows[0].pred_cls[:, 2] == 0).all()   # ties: the first maximum


# ---- 3. the generated cases ----------------------------------------------------------------------------------------------
def test_every_generated_case_has_clear_decisions():
    assert pc.CHUNK == pd.CHUNK_FRAMES and pc.MARGIN == 1e-4
    cases = pc.sweep()
    for case in cases + pc.nms_cases():
        r = pc.restate_case(case)
        assert r.far_margin.min() >= pc.MARGIN and r.size_margin.min() >= pc.MARGIN, case.name
    for case in pc.nms_cases():
        assert pc.nms_decisions_clear(case, margin=pc.MARGIN), case.name


def test_sweep_covers_what_it_claims():
    cases = pc.sweep()
    shape = lambda c: (c.center.shape[0], c.center.shape[1], c.joints.shape[1])             # noqa: E731
    assert {shape(c)[2] for c in cases} == set(pc.SWEEP_T) == {1, 63, 64, 65, 256, 257, 513}
    assert {shape(c)[1] for c in cases} == {1, 5, 128, 130}
    assert {(shape(c)[0], shape(c)[0] // c.joints.shape[0]) for c in cases} == {(1, 1), (3, 1), (3, 3)}
    assert {(c.nms_mode, shape(c)[0] // c.joints.shape[0]) for c in cases} == {(m, r) for m in (0, 1, 2) for r in (1, 3)}
    assert {c.cls_in is None for c in cases} == {True, False} and {c.remove_far_box for c in cases} == {True, False}
    assert {c.joints.shape[2] for c in cases} == {1, 7, 53}
    lone = set()                        # (frame of the only inside hip, T) over the boxes with exactly one
    none, edge, axis = 0, set(), set()
    for c in cases:
        if not c.remove_far_box:
            continue
        r = pc.restate_case(c)
        N, K, T = shape(c)
        lone |= {(int(f), T) for f in r.first_inside[(r.n_inside == 1) & (r.nonempty == 1)]}
        none += int(not r.nonempty.any())
        size = np.exp(c.size_log)
        edge |= {(bool(v)) for v in ((size < 0.01).any(), (size > 10).any())}
        edge_in = ((size > 0.01) & (size < 0.0104)).any() and ((size < 10) & (size > 9.999)).any()
        axis |= {tuple(h) for h in c.heading_sc.reshape(-1, 2).tolist() if tuple(h) in pc._AXIS_HEADINGS}
        if K >= 5:
            assert edge_in and (size < 0.01).any() and (size > 10).any(), c.name
    assert {(0, 513), (256, 513), (512, 513), (256, 257), (64, 65)} <= lone, sorted(lone)
    assert none >= 3 and len(axis) == 4                   # (0,-1) and (-0,-1) compare equal: +pi and -pi are both drawn
    assert any(np.signbit(c.heading_sc[..., 0][c.heading_sc[..., 1] == -1]).any() for c in cases)


# ---- 4. argument checks: on the host, before any launch ------------------------------------------------------------------
_BUF = ctypes.create_string_buffer(64)          # a non-NULL address; never read, every call below is refused first
_P = ctypes.addressof(_BUF)


def test_parse_boxes_refuses_bad_arguments():
    fn = pd.lib().p2r_parse_boxes
    good = dict(center=_P, size_log=_P, heading_sc=_P, objectness=_P, sem_scores=_P, cls_in=None, joints=_P, N=2, K=5,
                C=4, Bj=2, T=8, J=53, origin_joint=0, contact_dist=1.0, remove_far_box=1, nms_mode=0, corners=_P,
                boxes=_P, obj_prob=_P, pred_cls=_P, nonempty=_P)

    def call(**over):
        return fn(*{**good, **over}.values(), None)
    for bad in (dict(center=None), dict(size_log=None), dict(heading_sc=None), dict(objectness=None),
                dict(sem_scores=None), dict(joints=None), dict(corners=None), dict(boxes=None), dict(obj_prob=None),
                dict(pred_cls=None), dict(nonempty=None), dict(N=0), dict(N=-1), dict(K=0), dict(K=-4), dict(C=0),
                dict(Bj=0), dict(T=0), dict(T=-1), dict(J=0), dict(origin_joint=-1), dict(origin_joint=53),
                dict(nms_mode=-1), dict(nms_mode=3), dict(N=1 << 30, K=1 << 10), dict(Bj=1 << 20, T=1 << 20, J=53)):
        assert call(**bad) == EINVAL, bad


def test_python_layer_refuses_cpu_tensors_and_bad_shapes():
    import torch
    c = pc.sweep()[1]
    t = {k: torch.from_numpy(getattr(c, k)) for k in ('center', 'size_log', 'heading_sc', 'objectness', 'sem_scores')}
    with pytest.raises(RuntimeError, match="GPU tensor"):
        pd.parse_boxes(**t, joints=torch.from_numpy(c.joints))
    with pytest.raises(ValueError, match="nms_mode"):
        pd.parse_boxes(**t, joints=torch.from_numpy(c.joints), nms_mode=3)
    with pytest.raises(ValueError, match=r"center must be \(N,K,3\)"):
        pd.parse_boxes(**{**t, 'center': t['center'][..., :2]}, joints=None, remove_far_box=False)


# ---- 5. the switch -------------------------------------------------------------------------------------------------------
def test_parse_impl_default_and_rejection():
    from pose2room_amd.net_utils import ap_helper
    from pose2room_amd.p2rnet import P2RConfig, default_config
    assert default_config('test')['test']['parse_impl'] == 'torch'
    assert P2RConfig(default_config('test')).eval_config['parse_impl'] == 'torch'
    assert P2RConfig(default_config('test', test={'parse_impl': 'kernel'})).eval_config['parse_impl'] == 'kernel'
    legacy = default_config('test')
    del legacy['test']['parse_impl']                                        # a config written before the key existed
    assert P2RConfig(legacy).eval_config['parse_impl'] == 'torch'
    with pytest.raises(ValueError, match="parse_impl"):
        P2RConfig(default_config('test', test={'parse_impl': 'triton'}))
    cfg = P2RConfig(default_config('test')).eval_config
    with pytest.raises(ValueError, match="impl must be one of"):
        ap_helper.parse_predictions({}, {}, cfg, impl='eager')
    with pytest.raises(ValueError, match="impl must be one of"):
        ap_helper.parse_predictions({}, {}, {**cfg, 'parse_impl': 'hip'})
    assert ap_helper.PARSE_IMPLS == ('torch', 'kernel')
