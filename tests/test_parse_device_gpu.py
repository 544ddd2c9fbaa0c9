"""GPU: prediction parsing in one launch (csrc/parse_boxes.hip: p2r_parse_boxes, net_utils/parse_device.py) against the
float64 restatement of its arithmetic (tests/parse_cases.py), against the reference's own results (G14 with the Delaunay
far-box test, G3) and against the tensor path of `ap_helper.parse_predictions` it stands in for.

Masks and classes are compared bit for bit: every case has all its decisions at least MARGIN = 1e-4 from their thresholds
(asserted without a GPU in tests/test_parse_device_cpu.py), and the two sides differ by an ulp of exp / atan2 / cos / sin.
Values meet the tolerances of the existing golden test of the tensor path (tests/test_eval_gpu.py): rtol 1e-5 / atol 1e-6
for corners, rtol 1e-6 / atol 1e-7 for probabilities."""
import functools

import numpy as np
import pytest
import torch

from pose2room_amd import _lib
from pose2room_amd.net_utils import ap_helper, nms, parse_device as pd
from tests import parse_cases as pc
from tests.memguard import run_contract
from tests.test_model_cpu import G
from tests.test_parse_device_cpu import replay_keep

pytestmark = pytest.mark.gpu

CORNERS = dict(rtol=1e-5, atol=1e-6)
PROBS = dict(rtol=1e-6, atol=1e-7)
SWEEP = pc.sweep()


def _kernel(case, dev):
    t = lambda a: None if a is None else torch.from_numpy(a).to(dev)            # noqa: E731
    out = pd.parse_boxes(t(case.center), t(case.size_log), t(case.heading_sc), t(case.objectness), t(case.sem_scores),
                         joints=t(case.joints), cls_in=t(case.cls_in), origin_joint=case.origin_joint,
                         contact_dist=case.contact_dist, remove_far_box=case.remove_far_box, nms_mode=case.nms_mode)
    return out


@functools.lru_cache(maxsize=None)
def _swept(i, dev):
    return _kernel(SWEEP[i], dev), pc.restate_case(SWEEP[i])


def _eval_config(mode=0, far=True, thr=0.1, **over):
    from pose2room_amd.p2rnet import P2RConfig, default_config
    test = {'remove_far_box': far, 'use_3d_nms': mode != 2, 'use_cls_nms': mode == 1, 'nms_iou': thr, **over}
    return P2RConfig(default_config('test', test=test)).eval_config


def _end_points(case, dev):
    ep = {'center': case.center, 'size': case.size_log, 'heading': case.heading_sc, 'objectness_scores': case.objectness,
          'sem_cls_scores': case.sem_scores}
    return ({k: torch.from_numpy(v).to(dev) for k, v in ep.items()},
            {'input_joints': torch.from_numpy(case.joints).to(dev)})


# ---- 1. the sweep against the restatement ----------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(SWEEP)), ids=[c.name for c in SWEEP])
def test_sweep_matches_restatement(dev, i):
    (corners, boxes, obj_prob, pred_cls, nonempty), want = _swept(i, dev)
    case = SWEEP[i]
    N, K = case.center.shape[:2]
    assert corners.shape == (N, K, 8, 3) and corners.dtype == torch.float64
    assert boxes.shape == (N, K, 8 if case.nms_mode == 1 else 7) and boxes.dtype == torch.float64
    assert obj_prob.shape == (N, K) and obj_prob.dtype == torch.float32
    assert pred_cls.shape == (N, K) and pred_cls.dtype == torch.int64
    assert nonempty.shape == (N, K) and nonempty.dtype == torch.uint8
    assert np.array_equal(nonempty.cpu().numpy(), want.nonempty), np.nonzero(nonempty.cpu().numpy() != want.nonempty)
    assert np.array_equal(pred_cls.cpu().numpy(), want.pred_cls)
    np.testing.assert_allclose(corners.cpu().numpy(), want.corners, **CORNERS)
    np.testing.assert_allclose(obj_prob.cpu().numpy(), want.obj_prob, **PROBS)
    b = boxes.cpu().numpy()
    np.testing.assert_allclose(b[..., :6], want.boxes[..., :6], **CORNERS)
    np.testing.assert_allclose(b[..., 6], want.boxes[..., 6], **PROBS)
    if case.nms_mode == 1:
        assert np.array_equal(b[..., 7], want.boxes[..., 7])


@pytest.mark.parametrize("i", range(len(SWEEP)), ids=[c.name for c in SWEEP])
def test_rows_are_the_rows_of_the_tensor_path(dev, i):
    """`boxes` bit for bit what ap_helper builds from the kernel's own corners and probabilities: min / max, torch.cat,
    and boxes_2d_as_3d for the 2-D rows"""
    (corners, boxes, obj_prob, pred_cls, _), _ = _swept(i, dev)
    mins, maxs = corners.min(dim=2).values, corners.max(dim=2).values
    score = obj_prob.to(torch.float64).unsqueeze(-1)
    mode = SWEEP[i].nms_mode
    if mode == 2:
        want = nms.boxes_2d_as_3d(torch.cat([mins[..., 0:1], mins[..., 2:3], maxs[..., 0:1], maxs[..., 2:3], score], -1))
    elif mode == 0:
        want = torch.cat([mins, maxs, score], -1)
    else:
        want = torch.cat([mins, maxs, score, pred_cls.to(torch.float64).unsqueeze(-1)], -1)
    assert boxes.shape == want.shape
    assert torch.equal(boxes.view(torch.int64), want.contiguous().view(torch.int64))


# ---- 2. the reference's results through parse_predictions(impl='kernel') -----------------------------------------------------
@pytest.mark.parametrize("key,mode", [('pred_mask', 0), ('pred_mask_cls', 1), ('pred_mask_2d', 2)])
def test_g14_far_box_filter_and_masks(dev, oracle, key, mode):
    case, z = pc.g14()
    ep, data = _end_points(case, dev)
    cfg = _eval_config(mode, thr=float(z['nms_iou']))
    assert cfg['dataset_config'].contact_dist_thresh == float(z['contact_dist']) and cfg['remove_far_box']
    eval_dict, parsed = ap_helper.parse_predictions(ep, data, cfg, impl='kernel')
    assert eval_dict['pred_mask'].dtype == np.uint8 and np.array_equal(eval_dict['pred_mask'], z[key])
    np.testing.assert_allclose(parsed['pred_corners_3d'], z['pred_corners_3d'], **CORNERS)
    np.testing.assert_allclose(parsed['obj_prob'], z['obj_prob'], **PROBS)
    assert np.array_equal(parsed['pred_sem_cls'], z['pred_sem_cls'])
    # the far-box mask itself (the Delaunay hull test), and the keep mask as the reference's NMS on the kernel's own rows
    _, boxes, _, _, nonempty = _kernel(case._replace(nms_mode=mode), dev)
    assert np.array_equal(nonempty.cpu().numpy(), z['nonempty'])
    assert np.array_equal(replay_keep(oracle, boxes.cpu().numpy(), z['nonempty'], float(z['nms_iou']), mode == 1),
                          eval_dict['pred_mask'])


@pytest.mark.parametrize("tag,B,T", [('g3u', 1, 768), ('g3f', 2, 512)])
def test_g3_keep_masks_by_decisions(dev, oracle, tag, B, T):
    from pose2room_amd.p2rnet.synthetic import make_batch
    from tests.test_eval_gpu import _check_keep_masks
    z = np.load(G)
    cfg = _eval_config(0, far=False, thr=0.10)
    data = make_batch(B, T, seed=100 + T, device=dev)
    ep = {k: torch.from_numpy(z[f'{tag}_{k}']).to(dev)
          for k in ['center', 'size', 'heading', 'objectness_scores', 'sem_cls_scores']}
    eval_dict, parsed = ap_helper.parse_predictions(ep, data, cfg, impl='kernel')
    np.testing.assert_allclose(parsed['pred_corners_3d'], z[f'{tag}_pred_corners_3d'], **CORNERS)
    np.testing.assert_allclose(parsed['obj_prob'], z[f'{tag}_obj_prob'], **PROBS)
    np.testing.assert_allclose(parsed['sem_cls_probs'], z[f'{tag}_sem_cls_probs'], **PROBS)
    assert np.array_equal(parsed['pred_sem_cls'], z[f'{tag}_pred_sem_cls'])
    # (2) of the decision-level check is `oracle.nms_3d` on the kernel's own boxes == the kernel path's keep mask
    _check_keep_masks(oracle, f'parse_predictions(impl=kernel) ({tag})', cfg['nms_iou'],
                      (parsed['pred_corners_3d'], parsed['obj_prob']), (z[f'{tag}_pred_corners_3d'], z[f'{tag}_obj_prob']),
                      eval_dict['pred_mask'], z[f'{tag}_pred_mask'])


# ---- 3. kernel against tensor path ------------------------------------------------------------------------------------------
def _same_results(got, want, device_form):
    for g, w in zip(got, want):
        assert list(g.keys()) == list(w.keys())
        for k in g:
            a, b = g[k], w[k]
            assert type(a) is type(b) and a.dtype == b.dtype and a.shape == b.shape, k
            if device_form:
                assert a.device == b.device, k
                a, b = a.cpu().numpy(), b.cpu().numpy()
            if k in ('pred_mask', 'pred_sem_cls', 'sem_cls_scores'):
                assert np.array_equal(a, b), k
            else:
                np.testing.assert_allclose(a, b, err_msg=k, **(CORNERS if k == 'pred_corners_3d' else PROBS))


@pytest.mark.parametrize("i", range(len(pc.nms_cases())), ids=[c.name for c in pc.nms_cases()])
@pytest.mark.parametrize("return_device", [True, False])
def test_kernel_equals_tensor_path(dev, i, return_device):
    case = pc.nms_cases()[i]
    ep, data = _end_points(case, dev)
    cfg = _eval_config(case.nms_mode)
    want = ap_helper.parse_predictions(ep, data, cfg, return_device=return_device)              # impl: the default
    got = ap_helper.parse_predictions(ep, data, {**cfg, 'parse_impl': 'kernel'}, return_device=return_device)
    _same_results(got, want, return_device)
    mask = got[0]['pred_mask']
    n_kept = int(mask.sum())
    assert 0 < n_kept < int(pc.restate_case(case).nonempty.sum())                               # the NMS suppressed boxes


@pytest.mark.parametrize("return_device", [True, False])
def test_kernel_equals_tensor_path_with_sampled_classes(dev, return_device):
    case = pc.nms_cases()[1]
    ep, data = _end_points(case, dev)
    cfg = _eval_config(1, sample_cls=True)
    torch.manual_seed(5)
    want = ap_helper.parse_predictions(ep, data, cfg, return_device=return_device, impl='torch')
    torch.manual_seed(5)
    got = ap_helper.parse_predictions(ep, data, cfg, return_device=return_device, impl='kernel')
    _same_results(got, want, return_device)
    cls = got[1]['pred_sem_cls']
    cls = cls.cpu().numpy() if return_device else cls
    assert not np.array_equal(cls, case.sem_scores.argmax(-1))                                  # the draw was used


class _Counting:
    def __init__(self, fn):
        self.fn, self.argtypes, self.calls = fn, getattr(fn, 'argtypes', None), 0

    def __call__(self, *args):
        self.calls += 1
        return self.fn(*args)


def test_one_parse_launch_and_one_nms_launch(dev):
    case = pc.nms_cases()[0]
    ep, data = _end_points(case, dev)
    cfg = _eval_config(0)
    libs = (pd.lib(), 'p2r_parse_boxes'), (_lib.lib(), 'p2r_nms3d')
    saved = [getattr(l, n) for l, n in libs]
    counters = [_Counting(f) for f in saved]
    try:
        for (l, n), c in zip(libs, counters):
            setattr(l, n, c)
        pd.parse_predictions_device(ep, data, cfg)
        assert [c.calls for c in counters] == [1, 1]
        ap_helper.parse_predictions(ep, data, cfg, return_device=True)                         # 'torch': not a launch of it
        assert [c.calls for c in counters] == [1, 2]
    finally:
        for (l, n), f in zip(libs, saved):
            setattr(l, n, f)


def test_device_ap_calculator_picks_the_implementation_up(dev, monkeypatch):
    """`DeviceAPCalculator.step_end_points` reaches the kernel through eval_config alone, and the metric is the same"""
    from pose2room_amd.net_utils.ap_device import DeviceAPCalculator
    case = pc.nms_cases()[0]
    ep, data = _end_points(case, dev)
    G = 4                                                   # ground truth: the first proposals, slightly moved
    data.update({'center_label': ep['center'][:, :G] + 0.05, 'size': ep['size'][:, :G].clone(),
                 'heading': ep['heading'][:, :G].clone(), 'sem_cls_label': ep['sem_cls_scores'][:, :G].argmax(-1),
                 'box_label_mask': torch.ones(case.center.shape[0], G, dtype=torch.int64, device=dev)})
    calls = []
    real = pd.parse_boxes
    monkeypatch.setattr(pd, 'parse_boxes', lambda *a, **k: calls.append(1) or real(*a, **k))
    metrics = {}
    for impl in ap_helper.PARSE_IMPLS:
        calc = DeviceAPCalculator([0.25, 0.5], num_class=case.sem_scores.shape[-1])
        calc.step_end_points(ep, data, _eval_config(0, parse_impl=impl))
        metrics[impl] = calc.compute_metrics()
        assert len(calls) == (impl == 'kernel')
    for got, want in zip(metrics['kernel'], metrics['torch']):
        assert list(got) == list(want)
        np.testing.assert_allclose([float(v) for v in got.values()], [float(v) for v in want.values()], rtol=1e-12,
                                   equal_nan=True)
    assert np.isfinite(metrics['torch'][0]['mAP'])


# ---- 4. hypotheses ---------------------------------------------------------------------------------------------------------
def test_hypotheses_read_the_joints_in_place(dev, monkeypatch):
    from tests.test_model_cpu import build
    from pose2room_amd.p2rnet.synthetic import make_batch
    H, B, T = 3, 2, 64
    net, cfg = build('test', T, device=dev)
    net = net.to(dev).eval()
    data = make_batch(B, T, seed=77, device=dev)
    assert cfg.eval_config['parse_impl'] == 'torch' and cfg.eval_config['remove_far_box']
    seen = []
    real = pd.parse_boxes

    def spy(center, *args, joints=None, **kw):
        seen.append((tuple(center.shape), tuple(joints.shape), joints.data_ptr()))
        return real(center, *args, joints=joints, **kw)
    monkeypatch.setattr(pd, 'parse_boxes', spy)
    with torch.no_grad():
        want = net.generate_hypotheses(data, H, n_samples=[5, 40, 99], seed=321, return_device=True)
        assert not seen
        cfg.eval_config['parse_impl'] = 'kernel'
        got = net.generate_hypotheses(data, H, n_samples=[5, 40, 99], seed=321, return_device=True)
        host = net.generate_hypotheses(data, H, n_samples=[5, 40, 99], seed=321)
    K = got['center'].shape[2]
    assert seen == [((H * B, K, 3), tuple(data['input_joints'].shape), data['input_joints'].data_ptr())] * 2
    assert set(got) == set(want)
    for k in ('pred_mask', 'pred_sem_cls'):
        assert got[k].shape == (H, B, K) and got[k].dtype == want[k].dtype
        assert torch.equal(got[k], want[k]), k
    np.testing.assert_allclose(got['pred_corners_3d'].cpu().numpy(), want['pred_corners_3d'].cpu().numpy(), **CORNERS)
    np.testing.assert_allclose(got['obj_prob'].cpu().numpy(), want['obj_prob'].cpu().numpy(), **PROBS)
    for h in range(H):                                                                          # the host lists' form
        assert np.array_equal(host[h][1]['pred_mask'], want['pred_mask'][h].cpu().numpy())
    assert 0 < int(want['pred_mask'].sum()) < H * B * K


# ---- 5. an empty pick --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("impl", ['torch', 'kernel'])
def test_empty_pick_raises(dev, impl):
    case = pc.nms_cases()[0]
    joints = case.joints.copy()
    joints[1] += np.float32(500.0)                                                              # sample 1: every box is far
    ep, data = _end_points(case._replace(joints=joints), dev)
    with pytest.raises(AssertionError, match="NMS kept no box for some sample"):
        ap_helper.parse_predictions(ep, data, _eval_config(0), return_device=True, impl=impl)


# ---- 6. the memory contract --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,with_cls", [(0, False), (1, True), (2, False)])
def test_memory_contract(dev, mode, with_cls):
    """outputs in poisoned, guard-banded buffers at an odd K (a partial group of proposals) and T = one chunk + 1: every
    output element is overwritten, no halo is damaged, the inputs are bit-identical afterwards, and the results do not
    depend on what lies around the inputs"""
    case = pc.make_case('contract', N=3, K=21, T=pc.CHUNK + 1, J=7, origin_joint=2, nms_mode=mode, with_cls=with_cls,
                        seed=4100 + mode)
    want = pc.restate_case(case)
    inputs = {k: torch.from_numpy(getattr(case, k)) for k in ('center', 'size_log', 'heading_sc', 'objectness',
                                                              'sem_scores', 'joints')}
    if with_cls:
        inputs['cls_in'] = torch.from_numpy(case.cls_in)

    def fn(**t):
        return pd.parse_boxes(t['center'], t['size_log'], t['heading_sc'], t['objectness'], t['sem_scores'],
                              joints=t['joints'], cls_in=t.get('cls_in'), origin_joint=case.origin_joint,
                              contact_dist=case.contact_dist, nms_mode=mode)
    got = run_contract(fn, inputs, dev)
    assert np.array_equal(got['out.4'].cpu().numpy(), want.nonempty) and 0 < want.nonempty.sum() < want.nonempty.size
    assert np.array_equal(got['out.3'].cpu().numpy(), want.pred_cls)
    np.testing.assert_allclose(got['out.0'].cpu().numpy(), want.corners, **CORNERS)
