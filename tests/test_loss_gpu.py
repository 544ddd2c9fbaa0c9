"""GPU: the fused detection loss (csrc/det_loss.hip) against the same loss composed of torch ops around the HIP
nn_distance (BoxNetDetectionLoss.composed -- itself pinned to the reference by the G4 / G4e fixtures): the ten
loss-dict entries with their dtypes, and the gradients of the six differentiable inputs."""
import numpy as np
import pytest
import torch

from tests.cases import det_loss_scene as _scene

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("B,S,K,T,case", [(2, 512, 128, 64, 'near'), (3, 100, 37, 16, 'random'), (2, 64, 128, 32, 'none'),
                                          (2, 300, 128, 40, 'ties'), (1, 512, 128, 8, 'single'), (32, 512, 128, 64, 'near')])
def test_fused_detection_loss(dev, B, S, K, T, case):
    from pose2room_amd.p2rnet import P2RConfig, default_config
    from pose2room_amd.p2rnet.loss import BoxNetDetectionLoss
    cfg = P2RConfig(default_config('train', data={'num_frames': T}), device=dev)
    loss_fn = BoxNetDetectionLoss(1, dev, cfg)
    est, gt = _scene(B, S, K, T, seed=B * 1000 + K + T, case=case)
    gt = {k: v.to(dev) for k, v in gt.items()}
    diff = ['vote_xyz', 'center', 'size', 'heading', 'objectness_scores', 'sem_cls_scores']

    def run(fused):
        e = {k: v.clone().to(dev) for k, v in est.items()}
        for k in diff:
            e[k].requires_grad_(True)
        out = loss_fn(e, gt, None) if fused else loss_fn.composed(e, gt, None)
        out['total'].backward()
        return out, {k: e[k].grad for k in diff}

    want, gw = run(False)
    got, gg = run(True)
    assert list(got.keys()) == list(want.keys())
    for k in want:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (k, got[k].dtype, want[k].dtype)
        np.testing.assert_allclose(got[k].item(), want[k].item(), rtol=2e-5, atol=1e-6, err_msg=k)
    if case == 'none':
        assert got['pos_ratio'].item() == 0 and got['size_loss'].item() == 0
    else:
        assert got['pos_ratio'].item() > 0
    for k in diff:
        assert gg[k].dtype == gw[k].dtype
        scale = max(gw[k].abs().max().item(), 1e-12)
        err = (gg[k] - gw[k]).abs().max().item()
        assert err <= 2e-5 * scale, f'{k}: {err:.3e} vs scale {scale:.3e}'


def test_fused_detection_loss_component_gradients(dev):
    """Gradients requested for individual dict entries (not only `total`) arrive with their own weights."""
    from pose2room_amd.p2rnet import P2RConfig, default_config
    from pose2room_amd.p2rnet.loss import BoxNetDetectionLoss
    cfg = P2RConfig(default_config('train', data={'num_frames': 32}), device=dev)
    loss_fn = BoxNetDetectionLoss(1, dev, cfg)
    est, gt = _scene(2, 128, 64, 32, seed=5, case='near')
    gt = {k: v.to(dev) for k, v in gt.items()}

    def run(fused):
        e = {k: v.clone().to(dev) for k, v in est.items()}
        for k in ('center', 'heading', 'size'):
            e[k].requires_grad_(True)
        out = loss_fn(e, gt, None) if fused else loss_fn.composed(e, gt, None)
        (0.5 * out['center_loss'] + 3.0 * out['heading_loss'] + out['total']).backward()
        return e
    a, b = run(True), run(False)
    for k in ('center', 'heading', 'size'):
        torch.testing.assert_close(a[k].grad, b[k].grad, rtol=2e-5, atol=1e-7)


def test_fused_loss_dispatch_falls_back(dev):
    """Inputs the fused kernel cannot read as they are (float64 ground-truth boxes, more than 32 ground-truth slots)
    take the composed form instead of being misread or raising (advisor finding, round 2)."""
    from pose2room_amd.p2rnet import P2RConfig, default_config
    from pose2room_amd.p2rnet import loss as L
    cfg = P2RConfig(default_config('train', data={'num_frames': 16}), device=dev)
    loss_fn = L.BoxNetDetectionLoss(1, dev, cfg)
    est, gt = _scene(2, 64, 32, 16, seed=5, case='near')
    est = {k: v.to(dev) for k, v in est.items()}
    gt = {k: v.to(dev) for k, v in gt.items()}
    assert L.fused_supported(est, gt)
    want = loss_fn.composed(est, gt, None)
    gt64 = dict(gt, center_label=gt['center_label'].double())
    assert not L.fused_supported(est, gt64)
    got = loss_fn(est, gt64, None)                       # cast to the kernel's dtypes first, not misread
    np.testing.assert_allclose(got['total'].item(), want['total'].item(), rtol=1e-5)
    half = dict(est, center=est['center'].half())
    assert not L.fused_supported(half, gt)
    got = loss_fn(half, gt, None)
    assert got['center_loss'].dtype == torch.float32 and torch.isfinite(got['total'])
    # 40 ground-truth slots (8 more than the kernel's table): composed form, same value as 10 slots + padding
    pad = lambda t: torch.cat([t, torch.zeros(t.shape[0], 30, *t.shape[2:], dtype=t.dtype, device=dev)], 1)
    gt40 = dict(gt, **{k: pad(gt[k]) for k in ('center_label', 'box_label_mask', 'size', 'heading', 'sem_cls_label')})
    assert not L.fused_supported(est, gt40)
    got = loss_fn(est, gt40, None)
    for k in ('vote_loss', 'objectness_loss', 'size_loss', 'heading_loss', 'sem_cls_loss'):
        np.testing.assert_allclose(got[k].item(), want[k].item(), rtol=1e-5, err_msg=k)
