"""Test / evaluation loop: losses + detection AP over a stream of batches.

Mirror of the reference's models/p2rnet/testing.py:16-50 (`Tester.test_step`: generate -> loss ->
rank-averaged scalar dict, returns `(loss_dict, est_data)`) and test_epoch.py:10-76 (`test_func`,
`test`: one `APCalculator` per IoU threshold of `cfg.config[mode]['ap_iou_thresholds']`, fed with
`eval_dict['batch_pred_map_cls' / 'batch_gt_map_cls']` of every batch, loss meters synchronised over
ranks at the end).  Rendering is out of scope; what the dump and the demo compute in front of it -- confident boxes as
object nodes, unique frames, contact frames, the `pred_confident_nms_bbox.npz` layout -- is `P2RNet.predict_scenes`
(net_utils/scene_device.py: SceneBatch.nodes / records / save_npz).
"""
from time import time

import torch
import torch.distributed as dist

from ..net_utils.ap_helper import APCalculator
from .training import Trainer, reduce_dict


class AverageMeter(object):
    """Running average of a scalar (net_utils/utils.py:295-327)."""

    def __init__(self):
        self.val = self.avg = self.sum = self.count = 0

    def update(self, val, n=1):
        self.val = val
        if isinstance(val, list):
            self.sum += sum(val)
            self.count += len(val)
        else:
            self.sum += val * n
            self.count += n
        self.avg = self.sum / self.count

    def synchronize_between_processes(self, device=None):
        if not (dist.is_available() and dist.is_initialized()):
            return
        t = torch.tensor([self.count, self.sum], dtype=torch.float64,
                         device=device if device is not None else ('cuda' if torch.cuda.is_available() else 'cpu'))
        dist.barrier()
        dist.all_reduce(t)
        self.count, self.sum = int(t[0].item()), t[1].item()
        self.avg = self.sum / max(self.count, 1)


class LossRecorder(object):
    """Per-key meters (net_utils/utils.py:329-355)."""

    def __init__(self, batch_size=1):
        self._batch_size = batch_size
        self._loss_recorder = {}

    @property
    def batch_size(self):
        return self._batch_size

    @property
    def loss_recorder(self):
        return self._loss_recorder

    def update_loss(self, loss_dict):
        for key, item in loss_dict.items():
            self._loss_recorder.setdefault(key, AverageMeter()).update(item, self._batch_size)

    def synchronize_between_processes(self, device=None):
        for meter in self._loss_recorder.values():
            meter.synchronize_between_processes(device)


class Tester(Trainer):
    def __init__(self, cfg, net, device=None):
        super().__init__(cfg, net, None, device)

    def test_step(self, data):
        data = self.to_device(data)
        est_data = self.net.module.generate(data)
        loss = self.net.module.loss(est_data, data)
        loss_reduced = reduce_dict(loss)
        return {k: v.item() for k, v in loss_reduced.items()}, est_data


def _check_ap_impl(ap_impl):
    if ap_impl not in ('host', 'device'):
        raise ValueError("ap_impl must be 'host' or 'device', got %r" % (ap_impl,))


def test_func(cfg, tester, batches, ap_device='cpu', ap_impl='host'):
    """batches: any iterable of data dicts (the reference passes `test_loader.dataloader`).
    ap_impl 'host': one `APCalculator` per IoU threshold, fed with the per-scan lists (the reference's loop).
    ap_impl 'device': ONE `ap_device.DeviceAPCalculator` for all thresholds, fed with the end points and the batch on
    the device; `calculators` is then that one calculator in a list."""
    _check_ap_impl(ap_impl)
    mode = cfg.config['mode']
    recorder = LossRecorder(cfg.config[mode]['batch_size'])
    class2type = getattr(cfg.dataset_config, 'class2type', None)
    if ap_impl == 'device':
        from ..net_utils.ap_device import DeviceAPCalculator
        calculators = [DeviceAPCalculator(list(cfg.config[mode]['ap_iou_thresholds']), class2type,
                                          num_class=cfg.dataset_config.num_class,
                                          per_class_proposal=cfg.eval_config['per_class_proposal'],
                                          conf_thresh=cfg.eval_config['conf_thresh'])]
    else:
        calculators = [APCalculator(thr, class2type, False, device=ap_device) for thr in cfg.config[mode]['ap_iou_thresholds']]
    for data in batches:
        loss, est_data = tester.test_step(data)
        if ap_impl == 'device':
            calculators[0].step_end_points(est_data[0], data, cfg.eval_config)     # test_step moved `data` to the device
        else:
            eval_dict = est_data[1]
            for calc in calculators:
                calc.step(eval_dict['batch_pred_map_cls'], eval_dict['batch_gt_map_cls'])
        recorder.update_loss(loss)
    recorder.synchronize_between_processes(tester.device)
    return recorder.loss_recorder, calculators


def test(cfg, tester, batches, ap_device='cpu', ap_impl='host'):
    """test_epoch.py:52-76 -> {'loss': {key: avg}, 'metrics': [{...} per IoU threshold]}; also logged.
    ap_impl: 'host' (default) or 'device', see `test_func`; the result has the same shape either way."""
    mode = cfg.config['mode']
    tester.net.train(mode == 'train')
    start = time()
    with torch.no_grad():
        meters, calculators = test_func(cfg, tester, batches, ap_device, ap_impl)
    cfg.log_string('Test time elapsed: (%f).' % (time() - start))
    out = {'loss': {k: m.avg for k, m in meters.items()}, 'metrics': []}
    for key, avg in out['loss'].items():
        cfg.log_string('Test loss (%s): %f' % (key, avg))
    all_metrics = calculators[0].compute_metrics() if ap_impl == 'device' else [c.compute_metrics() for c in calculators]
    for thr, metrics in zip(cfg.config[mode]['ap_iou_thresholds'], all_metrics):
        cfg.log_string(('-' * 10 + 'iou_thresh: %f' + '-' * 10) % thr)
        for key in metrics:
            cfg.log_string('eval %s: %f' % (key, metrics[key]))
        out['metrics'].append(metrics)
    return out


def test_multi_modal(cfg, net, batches, num_hypotheses, n_samples=None, seed=None, ap_device='cpu',
                     dump_threshold=0.5, central_tendency=None, impl='host'):
    """Multi-modal evaluation: what `num_hypotheses` reference test runs in multi mode plus
    utils/eval/multi_modal_eval.py produce, from one trunk pass per batch (`P2RNet.generate_hypotheses`).
    Hypothesis h plays run h: its sample counts n_h are fixed for all batches (drawn once from `seed` when None, as
    the reference draws one count per run), one `APCalculator` per IoU threshold collects its detections, and its
    confident boxes (dump_threshold: the reference's generation.dump_threshold) are its dump records.
    net: P2RNet (or a wrapper exposing it as `.module`).  central_tendency: None (the heads' own), 'mean' or 'median'.
    impl 'host': the reference's evaluation, H x T `APCalculator`s (on `ap_device`) and the NumPy records and TMD.
    impl 'device': `generate_hypotheses(return_device=True)` into ONE `mm_device.DeviceMultiModalEvaluator`, fed with
    the batch on the device (`ap_device` does not apply); the result has the same keys and the same log lines.
    -> {'best_map': (T,) max over hypotheses of each threshold's mAP, 'tmd': mean TMD over every (sample, proposal),
        'metrics': [h][t] metric dicts, 'n_samples': [n_h], 'seed': the 64-bit seed,
        'central_tendency': as passed}."""
    from ..net_utils import multi_modal_eval as mm
    from .mdn_sample_op import resolve_draws
    if impl not in ('host', 'device'):
        raise ValueError("impl must be 'host' or 'device', got %r" % (impl,))
    model = getattr(net, 'module', net)
    seed, ns = resolve_draws(num_hypotheses, n_samples, seed)
    H = len(ns)
    thresholds = cfg.config[cfg.config['mode']]['ap_iou_thresholds']
    if impl == 'device':
        metrics, best, t = _multi_modal_device(cfg, model, batches, H, ns, seed, thresholds, dump_threshold,
                                               central_tendency)
        return _multi_modal_result(cfg, H, thresholds, metrics, best, t, ns, seed, central_tendency)
    calcs = [[APCalculator(thr, getattr(cfg.dataset_config, 'class2type', None), False, device=ap_device)
              for thr in thresholds] for _ in range(H)]
    records = [[] for _ in range(H)]
    model.train(False)
    with torch.no_grad():
        for i, data in enumerate(batches):
            batch_seed = (seed + i * 0x9E3779B97F4A7C15) & 0xffffffffffffffff     # one stream key per batch
            for h, (ep, eval_dict, parsed) in enumerate(model.generate_hypotheses(
                    data, H, ns, batch_seed, eval=True, central_tendency=central_tendency)):
                for calc in calcs[h]:
                    calc.step(eval_dict['batch_pred_map_cls'], eval_dict['batch_gt_map_cls'])
                records[h] += mm.confident_boxes(ep, eval_dict, parsed, dump_threshold)
    metrics = [[c.compute_metrics() for c in row] for row in calcs]
    best = mm.best_of_n_map([[m['mAP'] for m in row] for row in metrics])
    return _multi_modal_result(cfg, H, thresholds, metrics, best, mm.tmd(records), ns, seed, central_tendency)


def _multi_modal_result(cfg, H, thresholds, metrics, best, t, ns, seed, central_tendency):
    for thr, v in zip(thresholds, best):
        cfg.log_string('multi-modal (%d hypotheses) iou_thresh %f: best mAP %f' % (H, thr, v))
    cfg.log_string('multi-modal TMD: %f' % t)
    return {'best_map': best, 'tmd': t, 'metrics': metrics, 'n_samples': ns, 'seed': seed,
            'central_tendency': central_tendency}


def _multi_modal_device(cfg, model, batches, H, ns, seed, thresholds, dump_threshold, central_tendency):
    """`test_multi_modal(impl='device')`: -> (metrics [h][t], best_map (T,), tmd); the batches must be on the device"""
    from ..net_utils.ap_helper import boxes_to_corners
    from ..net_utils.mm_device import DeviceMultiModalEvaluator
    ev = DeviceMultiModalEvaluator(H, list(thresholds), getattr(cfg.dataset_config, 'class2type', None),
                                   num_class=cfg.dataset_config.num_class,
                                   per_class_proposal=cfg.eval_config['per_class_proposal'],
                                   conf_thresh=cfg.eval_config['conf_thresh'], dump_threshold=dump_threshold)
    model.train(False)
    with torch.no_grad():
        for i, data in enumerate(batches):
            batch_seed = (seed + i * 0x9E3779B97F4A7C15) & 0xffffffffffffffff     # one stream key per batch
            hyp = model.generate_hypotheses(data, H, ns, batch_seed, central_tendency=central_tendency,
                                            return_device=True)
            mask = data['box_label_mask'].detach()                                # as DeviceAPCalculator.step_end_points
            gt_heading = torch.atan2(data['heading'][..., 0], data['heading'][..., 1]).detach()
            corners = boxes_to_corners(torch.exp(data['size']).detach(), gt_heading.to(torch.float64),
                                       data['center_label'][:, :, 0:3].detach())
            corners = corners * (mask != 0).to(torch.float64)[:, :, None, None]
            ev.step_tensors(hyp['pred_corners_3d'], hyp['pred_mask'], hyp['obj_prob'], hyp['sem_cls_scores'],
                            hyp['pred_sem_cls'], corners, data['sem_cls_label'].detach(), mask)
    res = ev.compute()
    return res['metrics'], res['best_map'], res['tmd']
