#!/usr/bin/env python3
"""Stand-alone measurement (not bench.py): the detection metric of an evaluation run, host calculator against device
calculator, on an MI355X.

Workload: `--batches` batches of `--bs` scans with `--K` proposals, `--G` ground-truth slots (the loader's
max_gt_boxes), the data set's class count and the IoU thresholds [0.25, 0.5]; end points and batches are resident on
the device before anything is timed (seeded, jittered copies of the ground truths, so that matches happen).

  host    parse_predictions + assembly_pred_map_cls + parse_groundtruths + assembly_gt_map_cls + APCalculator.step
          (one calculator per threshold) over all batches, then compute_metrics once per threshold
  device  DeviceAPCalculator.step_end_points over all batches, then ONE compute_metrics
  kernels p2r_obb_iou and p2r_ap_match alone on one batch's tensors: device events around `--kernel-iters`
          back-to-back launches (launch overhead included)

Both paths are warmed up once and then timed alternately `--repeats` times with a host clock around work that ends in
a device synchronise; every repeat is printed, the summary is one JSON line.  Needs a GPU: there is no fallback.

    python tools/ap_eval_timing.py [--out FILE.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from pose2room_amd.net_utils import ap_device, ap_helper      # noqa: E402
from pose2room_amd.p2rnet import P2RConfig, default_config      # noqa: E402


def make_batch(rng, bs, K, G, C, dev):
    n_gt = rng.integers(1, G + 1, bs)
    mask = (np.arange(G)[None] < n_gt[:, None]).astype(np.int64)
    gsize, gcen = np.log(rng.uniform(0.4, 2.0, (bs, G, 3))), rng.uniform(-3, 3, (bs, G, 3))
    ghead = rng.uniform(-np.pi, np.pi, (bs, G))
    src = rng.integers(0, n_gt[:, None], (bs, K))
    take = lambda a: np.take_along_axis(a, src.reshape(bs, K, *([1] * (a.ndim - 2))), 1)      # noqa: E731
    cen, size = take(gcen) + rng.normal(0, 0.25, (bs, K, 3)), take(gsize) + rng.normal(0, 0.2, (bs, K, 3))
    head = take(ghead) + rng.normal(0, 0.3, (bs, K))
    f32 = lambda a: torch.from_numpy(a.astype(np.float32)).to(dev)                            # noqa: E731
    sc = lambda h: torch.from_numpy(np.stack([np.sin(h), np.cos(h)], -1)).to(dev)             # noqa: E731
    est = {'center': f32(cen), 'size': f32(size), 'heading': sc(head),
           'objectness_scores': f32(rng.normal(0, 2, (bs, K, 2))), 'sem_cls_scores': f32(rng.normal(0, 2, (bs, K, C)))}
    data = {'center_label': f32(gcen), 'size': f32(gsize), 'heading': sc(ghead), 'box_label_mask': torch.from_numpy(mask).to(dev),
            'sem_cls_label': torch.from_numpy(rng.integers(0, C, (bs, G))).to(dev)}
    return est, data


def host_path(batches, cfg, thresholds, class2type):
    calcs = [ap_helper.APCalculator(t, class2type, False) for t in thresholds]
    for est, data in batches:
        eval_dict, parsed = ap_helper.parse_predictions(est, data, cfg)
        eval_dict = ap_helper.assembly_pred_map_cls(eval_dict, parsed, cfg)
        gts = ap_helper.assembly_gt_map_cls(ap_helper.parse_groundtruths(data, cfg))
        for c in calcs:
            c.step(eval_dict['batch_pred_map_cls'], gts)
    return [c.compute_metrics() for c in calcs]


def device_path(batches, cfg, thresholds, class2type):
    calc = ap_device.DeviceAPCalculator(thresholds, class2type, num_class=cfg['dataset_config'].num_class,
                                        per_class_proposal=cfg['per_class_proposal'], conf_thresh=cfg['conf_thresh'])
    for est, data in batches:
        calc.step_end_points(est, data, cfg)
    return calc.compute_metrics()


def timed(fn, dev):
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize(dev)
    return time.perf_counter() - t0, out


def kernel_times(est, data, cfg, thresholds, iters, dev):
    eval_dict, parsed = ap_helper.parse_predictions(est, data, cfg, return_device=True)
    gt = ap_helper.boxes_to_corners(torch.exp(data['size']), torch.atan2(data['heading'][..., 0], data['heading'][..., 1]),
                                    data['center_label'])
    det = parsed['pred_corners_3d'].contiguous()
    B, K, C = parsed['sem_cls_scores'].shape
    score = torch.softmax(parsed['sem_cls_scores'], -1) * parsed['obj_prob'][..., None]
    valid = (eval_dict['pred_mask'] == 1)[..., None].expand(B, K, C).to(torch.uint8).contiguous()
    thr = torch.tensor(thresholds, dtype=torch.float64, device=dev)
    gt_cls, gt_mask = data['sem_cls_label'], (data['box_label_mask'] == 1).to(torch.uint8)
    iou3d, _ = ap_device.obb_iou(det, gt, want_2d=False)
    launches = {'p2r_obb_iou': lambda: ap_device.obb_iou(det, gt, want_2d=False),
                'p2r_ap_match': lambda: ap_device.ap_match(iou3d, score, valid, gt_cls, gt_mask, thr)}
    out = {}
    for name, fn in launches.items():
        for _ in range(5):
            fn()
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize(dev)
        start.record()
        for _ in range(iters):
            fn()
        stop.record()
        torch.cuda.synchronize(dev)
        out[name + '_us'] = start.elapsed_time(stop) * 1e3 / iters
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--batches', type=int, default=16)
    ap.add_argument('--bs', type=int, default=32)
    ap.add_argument('--K', type=int, default=128)
    ap.add_argument('--G', type=int, default=None, help="ground-truth slots (default: the configuration's max_gt_boxes)")
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--kernel-iters', type=int, default=200)
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("ap_eval_timing: needs a GPU (a CPU timing says nothing about the device path)")
    dev = torch.device('cuda:0')
    pc = P2RConfig(default_config('test', test={'remove_far_box': False}), device=dev)
    cfg, thresholds = pc.eval_config, list(pc.config['test']['ap_iou_thresholds'])
    G = a.G or pc.config['data']['max_gt_boxes']
    C = pc.dataset_config.num_class
    class2type = getattr(pc.dataset_config, 'class2type', None)
    rng = np.random.default_rng(a.seed)
    batches = [make_batch(rng, a.bs, a.K, G, C, dev) for _ in range(a.batches)]

    paths = {'host': host_path, 'device': device_path}
    results = {k: timed(lambda f=f: f(batches, cfg, thresholds, class2type), dev)[1] for k, f in paths.items()}     # warm-up
    gap = max(abs(float(h[k]) - float(d[k])) for h, d in zip(results['host'], results['device']) for k in h
              if not (np.isnan(h[k]) and np.isnan(d[k])))
    times = {k: [] for k in paths}
    for r in range(a.repeats):
        for k, f in paths.items():
            times[k].append(timed(lambda f=f: f(batches, cfg, thresholds, class2type), dev)[0])
            print(f"repeat {r} {k}: {times[k][-1] * 1e3:.1f} ms", flush=True)
    summary = {'workload': {'batches': a.batches, 'bs': a.bs, 'K': a.K, 'G': G, 'C': C, 'thresholds': thresholds},
               'host_ms': [round(t * 1e3, 2) for t in times['host']], 'device_ms': [round(t * 1e3, 2) for t in times['device']],
               'host_ms_median': round(float(np.median(times['host'])) * 1e3, 2),
               'device_ms_median': round(float(np.median(times['device'])) * 1e3, 2),
               'mAP': [float(m['mAP']) for m in results['device']], 'max_metric_gap_host_vs_device': gap,
               'kernels': {k: round(v, 2) for k, v in kernel_times(*batches[0], cfg, thresholds, a.kernel_iters, dev).items()}}
    line = json.dumps(summary)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
