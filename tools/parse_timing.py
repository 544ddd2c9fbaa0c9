#!/usr/bin/env python3
"""Stand-alone measurement (not bench.py): prediction parsing with the far-box filter ON, tensor path against kernel
path, on an MI355X.

`parse_predictions(..., return_device=True)` -- heads to NMS keep mask -- under `impl='torch'` (ap_helper.py: ATen
launches in float64, three (N,K,T,3) intermediates for the far-box filter) and `impl='kernel'` (parse_device.py: one
p2r_parse_boxes launch and the p2r_nms3d launch), with `remove_far_box: True`, the configured default that the other
timing tools switch off.  Inputs are resident before anything is timed: per sample a hip track of T frames among 53
joints that walks through a room, and K proposals of which `--near` are drawn around the track (they pass the filter, the
first chunk of frames usually decides) and the rest across a wider floor (most of them fail it after a full scan).

Shapes: bs x T x K = 32 x 1024 x 128; the stacked H * bs = 320 samples of `generate_hypotheses` at H = 10 (tensor path:
the joints expanded H-fold as network.py does it, timed with and without that copy; kernel path: the batch's joints read
in place with joints_repeat = H); and 32 x 2048 x 128.

Per shape and path: the results are compared first (masks, classes, corners), both are warmed up, then timed alternately
`--repeats` times, `--iters` calls each, with a host clock around work that ends in a device synchronise; the peak of
`torch.cuda.max_memory_allocated` above the resident inputs is taken in a call of its own.  The two launches of the kernel
path are also timed alone with device events.  Every repeat is printed, the summary is one JSON line.  Needs a GPU.

    python tools/parse_timing.py [--out FILE.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from pose2room_amd.net_utils import ap_helper, nms, parse_device      # noqa: E402
from pose2room_amd.p2rnet import P2RConfig, default_config              # noqa: E402


def make_inputs(rng, bs, T, K, C, near, dev, H=1):
    """-> (end points of H * bs samples, hypothesis-major; joints (bs,T,53,3))"""
    t = np.linspace(0.0, 1.0, T)
    phase = rng.uniform(0, 6, (bs, 2, 1))
    track = np.stack([3.0 * np.cos(2.3 * np.pi * t + phase[:, 0]), 0.9 + 0.05 * np.sin(9 * t) + 0 * phase[:, 0],
                      2.5 * np.sin(1.7 * np.pi * t + phase[:, 1])], -1)                  # (bs,T,3)
    joints = track[:, :, None, :] + rng.normal(0, 0.3, (bs, T, 53, 3))
    joints[:, :, 0] = track
    N = H * bs
    anchor = track[np.arange(N) % bs][np.arange(N)[:, None], rng.integers(0, T, (N, K))]  # (N,K,3): a frame per proposal
    wide = np.stack([rng.uniform(-14, 14, (N, K)), rng.uniform(0, 2, (N, K)), rng.uniform(-14, 14, (N, K))], -1)
    is_near = rng.uniform(size=(N, K, 1)) < near
    centre = np.where(is_near, anchor + rng.normal(0, 0.8, (N, K, 3)), wide)
    heading = rng.uniform(-np.pi, np.pi, (N, K))
    f32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)     # noqa: E731
    est = {'center': f32(centre), 'size': f32(rng.normal(-0.2, 0.5, (N, K, 3))),
           'heading': torch.from_numpy(np.stack([np.sin(heading), np.cos(heading)], -1)).to(dev),
           'objectness_scores': f32(rng.normal(0, 2, (N, K, 2))), 'sem_cls_scores': f32(rng.normal(0, 2, (N, K, C)))}
    return est, f32(joints)


def timed(fn, iters, dev):
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    for _ in range(iters):
        out = fn()
    torch.cuda.synchronize(dev)
    return (time.perf_counter() - t0) / iters, out


def peak_bytes(fn, dev):
    torch.cuda.synchronize(dev)
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated(dev)
    torch.cuda.reset_peak_memory_stats(dev)
    out = fn()
    torch.cuda.synchronize(dev)
    peak = torch.cuda.max_memory_allocated(dev) - base
    del out
    return int(peak)


def event_us(fn, iters, dev):
    for _ in range(5):
        fn()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(dev)
    start.record()
    for _ in range(iters):
        fn()
    stop.record()
    torch.cuda.synchronize(dev)
    return start.elapsed_time(stop) * 1e3 / iters


def measure(name, bs, T, K, H, cfg, a, rng, dev):
    C = cfg['dataset_config'].num_class
    est, joints = make_inputs(rng, bs, T, K, C, a.near, dev, H)
    expand = lambda: joints.unsqueeze(0).expand(H, *joints.shape).reshape(H * bs, *joints.shape[1:])    # noqa: E731
    paths = {'kernel': lambda: ap_helper.parse_predictions(est, {'input_joints': joints}, cfg, return_device=True,
                                                           impl='kernel', joints_repeat=H)}
    if H == 1:
        paths['torch'] = lambda: ap_helper.parse_predictions(est, {'input_joints': joints}, cfg, return_device=True,
                                                             impl='torch')
    else:
        stacked = expand()
        paths['torch'] = lambda: ap_helper.parse_predictions(est, {'input_joints': stacked}, cfg, return_device=True,
                                                             impl='torch')
        paths['torch+expand'] = lambda: ap_helper.parse_predictions(est, {'input_joints': expand()}, cfg,
                                                                    return_device=True, impl='torch')
    # the same results first
    (ev_t, pa_t), (ev_k, pa_k) = paths['torch'](), paths['kernel']()
    same = {'keep_entries_that_differ': int((ev_t['pred_mask'] != ev_k['pred_mask']).sum()),
            'classes_that_differ': int((pa_t['pred_sem_cls'] != pa_k['pred_sem_cls']).sum()),
            'corners_max_abs_diff': float((pa_t['pred_corners_3d'] - pa_k['pred_corners_3d']).abs().max()),
            'obj_prob_max_abs_diff': float((pa_t['obj_prob'] - pa_k['obj_prob']).abs().max())}
    corners, boxes, _, _, nonempty = parse_device.parse_boxes(
        est['center'], est['size'], est['heading'], est['objectness_scores'], est['sem_cls_scores'], joints=joints,
        origin_joint=cfg['dataset_config'].origin_joint_id, contact_dist=cfg['dataset_config'].contact_dist_thresh)
    share = {'pass_far_box_filter': float(nonempty.float().mean()), 'kept_by_nms': float(ev_k['pred_mask'].float().mean())}
    del ev_t, pa_t, ev_k, pa_k
    for fn in paths.values():                                                           # warm-up
        timed(fn, 2, dev)
    times = {k: [] for k in paths}
    for r in range(a.repeats):
        for k, fn in paths.items():
            times[k].append(timed(fn, a.iters, dev)[0])
            print(f"{name} repeat {r} {k}: {times[k][-1] * 1e3:.3f} ms per call", flush=True)
    peaks = {k: peak_bytes(fn, dev) for k, fn in paths.items()}
    med = {k: float(np.median(v)) * 1e3 for k, v in times.items()}
    kernels = {
        'p2r_parse_boxes_us': event_us(lambda: parse_device.parse_boxes(
            est['center'], est['size'], est['heading'], est['objectness_scores'], est['sem_cls_scores'], joints=joints,
            origin_joint=cfg['dataset_config'].origin_joint_id, contact_dist=cfg['dataset_config'].contact_dist_thresh),
            a.kernel_iters, dev),
        'p2r_nms3d_us': event_us(lambda: nms.nms_3d_batched(boxes, cfg['nms_iou'], False, False, valid=nonempty,
                                                            return_pick=True), a.kernel_iters, dev)}
    return {'shape': {'bs': bs, 'T': T, 'K': K, 'H': H, 'samples': H * bs}, 'share': share, 'same_results': same,
            'ms_per_call': {k: [round(t * 1e3, 3) for t in v] for k, v in times.items()},
            'ms_median': {k: round(v, 3) for k, v in med.items()},
            'torch_over_kernel': {k: round(med[k] / med['kernel'], 2) for k in med if k != 'kernel'},
            'peak_bytes': peaks, 'kernels': {k: round(v, 2) for k, v in kernels.items()}}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--bs', type=int, default=32)
    ap.add_argument('--T', type=int, default=1024)
    ap.add_argument('--K', type=int, default=128)
    ap.add_argument('--H', type=int, default=10, help="hypotheses of the stacked shape")
    ap.add_argument('--near', type=float, default=0.6, help="share of the proposals drawn around the hip track")
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--kernel-iters', type=int, default=200)
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("parse_timing: needs a GPU (a CPU timing says nothing about either path)")
    dev = torch.device('cuda:0')
    cfg = P2RConfig(default_config('test'), device=dev).eval_config
    assert cfg['remove_far_box'] and cfg['parse_impl'] == 'torch'
    rng = np.random.default_rng(a.seed)
    shapes = [('batch', a.bs, a.T, a.K, 1), ('stacked', a.bs, a.T, a.K, a.H), ('long', a.bs, 2 * a.T, a.K, 1)]
    summary = {'config': {'remove_far_box': True, 'nms_iou': cfg['nms_iou'], 'near': a.near, 'iters': a.iters,
                          'repeats': a.repeats},
               'shapes': {name: measure(name, bs, T, K, H, cfg, a, rng, dev) for name, bs, T, K, H in shapes}}
    line = json.dumps(summary)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
