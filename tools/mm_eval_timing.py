#!/usr/bin/env python3
"""Stand-alone measurement (not bench.py): `testing.test_multi_modal` with impl='host' against impl='device' on an
MI355X.

Workload: `--batches` batches of `--bs` samples of `--frames` frames (resident on the device before anything is
timed), `--hyps` hypotheses, untrained weights, `n_samples` fixed at 50 and one seed, so both paths evaluate the same
hypotheses.

  host        test_multi_modal(impl='host'): generate_hypotheses with its host lists, H x T APCalculators, NumPy
              records and TMD
  device      test_multi_modal(impl='device'): generate_hypotheses(return_device=True) into one
              DeviceMultiModalEvaluator
  generation  generate_hypotheses(return_device=True) alone over the same batches: what both paths spend in the
              network, the sampler, the parsing and the NMS
  kernels     p2r_box_params and p2r_tmd alone on one batch's tensors: device events around `--kernel-iters`
              back-to-back launches (launch overhead included)

Every path is warmed up once and then timed alternately `--repeats` times with a host clock around work that ends in
a device synchronise; every repeat is printed, the summary is one JSON line.  Needs a GPU: there is no fallback.

    python tools/mm_eval_timing.py [--out FILE.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn, dev):
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize(dev)
    return time.perf_counter() - t0, out


def kernel_times(hyp, dump_threshold, iters, dev):
    from pose2room_amd.net_utils import mm_device
    corners = hyp['pred_corners_3d'].contiguous()
    keep = ((hyp['pred_mask'] == 1) & (hyp['obj_prob'] > dump_threshold)).to(torch.uint8)
    cls = hyp['pred_sem_cls'].contiguous()
    obbs = mm_device.box_params(corners)
    launches = {'p2r_box_params': lambda: mm_device.box_params(corners),
                'p2r_tmd': lambda: mm_device.tmd_values(obbs, keep, cls)}
    out = {'kept_fraction': round(float(keep.float().mean()), 4)}
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
        out[name + '_us'] = round(start.elapsed_time(stop) * 1e3 / iters, 2)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--batches', type=int, default=3)
    ap.add_argument('--bs', type=int, default=32)
    ap.add_argument('--frames', type=int, default=1024)
    ap.add_argument('--hyps', type=int, default=10)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--kernel-iters', type=int, default=200)
    ap.add_argument('--dump-threshold', type=float, default=0.5)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("mm_eval_timing: needs a GPU (a CPU timing says nothing about the device path)")
    from tests.test_model_cpu import build
    from pose2room_amd.p2rnet import testing
    from pose2room_amd.p2rnet.synthetic import make_batch
    dev = torch.device('cuda:0')
    net, cfg = build('test', a.frames, device=dev)
    net = net.to(dev).eval()
    cfg.log_string = lambda s: None
    batches = [make_batch(a.bs, a.frames, seed=5100 + i, device=dev) for i in range(a.batches)]
    H, kw = a.hyps, dict(n_samples=50, seed=77, dump_threshold=a.dump_threshold)

    def generation():
        with torch.no_grad():
            return [net.generate_hypotheses(d, H, 50, 77 + i, return_device=True) for i, d in enumerate(batches)]

    paths = {'host': lambda: testing.test_multi_modal(cfg, net, batches, H, **kw),
             'device': lambda: testing.test_multi_modal(cfg, net, batches, H, impl='device', **kw),
             'generation': generation}
    results = {k: timed(f, dev)[1] for k, f in paths.items()}                                     # warm-up
    times = {k: [] for k in paths}
    for r in range(a.repeats):
        for k, f in paths.items():
            times[k].append(timed(f, dev)[0])
            print(f"repeat {r} {k}: {times[k][-1] * 1e3:.1f} ms", flush=True)
    host, device = results['host'], results['device']
    summary = {'workload': {'batches': a.batches, 'bs': a.bs, 'frames': a.frames, 'hypotheses': H,
                            'proposals': int(results['generation'][0]['pred_mask'].shape[2]),
                            'thresholds': list(cfg.config['test']['ap_iou_thresholds']), 'dump_threshold': a.dump_threshold},
               'device_name': torch.cuda.get_device_name(dev)}
    for k in paths:
        summary[k + '_ms'] = [round(t * 1e3, 2) for t in times[k]]
        summary[k + '_ms_median'] = round(float(np.median(times[k])) * 1e3, 2)
    summary.update({'tmd_host': host['tmd'], 'tmd_device': device['tmd'],
                    'best_map_host': [float(v) for v in host['best_map']],
                    'best_map_device': [float(v) for v in device['best_map']],
                    'kernels': kernel_times(results['generation'][0], a.dump_threshold, a.kernel_iters, dev)})
    line = json.dumps(summary)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
