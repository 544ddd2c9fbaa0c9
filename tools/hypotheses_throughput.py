"""Multi-hypothesis generation throughput at bs=32, T=1024, K=128 (one GPU).

    python tools/hypotheses_throughput.py [--reps 5] [--out profiles/hypotheses_throughput.json]

Times, with device synchronisation around every timed call (median of --reps after warm-up):
  generate          one `P2RNet.generate` (deterministic mixture means)
  ref_n99 / ref_nrand
                    10 hypotheses the reference way: 10 x `generate` with `multi_mode` on (the module path, torch RNG),
                    n_samples = 99, and n_samples drawn in 1..99 per run (proposal_net.py:56-59)
  hyp10             `P2RNet.generate_hypotheses(data, 10)` (trunk once, one sampling launch, one parse / NMS)
  kernel_n99 / kernel_n50
                    the sampling kernel alone (three heads, 10 hypotheses) at n = 99 and n = 50
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, reps, warm=2):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), float(np.min(ts)), float(np.max(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--bs', type=int, default=32)
    ap.add_argument('--frames', type=int, default=1024)
    ap.add_argument('--hyps', type=int, default=10)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("hypotheses_throughput needs a GPU")
    from tests.test_model_cpu import build
    from pose2room_amd.p2rnet import mdn_sample_op
    from pose2room_amd.p2rnet.synthetic import make_batch
    dev = torch.device('cuda:0')
    net, cfg = build('test', a.frames, device=dev, remove_far_box=False)   # untrained weights: keep every box
    net = net.to(dev).eval()
    data = make_batch(a.bs, a.frames, seed=31, device=dev)
    det = net.detection
    H = a.hyps
    res = {'bs': a.bs, 'frames': a.frames, 'proposals': cfg.config['data']['num_target'], 'hypotheses': H,
           'device': torch.cuda.get_device_name(dev)}
    with torch.no_grad():
        res['generate_ms'] = timed(lambda: net.generate(data), a.reps)

        def ref_way(ns):
            det.multi_mode = True
            try:
                for n in ns:
                    det.n_samples = int(n)
                    net.generate(data)
            finally:
                det.multi_mode = False
        res['ref_n99_ms'] = timed(lambda: ref_way([99] * H), a.reps, warm=1)
        rng = np.random.default_rng(0)
        res['ref_nrand_ms'] = timed(lambda: ref_way(rng.integers(1, 100, H)), a.reps, warm=1)
        seeds = iter(range(10 ** 6))
        res['hyp_ms'] = timed(lambda: net.generate_hypotheses(data, H, seed=next(seeds)), a.reps)
        ep = net.generate_end_points(data)
        heads = [det.gmm_center.mdn, det.gmm_size.mdn, det.gmm_heading.mdn]
        pis = [ep['pi'][k] for k in ('center', 'size', 'heading')]
        for n in (99, 50):
            res[f'kernel_n{n}_ms'] = timed(lambda: mdn_sample_op.sample(heads, pis, [n] * H, 7), a.reps)
    res['hyp_over_generate'] = res['hyp_ms'][0] / res['generate_ms'][0]
    res['kernel_n99_ms_per_hypothesis'] = res['kernel_n99_ms'][0] / H
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
