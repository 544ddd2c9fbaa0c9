#!/usr/bin/env python3
"""Stand-alone measurement (not bench.py): the consensus scene of H hypotheses, device form against the NumPy definition,
on an MI355X.

Device form: `consensus_device.consensus_clusters` on the node tensors of a SceneBatch (p2r_consensus: two launches,
nothing copied to the host).  Host form: `consensus_device.consensus_reference` on the same arrays already on the host --
the definition, which evaluates the pair IoUs in chunks with the tensor code of net_utils/box_util.py on the CPU and walks
the items in a Python loop; a loop over `box3d_iou` pairs, which it restates, is slower still.

Shape: bs x H x K = 32 x 10 x 128, once with about `--keep` = 10 % of the node slots in use (what a dump threshold leaves
of a trained model's proposals) and once with all of them.  Every sample has its own objects (22 classes); every
hypothesis places jittered copies of a random choice of them, so clusters form across hypotheses and, at 100 %, boxes
overlap inside a hypothesis too.

Per shape: the device and the host result are compared first (no margin is designed into these inputs: the number of
samples whose clustering differs is reported, not asserted); the device form is warmed up and timed `--repeats` times with
device events around `--iters` calls; the host form is timed `--host-repeats` times with a host clock (once for the full
shape).  Every repeat is printed, the summary is one JSON line with the medians.  Needs a GPU.

    python tools/consensus_timing.py [--out FILE.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from scene_timing import event_ms, spread                                         # noqa: E402
from pose2room_amd.net_utils import consensus_device as cd                        # noqa: E402


def make_nodes(rng, bs, H, K, keep, classes=22):
    """-> count (N) i32, node_obbs (N,K,7) f64, node_cls (N,K) i64, node_score (N,K) f32, hypothesis-major"""
    N = H * bs
    per = max(int(round(keep * K)), 1)
    n_obj = per + max(per // 6, 3)
    extent = 1.2 * np.sqrt(n_obj)                            # the room grows with the objects: the density stays
    count = np.zeros(N, np.int32)
    obbs, cls, score = np.zeros((N, K, 7)), np.zeros((N, K), np.int64), np.zeros((N, K), np.float32)
    for b in range(bs):
        ctr = np.stack([rng.uniform(-extent, extent, n_obj), rng.uniform(0, 1, n_obj), rng.uniform(-extent, extent, n_obj)], -1)
        size = np.exp(rng.normal(-0.2, 0.4, (n_obj, 3)))
        head = rng.uniform(-np.pi, np.pi, n_obj)
        ocls = rng.integers(0, classes, n_obj)
        for h in range(H):
            n = h * bs + b
            c = min(max(per + int(rng.integers(-2, 3)) if keep < 1 else K, 0), K, n_obj)
            o = rng.permutation(n_obj)[:c]
            count[n] = c
            obbs[n, :c, 0:3] = ctr[o] + rng.normal(0, 0.05, (c, 3))
            obbs[n, :c, 3:6] = size[o] * np.exp(rng.normal(0, 0.05, (c, 3)))
            obbs[n, :c, 6] = head[o] + rng.normal(0, 0.05, c) + np.pi * (rng.uniform(size=c) < 0.2)
            cls[n, :c] = np.where(rng.uniform(size=c) < 0.9, ocls[o], rng.integers(0, classes, c))
            score[n, :c] = rng.uniform(0.5, 1.0, c)
    return count, obbs, cls, score


def measure(name, bs, H, K, keep, a, rng, dev):
    host_in = make_nodes(rng, bs, H, K, keep)
    dev_in = [torch.from_numpy(x).to(dev) for x in host_in]
    run = lambda: cd.consensus_clusters(*dev_in, H, a.iou_thresh, True)           # noqa: E731
    got = cd.Consensus(*[t.cpu().numpy() for t in run()])
    host_times = []
    for r in range(a.host_repeats if keep < 1 else 1):
        t0 = time.perf_counter()
        want = cd.consensus_reference(*host_in, H, a.iou_thresh, True)
        host_times.append((time.perf_counter() - t0) * 1e3)
        print(f"{name} host repeat {r}: {host_times[-1]:.1f} ms", flush=True)
    differ = sum(not (got.n_clusters[b] == want.n_clusters[b] and np.array_equal(got.cluster_of[b::bs], want.cluster_of[b::bs]))
                 for b in range(bs))
    stat = max(float(np.nanmax(np.abs(getattr(got, f) - getattr(want, f)))) for f in ('score_mean', 'center_mean',
                                                                                       'center_rms', 'iou_mean')) if not differ else None
    times = event_ms(run, a.iters, a.repeats, dev, f"{name} consensus_clusters")
    pool = np.clip(host_in[0], 0, K).reshape(H, bs).sum(0)
    n = want.n_clusters
    return {'shape': {'bs': bs, 'H': H, 'K': K, 'keep': keep, 'pool_mean': float(pool.mean()), 'pool_max': int(pool.max())},
            'clusters_mean': float(n.mean()), 'support_mean': float(np.mean([want.support[b, :n[b]].mean() for b in range(bs)])),
            'samples_whose_clustering_differs': differ, 'max_statistic_difference': stat,
            'workspace_bytes': int(cd.lib().p2r_consensus_workspace_bytes(H, bs, K)),
            'device_ms': spread(times), 'host_ms': spread(host_times),
            'host_over_device': round(float(np.median(host_times)) / float(np.median(times)), 1)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--bs', type=int, default=32)
    ap.add_argument('--H', type=int, default=10)
    ap.add_argument('--K', type=int, default=128)
    ap.add_argument('--keep', type=float, default=0.1, help="share of the node slots in use in the sparse shape")
    ap.add_argument('--iou-thresh', type=float, default=0.25)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--host-repeats', type=int, default=3)
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("consensus_timing: needs a GPU (a CPU timing says nothing about the device form)")
    dev = torch.device('cuda:0')
    rng = np.random.default_rng(a.seed)
    summary = {'config': {'iou_thresh': a.iou_thresh, 'iters': a.iters, 'repeats': a.repeats},
               'shapes': {name: measure(name, a.bs, a.H, a.K, keep, a, rng, dev) for name, keep in (('sparse', a.keep), ('full', 1.0))}}
    line = json.dumps(summary)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
