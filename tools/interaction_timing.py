#!/usr/bin/env python3
"""Stand-alone measurement (not bench.py): the interaction timeline of predicted scenes, device form against the NumPy
definition, against a plain torch formulation on the same GPU and against `p2r_contact_frames` on the same inputs, on
an MI355X.

Device form: the three launches alone -- `contact_bits` (without and with the per-frame joint counts), `contact_intervals`,
`frame_labels` -- and the whole of `interactions_of` (three launches and their allocations).  Compared with:
  (a) `interaction_reference`, the definition, on `--host-samples` samples of the stack; its time for the whole stack is
      that figure times N / samples and is reported as an extrapolation, not as a measurement;
  (b) the box rule written with torch broadcasting in this file -- per sample a (nodes, T * J, 3) float64 tensor of
      offsets, a product with R, a comparison, reductions over joints and frames; bit-packing, intervals and labels left
      out -- timed over the whole stack;
  (c) `scene_device.contact_frames` (p2r_contact_frames), which runs the same N * K * T * J loop with a maximum and a
      minimum where `contact_bits` has three comparisons and a ballot.

Shape: bs x K = 32 x 128, T = 1024 frames of 53 joints, H = 1 and 10, with `--keep` = 10 % of the node slots in use and
with all of them.  A body wanders through a room of furniture-sized boxes, so that contacts come and go.

Per shape the results are compared first (the number of differing elements is reported, not asserted); the device forms
are warmed up and timed `--repeats` times with device events around `--iters` calls, the torch form with `--torch-iters`;
the host form with a host clock.  Every repeat is printed, the summary is one JSON line with the medians.  Needs a GPU.

    python tools/interaction_timing.py [--out FILE.json]
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

from occupancy_timing import head2rot, torch_ms                                    # noqa: E402
from scene_timing import event_ms, spread                                          # noqa: E402
from pose2room_amd.net_utils import interaction_device as idv                      # noqa: E402
from pose2room_amd.net_utils import scene_device as sd                             # noqa: E402


def make_scene(rng, bs, H, K, keep, T, J):
    """-> joints (bs,T,J,3) f32, count (N) i32, node_obbs (N,K,7) f64, node_rmat (N,K,3,3) f64"""
    N = H * bs
    t = np.arange(T)[None, :, None] / T
    f, ph = rng.uniform(1.0, 6.0, (bs, 1, 3)), rng.uniform(0, 2 * np.pi, (bs, 1, 3))
    centre = np.array([2.5, 0.0, 2.5]) * np.sin(2 * np.pi * f * t + ph) + np.array([0.0, 0.9, 0.0])
    joints = (centre[:, :, None, :] + rng.uniform(-0.5, 0.5, (bs, 1, J, 3)) + rng.normal(0, 0.03, (bs, T, J, 3)))
    per = max(int(round(keep * K)), 1)
    count = np.full(N, K, np.int32) if keep >= 1 else np.clip(per + rng.integers(-2, 3, N), 0, K).astype(np.int32)
    obbs = np.zeros((N, K, 7))
    obbs[..., 0:3] = rng.uniform([-3.0, 0.2, -3.0], [3.0, 1.4, 3.0], (N, K, 3))
    obbs[..., 3:6] = np.exp(rng.normal(-0.2, 0.4, (N, K, 3)))
    obbs[..., 6] = rng.uniform(-np.pi, np.pi, (N, K))
    live = np.arange(K)[None] < count[:, None]
    obbs *= live[..., None]
    return joints.astype(np.float32), count, obbs, head2rot(obbs[..., 6]) * live[..., None, None]


def torch_form(count_host, joints, obbs, rmat, thresh):
    """The box rule with broadcasting -> (contact bool (N,K,T), njoint int64 (N,K,T)).  count_host: the counts on the host
    (the formulation slices the counted nodes; a device count would cost a read-back per call)."""
    N, K = obbs.shape[:2]
    B, T, J = joints.shape[:3]
    contact = torch.zeros((N, K, T), dtype=torch.bool, device=obbs.device)
    njoint = torch.zeros((N, K, T), dtype=torch.int64, device=obbs.device)
    for n in range(N):
        m = int(min(max(count_host[n], 0), K))
        if m == 0:
            continue
        p = joints[n % B, :, :, 0:3].reshape(-1, 3).to(torch.float64)
        d = p[None] - obbs[n, :m, None, 0:3]                                                  # (m, T * J, 3)
        local = (d[:, :, None, :] * rmat[n, :m, None]).sum(-1)                                # (m, T * J, 3)
        inside = (local.abs() <= (obbs[n, :m, None, 3:6] / 2.0 + thresh)).all(-1).reshape(m, T, J)
        njoint[n, :m] = inside.sum(-1)
        contact[n, :m] = inside.any(-1)
    return contact, njoint


def measure(name, bs, H, K, keep, a, rng, dev):
    N = H * bs
    joints_h, count_h, obbs_h, rmat_h = make_scene(rng, bs, H, K, keep, a.T, a.J)
    joints, count, obbs, rmat = (torch.from_numpy(x).to(dev) for x in (joints_h, count_h, obbs_h, rmat_h))
    scenes = sd.SceneBatch(H, bs, K, count, torch.zeros(N, K, dtype=torch.int32, device=dev), obbs, rmat,
                           torch.zeros(N, K, dtype=torch.int64, device=dev), torch.zeros(N, K, dtype=torch.float32, device=dev))
    run = dict(contact_thresh=a.thresh, merge_gap=a.merge_gap, min_len=a.min_len, max_intervals=16)
    batch = scenes.interactions(joints, **run)
    got = batch.host()
    dense = idv.unpack_bits(got['bits'], a.T)
    res = {'shape': {'bs': bs, 'H': H, 'K': K, 'T': a.T, 'J': a.J, 'keep': keep, 'nodes_mean': float(np.clip(count_h, 0, K).mean()),
                     'box_tests': int(np.clip(count_h, 0, K).sum()) * a.T * a.J, **run},
           'contact_share_of_node_frames': float(dense[np.arange(K)[None] < count_h[:, None]].mean()),
           'intervals_per_node': float(got['n_intervals'].sum() / max(int(np.clip(count_h, 0, K).sum()), 1)),
           'labelled_share_of_frames': float(got['n_labelled'].sum() / (N * a.T))}
    # (a) the definition on a few samples: rows 0 .. ns-1 of the stack read joints rows 0 .. ns-1
    ns = min(a.host_samples, bs)
    t0 = time.perf_counter()
    want = idv.interaction_reference(joints_h[:ns], count_h[:ns], obbs_h[:ns], rmat_h[:ns], a.thresh, a.merge_gap, a.min_len, 16)
    host_ms = (time.perf_counter() - t0) * 1e3
    print(f"{name} host definition, {ns} of {N} samples: {host_ms:.1f} ms", flush=True)
    res.update(host_samples=ns, host_ms_measured=round(host_ms, 1), host_ms_extrapolated_to_N=round(host_ms * N / ns, 1),
               elements_differing_from_definition={f: int((got[f][:ns] != getattr(want, f)).sum()) for f in idv.Interaction._fields})
    # (b) the torch form
    tf = lambda: torch_form(count_h, joints, obbs, rmat, a.thresh)                # noqa: E731
    contact, njoint = tf()
    res['frames_differing_from_torch_form'] = int((torch.from_numpy(dense).to(dev) != contact).sum())
    res['njoint_differing_from_torch_form'] = int((batch.njoint.to(torch.int64) != njoint).sum())
    del contact, njoint
    res['torch_form_ms'] = spread(torch_ms(tf, a.torch_iters, a.torch_repeats, dev, f"{name} torch form"))
    # the launches
    ev = lambda fn, label: spread(event_ms(fn, a.iters, a.repeats, dev, f"{name} {label}"))      # noqa: E731
    res['contact_bits_ms'] = ev(lambda: idv.contact_bits(joints, obbs, rmat, count, a.thresh, njoint=False), "contact_bits")
    res['contact_bits_njoint_ms'] = ev(lambda: idv.contact_bits(joints, obbs, rmat, count, a.thresh), "contact_bits with njoint")
    res['contact_intervals_ms'] = ev(lambda: idv.contact_intervals(batch.bits, count, a.T, a.merge_gap, a.min_len, 16),
                                     "contact_intervals")
    res['frame_labels_ms'] = ev(lambda: idv.frame_labels(batch.clean, batch.njoint, count), "frame_labels")
    res['interactions_of_ms'] = ev(lambda: scenes.interactions(joints, **run), "SceneBatch.interactions")
    # (c) the same loop with a minimum at its end
    res['contact_frames_ms'] = ev(lambda: sd.contact_frames(joints, obbs, rmat, count), "contact_frames")
    res['bits_over_contact_frames'] = round(res['contact_bits_ms']['median'] / res['contact_frames_ms']['median'], 2)
    res['torch_over_interactions_of'] = round(res['torch_form_ms']['median'] / res['interactions_of_ms']['median'], 1)
    res['host_extrapolated_over_interactions_of'] = round(res['host_ms_extrapolated_to_N'] / res['interactions_of_ms']['median'], 1)
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--bs', type=int, default=32)
    ap.add_argument('--K', type=int, default=128)
    ap.add_argument('--T', type=int, default=1024)
    ap.add_argument('--J', type=int, default=53)
    ap.add_argument('--keep', type=float, default=0.1, help="share of the node slots in use in the sparse shape")
    ap.add_argument('--thresh', type=float, default=0.1)
    ap.add_argument('--merge-gap', type=int, default=2)
    ap.add_argument('--min-len', type=int, default=3)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--torch-repeats', type=int, default=2)
    ap.add_argument('--torch-iters', type=int, default=1)
    ap.add_argument('--host-samples', type=int, default=1)
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("interaction_timing: needs a GPU (a CPU timing says nothing about the device form)")
    dev = torch.device('cuda:0')
    rng = np.random.default_rng(a.seed)
    shapes = {}
    for H in (1, 10):
        for tag, keep in (('sparse', a.keep), ('full', 1.0)):
            name = f"H{H}-{tag}"
            shapes[name] = measure(name, a.bs, H, a.K, keep, a, rng, dev)
    summary = {'config': {'iters': a.iters, 'repeats': a.repeats, 'torch_iters': a.torch_iters, 'torch_repeats': a.torch_repeats},
               'shapes': shapes}
    line = json.dumps(summary)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
