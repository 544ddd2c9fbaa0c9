#!/usr/bin/env python3
"""Stand-alone measurement (not bench.py): raw recordings to a finished DeviceSampleStore, device path against host
path, on an MI355X.

Device path: `DeviceSampleStore.from_recordings` over recordings whose float64 joints already sit on the device
(net_utils/sample_build.py: p2r_recording_scan, the read-back of 8 bytes per recording, p2r_build_samples,
p2r_floor_percentile; the per-box rows and box tables on the host).  Host path, on the same input as NumPy arrays:
`sample_build.build_reference` per recording plus the existing `DeviceSampleStore` constructor over its samples, which
walks every sample on the host (`floor_heights`: two np.percentile per sample) and uploads the packed frames.  The
reference's own host path additionally writes and re-reads one file per sample; that is not timed.

Size: `--recordings` 32 recordings of about `--frames` 1100 frames (seeded, +-10 %), 53 joints, `--boxes` 6 objects, 8
variants each; every recording has a few leading frames outside its room.  The two stores are compared first, tensor for
tensor.  Then both paths are warmed up and timed alternately, `--repeats` times each, with a host clock between device
synchronisations (the device path contains a read-back and host work, so device events alone would not cover it); the
three kernels are timed alone with device events, `--repeats` times `--iters` calls each (wrapper allocations
included).  Every repeat is printed, the summary is one JSON line.  Needs a GPU.

    python tools/sample_build_timing.py [--out FILE.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from pose2room_amd.net_utils import sample_build as sb                            # noqa: E402
from pose2room_amd.net_utils import vote_labels as vl                             # noqa: E402
from pose2room_amd.p2rnet import device_loader as dv                              # noqa: E402
from pose2room_amd.p2rnet.synthetic import make_raw_sample                        # noqa: E402


def make_recording(i, frames, boxes, rng):
    """a seeded pose sequence moved to a world offset inside a room, its first frames outside"""
    joints32, _, inst, _ = make_raw_sample(frames, n_boxes=boxes, seed=100 + i)
    world = np.array([rng.uniform(-40, 40), rng.uniform(-2, 2), rng.uniform(-40, 40)])
    joints = joints32.astype(np.float64) + rng.normal(0.0, 1e-5, joints32.shape) + world
    joints[:int(rng.integers(0, 20))] += np.array([25.0, 0.0, 0.0])
    nodes = [dict(class_id=int(n['class_id']), centroid=np.array(n['centroid']) + world, R_mat=np.array(n['R_mat']),
                  size=np.array(n['size'])) for n in inst]
    nodes[0]['centroid'][[0, 2]] = joints[-1, 0, [0, 2]] + 0.2
    room = dict(centroid=world + np.array([0.0, 1.5, 0.0]), size=np.array([9.0, 3.0, 9.5]), R_mat=np.eye(3))
    return dict(name=f'rec{i}', joints=joints, room_bbox=room, object_nodes=nodes)


def spread(v):
    return {'median': round(float(np.median(v)), 4), 'min': round(float(min(v)), 4), 'max': round(float(max(v)), 4),
            'all': [round(float(x), 4) for x in v]}


def clock_ms(fn, dev):
    torch.cuda.synchronize(dev)
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize(dev)
    return (time.perf_counter() - t) * 1e3


def event_ms(fn, iters, repeats, dev):
    """-> ms per call of every repeat: device events around `iters` calls, after a warm-up"""
    for _ in range(3):
        fn()
    out = []
    for _ in range(repeats):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize(dev)
        start.record()
        for _ in range(iters):
            fn()
        stop.record()
        torch.cuda.synchronize(dev)
        out.append(start.elapsed_time(stop) / iters)
    return out


def host_path(recordings, dev):
    samples = []
    for r in recordings:
        built = sb.build_reference(r)
        if built.samples is not None:
            samples += built.samples
    return dv.DeviceSampleStore(samples, device=dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--recordings', type=int, default=32)
    ap.add_argument('--frames', type=int, default=1100)
    ap.add_argument('--boxes', type=int, default=6)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--iters', type=int, default=200, help='calls per repeat of a kernel timed alone')
    ap.add_argument('--out')
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    rng = np.random.default_rng(0)
    host_recs = [make_recording(i, int(a.frames * rng.uniform(0.9, 1.1)), a.boxes, rng) for i in range(a.recordings)]
    dev_recs = [dict(r, joints=torch.from_numpy(r['joints']).to(dev)) for r in host_recs]
    device_path = lambda: dv.DeviceSampleStore.from_recordings(dev_recs, device=dev)              # noqa: E731

    got, want = device_path(), host_path(host_recs, dev)
    for k in ('joints', 'votes', 'frame_offset', 'n_frames', 'floor_height', 'box_center', 'box_heading', 'box_size',
              'box_mask', 'box_cls'):
        assert torch.equal(getattr(got, k), getattr(want, k)), k
    assert got.names == want.names
    N, F = len(got), int(got.joints.shape[0])
    print(f"{a.recordings} recordings -> {N} samples, {F} frames, stores equal", flush=True)

    for _ in range(2):
        device_path()
    host_path(host_recs, dev)
    t_dev, t_host = [], []
    for r in range(a.repeats):                  # alternated: drift of the machine reaches both alike
        t_dev.append(clock_ms(device_path, dev))
        t_host.append(clock_ms(lambda: host_path(host_recs, dev), dev))
        print(f"repeat {r}: device path {t_dev[-1]:.2f} ms, host path {t_host[-1]:.1f} ms", flush=True)

    # the three kernels alone
    built = sb.build_samples(dev_recs, device=dev, max_num_obj=10)
    rec = sb.Recordings([r['joints'] for r in dev_recs], dev)
    objects = vl.ContactBoxes([vl.contact_tables(sb.enlarged_nodes(r['object_nodes'], 1.0), 10, 0.0)
                               for r in host_recs], dev)
    room = torch.from_numpy(np.stack([sb.room_row(r['room_bbox']) for r in host_recs])).to(dev)
    S = len(built.names)
    per = S // len(built.kept)
    col = lambda v: torch.tensor(v, dtype=torch.int32, device=dev)                                  # noqa: E731
    plan = (col(np.repeat(built.kept, per)), col(np.repeat(built.first, per)), col(list(range(8)) * len(built.kept)),
            built.frame_offset, torch.from_numpy(np.stack([sb.floor_shift(host_recs[i]['room_bbox'])
                                                           for i in np.repeat(built.kept, per)])).to(dev))
    max_frames = int(built.n_frames.max())
    kernels = {
        'p2r_recording_scan': event_ms(lambda: sb.recording_scan(rec, room, objects, 0), a.iters, a.repeats, dev),
        'p2r_build_samples': event_ms(lambda: sb.build_packed(rec, *plan, F, built.contact), a.iters, a.repeats, dev),
        'p2r_floor_percentile': event_ms(lambda: sb.floor_percentile(built.joints, built.frame_offset, built.n_frames,
                                                                     max_frames), a.iters, a.repeats, dev)}
    for k, v in kernels.items():
        print(f"{k}: {' '.join(f'{x:.4f}' for x in v)} ms per call", flush=True)
    res = {'tool': 'sample_build_timing', 'recordings': a.recordings, 'frames_in': int(rec.joints.shape[0]), 'samples': N,
           'frames_out': F, 'joints': 53,
           'boxes': a.boxes, 'repeats': a.repeats, 'device_path_ms': spread(t_dev), 'host_path_ms': spread(t_host),
           'kernel_ms': {k: spread(v) for k, v in kernels.items()}, 'kernel_iters': a.iters,
           'gpu': torch.cuda.get_device_name(dev)}
    print(json.dumps(res), flush=True)
    if a.out:
        with open(a.out, 'w') as f:
            json.dump(res, f, indent=1)
            f.write('\n')


if __name__ == '__main__':
    main()
