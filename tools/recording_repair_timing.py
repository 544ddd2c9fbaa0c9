#!/usr/bin/env python3
"""Stand-alone measurement (not bench.py): the recording repair on an MI355X against its NumPy definition on the host
of the same machine.

Input: `--recordings` 32 recordings of about `--frames` 1100 frames (seeded, +-10 %), 53 joints, float64, `--missing`
2 % of the (frame, joint) items missing in gaps of 1 to `--longest` 40 frames.  The spec is RepairSpec(30, True,
`--smooth` 2): gaps above 30 frames stay NaN.  The device result is compared with `repair_reference` first, bit for bit
where it is finite.  Then the three entry points are timed alone with device events (`--repeats` times `--iters` calls,
wrapper allocations included), `repair_packed` likewise (its launches are asynchronous, so device events cover it), and
`repair_reference` with a host clock on the same recordings as NumPy arrays.  Every repeat is printed, the summary is one
JSON line.  Needs a GPU.

    python tools/recording_repair_timing.py [--out FILE.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from pose2room_amd.net_utils import recording_repair as rr                        # noqa: E402
from pose2room_amd.net_utils import sample_build as sb                            # noqa: E402


def make_recording(frames, share, longest, rng, J=53):
    """(frames, J, 3) f64 random-walk tracks with `share` of the items missing in gaps of 1 .. longest frames"""
    x = np.cumsum(rng.normal(0.0, 0.01, (frames, J, 3)), 0) + rng.uniform(-2, 2, (1, J, 3))
    want, missing = int(share * frames * J), 0
    while missing < want:
        g, j = int(rng.integers(1, longest + 1)), int(rng.integers(J))
        f = int(rng.integers(-g // 2, frames))
        x[max(f, 0):f + g, j] = np.nan
        missing = int(np.isnan(x[:, :, 0]).sum())
    return x


def spread(v):
    return {'median': round(float(np.median(v)), 4), 'min': round(float(min(v)), 4), 'max': round(float(max(v)), 4),
            'all': [round(float(x), 4) for x in v]}


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--recordings', type=int, default=32)
    ap.add_argument('--frames', type=int, default=1100)
    ap.add_argument('--missing', type=float, default=0.02)
    ap.add_argument('--longest', type=int, default=40)
    ap.add_argument('--smooth', type=int, default=2)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--iters', type=int, default=100, help='calls per repeat of what is timed with device events')
    ap.add_argument('--out')
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    rng = np.random.default_rng(0)
    host = [make_recording(int(a.frames * rng.uniform(0.9, 1.1)), a.missing, a.longest, rng) for _ in range(a.recordings)]
    spec = rr.RepairSpec(30, True, a.smooth)
    rec = sb.Recordings(host, dev)

    want = rr.repair_reference(host, spec)
    fixed, how, stats = rr.repair_packed(rec, spec)
    got, finite = fixed.joints.cpu().numpy(), np.isfinite(want[0])
    assert np.array_equal(np.isfinite(got), finite) and np.array_equal(got[finite].view(np.uint64), want[0][finite].view(np.uint64))
    assert np.array_equal(how.cpu().numpy(), want[1]) and np.array_equal(stats.cpu().numpy(), want[2])
    total = want[2].sum(0)
    print(f"{a.recordings} recordings, {rec.joints.shape[0]} frames, {int(total[0])} of {want[1].size} items missing, "
          f"{int(total[1])} filled, {int(total[2])} left; device equals the definition", flush=True)

    bits = rr.valid_bits(rec)
    timed = {
        'p2r_joint_valid_bits': lambda: rr.valid_bits(rec),
        'p2r_gap_fill': lambda: rr.gap_fill(rec, bits, spec.max_gap, spec.hold_ends),
        'p2r_smooth_frames': lambda: rr.smooth_frames(fixed, max(a.smooth, 1)),
        'repair_packed': lambda: rr.repair_packed(rec, spec),
    }
    device_ms = {k: event_ms(fn, a.iters, a.repeats, dev) for k, fn in timed.items()}
    for k, v in device_ms.items():
        print(f"{k}: {' '.join(f'{x:.4f}' for x in v)} ms per call", flush=True)
    t_host = []
    rr.repair_reference(host, spec)
    for r in range(a.repeats):
        t = time.perf_counter()
        rr.repair_reference(host, spec)
        t_host.append((time.perf_counter() - t) * 1e3)
        print(f"repeat {r}: repair_reference {t_host[-1]:.1f} ms", flush=True)
    res = {'tool': 'recording_repair_timing', 'recordings': a.recordings, 'frames': int(rec.joints.shape[0]), 'joints': 53,
           'items': int(want[1].size), 'missing': int(total[0]), 'filled': int(total[1]), 'left': int(total[2]),
           'spec': list(spec), 'repeats': a.repeats, 'iters': a.iters,
           'device_ms': {k: spread(v) for k, v in device_ms.items()}, 'repair_reference_ms': spread(t_host),
           'gpu': torch.cuda.get_device_name(dev)}
    print(json.dumps(res), flush=True)
    if a.out:
        with open(a.out, 'w') as f:
            json.dump(res, f, indent=1)
            f.write('\n')


if __name__ == '__main__':
    main()
