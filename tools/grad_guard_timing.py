#!/usr/bin/env python3
"""Stand-alone measurement (not bench.py): what the stretch between `backward()` and the end of `optimizer.step()` costs on
an MI355X with torch's clipping and with the gradient guard (pose2room_amd/p2rnet/grad_guard.py, csrc/grad_guard.hip).

The model, the optimizer and the batch are bench.py's (bs = 32, T = 1024, fused AdamW).  `optimizer.clip_norm` is set to
half of a norm measured first, so clipping is active in every timed step; the scales seen are reported.

  (after the norm is measured the learning rate is set to 0: the optimizer launches and computes the same, but the weights,
  and so the norm, stay, and every timed step clips)
  stretch   device events around clip + step of a step that is otherwise `Trainer.train_step`, for `clip_impl: 'torch'`
            (torch.nn.utils.clip_grad_norm_ + optimizer.step()) and for `'kernel'` (GradGuard.step); the two alternate
            inside one process, block by block, after both were warmed; every step is one sample; medians and spread.
  launches  the device activities (kernels, copies, memsets) between two marker kernels around that stretch in one
            profiled step per path -- a run of its own after the timings, since the profiler slows the host.
  step      the whole `Trainer.train_step` (device events around `--iters` steps, per step) with the guard off and no
            clipping, with torch's clipping, with 'kernel' clipping, with 'kernel' clipping and `nonfinite: 'skip'`, and
            with 'skip' alone; alternating in the same way.

No ratio is promised: the JSON says what was measured.  Needs a GPU.

    python tools/grad_guard_timing.py [--out profiles/grad_guard_timing.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench                                                                    # noqa: E402
from pose2room_amd.p2rnet.grad_guard import GradGuard                            # noqa: E402
from pose2room_amd.p2rnet.synthetic import make_batch                            # noqa: E402
from pose2room_amd.p2rnet.training import _ScalarFetch, reduce_dict              # noqa: E402


def spread(v):
    v = [float(x) for x in v]
    return {'median': round(float(np.median(v)), 4), 'min': round(min(v), 4), 'max': round(max(v), 4),
            'p10': round(float(np.percentile(v, 10)), 4), 'p90': round(float(np.percentile(v, 90)), 4), 'n': len(v)}


class Paths(object):
    """One trainer, several ways through clip + step: the trainer's keys and guard are switched per path"""

    def __init__(self, trainer, clip_norm):
        self.trainer, self.clip_norm = trainer, clip_norm
        net, opt = trainer.net, trainer.optimizer
        self.guards = {'kernel': GradGuard(net.named_parameters(), clip_norm, 'ignore', optimizer=opt),
                       'kernel+skip': GradGuard(net.named_parameters(), clip_norm, 'skip', optimizer=opt),
                       'skip': GradGuard(net.named_parameters(), 0.0, 'skip', optimizer=opt)}

    def use(self, path):
        """'off' | 'torch' | 'kernel' | 'kernel+skip' | 'skip' -> the trainer as `Trainer.__init__` would have made it"""
        self.trainer.cfg.config['optimizer']['clip_norm'] = -1 if path in ('off', 'skip') else self.clip_norm
        self.trainer.grad_guard = self.guards.get(path)

    def stretch_step(self, batch, start, stop):
        """`Trainer.train_step` with `start` / `stop` recorded around clip + step"""
        t = self.trainer
        t.optimizer.zero_grad()
        loss = t.compute_loss(batch)
        fetch = _ScalarFetch(reduce_dict(loss))
        loss['total'].backward()
        start.record()
        with torch.profiler.record_function('gg_stretch'):       # a range to find in a trace
            if t.grad_guard is not None:
                t.grad_guard.step(t.optimizer)
            else:
                torch.nn.utils.clip_grad_norm_(t.net.parameters(), self.clip_norm)
                t.optimizer.step()
        stop.record()
        return fetch.result()


def time_stretch(paths, batch, dev, a):
    out = {'torch': [], 'kernel': []}
    scales = []
    for path in out:                                    # warm both first
        paths.use(path)
        for _ in range(a.warmup):
            paths.stretch_step(dict(batch), torch.cuda.Event(), torch.cuda.Event())
    torch.cuda.synchronize(dev)
    for r in range(a.repeats):
        for path in out:
            paths.use(path)
            evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.iters)]
            for s, e in evs:
                paths.stretch_step(dict(batch), s, e)
            torch.cuda.synchronize(dev)
            ms = [s.elapsed_time(e) for s, e in evs]
            out[path] += ms
            if path == 'kernel':
                scales.append(paths.guards[path].report()['scale'])
            print(f"stretch {path} block {r}: median {np.median(ms) * 1e3:.1f} us", flush=True)
    res = {k: spread([x * 1e3 for x in v]) for k, v in out.items()}       # microseconds
    res['kernel_scale_at_block_ends'] = scales
    return res


def time_steps(paths, batch, dev, a):
    names = ('off', 'torch', 'kernel', 'kernel+skip', 'skip')
    out = {k: [] for k in names}
    for path in names:
        paths.use(path)
        for _ in range(a.warmup):
            paths.trainer.train_step(dict(batch))
    torch.cuda.synchronize(dev)
    for r in range(a.repeats):
        for path in names:
            paths.use(path)
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize(dev)
            s.record()
            for _ in range(a.iters):
                paths.trainer.train_step(dict(batch))
            e.record()
            torch.cuda.synchronize(dev)
            out[path].append(s.elapsed_time(e) / a.iters)
            print(f"step {path} block {r}: {out[path][-1]:.3f} ms per step", flush=True)
    return {k: spread(v) for k, v in out.items()}                         # milliseconds


def count_launches(paths, batch, dev):
    """-> {path: {'launches': n, 'by_name': {name: n}}} of one profiled step per path: the device activities (kernels,
    copies, memsets) that lie on the device's timeline between two marker kernels (`torch.cuda._sleep`) launched right in
    front of and right behind the stretch"""
    from torch.autograd import DeviceType
    from torch.profiler import ProfilerActivity, profile

    class Marker(object):
        def record(self):
            torch.cuda._sleep(1000)

    res = {}
    for path in ('torch', 'kernel'):
        paths.use(path)
        torch.cuda.synchronize(dev)
        with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
            paths.stretch_step(dict(batch), Marker(), Marker())
            torch.cuda.synchronize(dev)
        # the device timeline also mirrors the host's annotations (record_function ranges): those are no launches
        host_names = {ev.name for ev in prof.events() if ev.device_type == DeviceType.CPU}
        device = sorted((ev for ev in prof.events() if ev.device_type == DeviceType.CUDA and ev.name not in host_names),
                        key=lambda ev: ev.time_range.start)
        marks = [i for i, ev in enumerate(device) if 'spin_kernel' in ev.name]
        if len(marks) != 2:
            raise RuntimeError(f"grad_guard_timing: {len(marks)} marker kernels in the trace, 2 expected")
        by_name = {}
        for ev in device[marks[0] + 1:marks[1]]:
            by_name[ev.name] = by_name.get(ev.name, 0) + 1
        res[path] = {'launches': sum(by_name.values()), 'by_name': dict(sorted(by_name.items(), key=lambda kv: -kv[1]))}
        print(f"launches {path}: {res[path]['launches']}", flush=True)
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--frames', type=int, default=1024)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--repeats', type=int, default=5, help="blocks per path; the paths alternate block by block")
    ap.add_argument('--iters', type=int, default=10, help="steps per block")
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("grad_guard_timing: needs a GPU (a CPU timing says nothing about the device)")
    dev = torch.device('cuda:0')
    trainer, cfg = bench.build_trainer(dev, a.frames, 1)
    batch = make_batch(a.batch, a.frames, seed=1234, device=dev)
    for _ in range(a.warmup):
        trainer.train_step(dict(batch))
    probe = GradGuard(trainer.net.named_parameters(), 0.0, 'ignore', optimizer=trainer.optimizer)
    trainer.grad_guard = probe
    trainer.train_step(dict(batch))
    measured = probe.report()
    clip_norm = measured['norm'] / 2
    n_params = len(probe.params)
    numel = sum(p.numel() for p in probe.params)
    print(f"measured norm {measured['norm']:.6g} over {n_params} tensors / {numel} elements -> clip_norm {clip_norm:.6g}",
          flush=True)
    # the learning rate is 0 from here on: the same launches and the same arithmetic in the optimizer, but the weights --
    # and with them the gradient norm that was just measured -- stay, so clipping is active in every timed step
    for group in trainer.optimizer.param_groups:
        group['lr'] = 0.0
    paths = Paths(trainer, clip_norm)
    stretch = time_stretch(paths, batch, dev, a)
    steps = time_steps(paths, batch, dev, a)
    launches = count_launches(paths, batch, dev)
    reports = {k: g.report() for k, g in paths.guards.items()}
    summary = {'config': {'batch': a.batch, 'frames': a.frames, 'warmup': a.warmup, 'repeats': a.repeats, 'iters': a.iters,
                          'torch': torch.__version__, 'device': torch.cuda.get_device_name(dev)},
               'gradients': {'tensors': n_params, 'elements': numel, 'measured_norm': measured['norm'], 'clip_norm': clip_norm},
               'stretch_us': stretch, 'stretch_launches': launches, 'step_ms': steps,
               'guards_after': {k: {f: r[f] for f in ('steps', 'skipped', 'norm', 'scale')} for k, r in reports.items()}}
    line = json.dumps(summary)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
