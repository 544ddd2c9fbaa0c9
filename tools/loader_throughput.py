"""Sample loader throughput at bs=32, T=1024 (one GPU): the host loader against the device sample store.

    python tools/loader_throughput.py [--samples 384] [--t0 512 2048] [--batches 12] [--workers 0 4 15]
                                      [--train-steps 20] [--only device] [--lean] [--store-build 256 1024]
                                      [--out profiles/loader_throughput.json]

Raw samples are synthetic (p2rnet/synthetic.make_raw_sample, six boxes), T0 drawn uniformly from the --t0 range.
Timed, with a device synchronisation at the end of each measurement, in 'train' mode (augmentation on):
  host_w<N>     P2RNet_dataloader over the samples in host memory (dataloader.py: augment_sample + sample_to_tensors +
                collate_fn in N worker processes), each batch copied to the GPU as Trainer.to_device does; timed from
                the start of the epoch (worker start-up included) to the last batch
  device        P2RNet_device_dataloader over a DeviceSampleStore of the same samples (one launch per batch)
  assemble_ms   one DeviceSampleStore.assemble call at bs, T, median of --reps (host draws + launch, synchronised)
  assemble_kernel_us  the assemble launch alone: --kernel-reps back-to-back launches between device events, launch
                overhead included, per launch; with --lean also for the lean store (votes='derive': no stored votes,
                p2r_assemble_batch_lean derives them in the launch) built from the same samples, plus that store's
                bytes and its device-loader rate
  store_build   with --store-build N T: the votes of N samples of T frames (six boxes each) by ONE p2r_vote_labels launch
                (device events, median of --reps, and the achieved GB/s of its 12 bytes in + 40 bytes out per item)
                against the NumPy mirror on the host for the same samples, and the wall time of building the store
                from samples that bring no votes
  step_<loader> with --train-steps S: S train steps (Trainer.train_step) fed by the host loader with the most workers
                and by the device loader, wall time per step
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


def rate(loader, n_batches, dev):
    """samples / s from the start of the epoch (worker start-up included) to the n_batches-th batch on the device."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    n = 0
    for i, b in enumerate(loader):
        for k, v in b.items():
            if torch.is_tensor(v):
                b[k] = v.to(dev)
        n += len(b['sample_idx'])
        if i + 1 == n_batches:
            break
    torch.cuda.synchronize()
    return n / (time.perf_counter() - t0)


def kernel_us(store, dv, dl, bs, frames, reps):
    """one assemble launch, microseconds: `reps` back-to-back launches on preallocated operands between device events"""
    ids = list(range(bs))
    out = store.assemble(ids, frames, True, [dl.draw_augmentation() for _ in ids])           # warm-up; the operands
    tens = {k: v for k, v in out.items() if torch.is_tensor(v)}
    sel = torch.zeros((bs, 3), dtype=torch.int64)
    sel[:, 0] = torch.arange(bs)
    sel[:, 1], sel[:, 2] = 1, 4 + 1
    aug = torch.zeros((bs, 10), dtype=torch.float64)
    aug[:, 0:9] = torch.from_numpy(dl.rot_y(dv.ANGLES[1]).reshape(9))
    aug[:, 9] = 0.37
    sel, aug = sel.to(store.device), aug.to(store.device)
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    dv.assemble_batch(store, sel, aug, True, False, frames, tens)
    torch.cuda.synchronize()
    start.record()
    for _ in range(reps):
        dv.assemble_batch(store, sel, aug, True, False, frames, tens)
    end.record()
    torch.cuda.synchronize()
    return round(start.elapsed_time(end) * 1e3 / reps, 2)


def store_build(n, frames, reps, dev, dv, make_raw_sample):
    """p2r_vote_labels over n samples of `frames` frames against the NumPy mirror on the host"""
    from pose2room_amd.net_utils import vote_labels as vl
    samples = [make_raw_sample(frames, n_boxes=6, seed=1000 + i) for i in range(n)]
    bare = [(j, None, inst, name) for j, _, inst, name in samples]
    t = time.perf_counter()
    mirror = [vl.vote_labels_reference(j, inst, 1.0) for j, _, inst, _ in samples]
    mirror_s = time.perf_counter() - t
    torch.cuda.synchronize()
    t = time.perf_counter()
    store = dv.DeviceSampleStore.from_samples(bare, device=dev)
    torch.cuda.synchronize()
    build_s = time.perf_counter() - t
    equal = bool(torch.equal(store.votes.cpu().view(torch.int32), torch.from_numpy(np.concatenate(mirror)).view(torch.int32)))
    boxes = vl.ContactBoxes([vl.contact_tables(inst, 10, 1.0) for _, _, inst, _ in samples], dev)
    ms = []
    for _ in range(reps + 2):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        vl.vote_labels(store.joints, store.frame_offset, store.n_frames, boxes)
        end.record()
        torch.cuda.synchronize()
        ms.append(start.elapsed_time(end))
    k_ms = float(np.median(ms[2:]))
    items = n * frames * 53
    return {'samples': n, 'frames': frames, 'items': items, 'vote_labels_ms': round(k_ms, 4),
            'vote_labels_GBps': round(items * 52 / (k_ms * 1e-3) / 1e9, 1), 'mirror_host_s': round(mirror_s, 2),
            'store_from_bare_samples_s': round(build_s, 2), 'kernel_equals_mirror': equal}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--samples', type=int, default=384)
    ap.add_argument('--t0', type=int, nargs=2, default=[512, 2048])
    ap.add_argument('--bs', type=int, default=32)
    ap.add_argument('--frames', type=int, default=1024)
    ap.add_argument('--batches', type=int, default=12)
    ap.add_argument('--workers', type=int, nargs='*', default=[0, 4, 15])
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--train-steps', type=int, default=0)
    ap.add_argument('--only', choices=['device'], default=None, help="device loader only (for a kernel trace)")
    ap.add_argument('--kernel-reps', type=int, default=200)
    ap.add_argument('--lean', action='store_true', help="also build and time the lean store (votes='derive')")
    ap.add_argument('--store-build', type=int, nargs=2, default=None, metavar=('N', 'T'),
                    help="time p2r_vote_labels over N samples of T frames against the NumPy mirror")
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("loader_throughput needs a GPU")
    from pose2room_amd.p2rnet import P2RConfig, default_config, dataloader as dl, device_loader as dv
    from pose2room_amd.p2rnet.synthetic import make_raw_sample
    dev = torch.device('cuda:0')
    rng = np.random.default_rng(0)
    t0s = rng.integers(a.t0[0], a.t0[1] + 1, a.samples)
    samples = [make_raw_sample(int(t), n_boxes=6, seed=i) for i, t in enumerate(t0s)]
    t = time.perf_counter()
    store = dv.DeviceSampleStore.from_samples(samples, device=dev)
    torch.cuda.synchronize()
    res = {'bs': a.bs, 'frames': a.frames, 'samples': a.samples, 't0_range': list(a.t0), 'mean_t0': float(t0s.mean()),
           'device': torch.cuda.get_device_name(dev), 'cpus': len(os.sched_getaffinity(0)),
           'store_bytes': store.nbytes, 'store_build_s': round(time.perf_counter() - t, 2), 'samples_per_s': {}}

    def cfg_for(workers):
        return P2RConfig(default_config('train', data={'num_frames': a.frames}, train={'batch_size': a.bs},
                                        device={'num_workers': workers}), device=dev)

    nb = min(a.batches, a.samples // a.bs)
    devl = dv.P2RNet_device_dataloader(cfg_for(0), 'train', store)
    rate(devl.dataloader, 1, dev)                                           # warm-up: module load, allocator
    res['samples_per_s']['device'] = round(rate(devl.dataloader, nb, dev), 1)
    ids = list(range(a.bs))
    ts = []
    for _ in range(a.reps + 2):
        draws = [dl.draw_augmentation() for _ in ids]
        torch.cuda.synchronize()
        t = time.perf_counter()
        store.assemble(ids, a.frames, True, draws)
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t) * 1e3)
    res['assemble_ms'] = round(float(np.median(ts[2:])), 3)
    res['assemble_kernel_us'] = {'full': kernel_us(store, dv, dl, a.bs, a.frames, a.kernel_reps)}
    if a.lean:
        t = time.perf_counter()
        lean = dv.DeviceSampleStore.from_samples(samples, device=dev, votes='derive')
        torch.cuda.synchronize()
        res['lean'] = {'store_bytes': lean.nbytes, 'store_build_s': round(time.perf_counter() - t, 2),
                       'bytes_ratio': round(lean.nbytes / store.nbytes, 4)}
        leanl = dv.P2RNet_device_dataloader(cfg_for(0), 'train', lean)
        rate(leanl.dataloader, 1, dev)
        res['samples_per_s']['device_lean'] = round(rate(leanl.dataloader, nb, dev), 1)
        res['assemble_kernel_us']['lean'] = kernel_us(lean, dv, dl, a.bs, a.frames, a.kernel_reps)
        res['assemble_kernel_us']['full_again'] = kernel_us(store, dv, dl, a.bs, a.frames, a.kernel_reps)
    if a.store_build:
        res['store_build'] = store_build(a.store_build[0], a.store_build[1], a.reps, dev, dv, make_raw_sample)
    print(json.dumps(res), flush=True)
    if a.only == 'device':
        return
    for w in a.workers:
        cfg = cfg_for(w)
        host = dl.P2RNet_dataloader(cfg, 'train', dataset=dv.SampleListDataset(cfg, 'train', samples))
        res['samples_per_s'][f'host_w{w}'] = round(rate(host.dataloader, nb if w else min(nb, 3), dev), 1)
        print(json.dumps(res['samples_per_s']), flush=True)
    if a.train_steps:
        from pose2room_amd.p2rnet import METHODS
        from pose2room_amd.p2rnet.training import Trainer, ModuleWrapper, load_optimizer
        cfg = cfg_for(max(a.workers))
        torch.manual_seed(0)
        net = ModuleWrapper(METHODS.get('P2RNet')(cfg).to(dev)).train()
        trainer = Trainer(cfg, net, load_optimizer(cfg.config, net), dev)
        loaders = {'device': dv.P2RNet_device_dataloader(cfg, 'train', store).dataloader,
                   f'host_w{max(a.workers)}': dl.P2RNet_dataloader(
                       cfg, 'train', dataset=dv.SampleListDataset(cfg, 'train', samples)).dataloader}
        res['step_ms'] = {}
        for name, loader in loaders.items():
            n, t = 0, None
            while n < a.train_steps + 2:
                for data in loader:
                    trainer.train_step(data)
                    n += 1
                    if n == 2:
                        torch.cuda.synchronize()
                        t = time.perf_counter()
                    if n == a.train_steps + 2:
                        break
            torch.cuda.synchronize()
            res['step_ms'][name] = round((time.perf_counter() - t) * 1e3 / a.train_steps, 2)
            print(json.dumps(res['step_ms']), flush=True)
    print(json.dumps(res), flush=True)
    if a.out:
        with open(a.out, 'w') as f:
            json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
