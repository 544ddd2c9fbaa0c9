"""Sample loader throughput at bs=32, T=1024 (one GPU): the host loader against the device sample store.

    python tools/loader_throughput.py [--samples 384] [--t0 512 2048] [--batches 12] [--workers 0 4 15]
                                      [--train-steps 20] [--only device] [--out profiles/loader_throughput.json]

Raw samples are synthetic (p2rnet/synthetic.make_raw_sample, six boxes), T0 drawn uniformly from the --t0 range.
Timed, with a device synchronisation at the end of each measurement, in 'train' mode (augmentation on):
  host_w<N>     P2RNet_dataloader over the samples in host memory (dataloader.py: augment_sample + sample_to_tensors +
                collate_fn in N worker processes), each batch copied to the GPU as Trainer.to_device does; timed from
                the start of the epoch (worker start-up included) to the last batch
  device        P2RNet_device_dataloader over a DeviceSampleStore of the same samples (one launch per batch)
  assemble_ms   one DeviceSampleStore.assemble call at bs, T, median of --reps (host draws + launch, synchronised)
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
