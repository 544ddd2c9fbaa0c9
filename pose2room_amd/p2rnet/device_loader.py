"""Device-resident sample store and on-device batch assembly (csrc/batch_assemble.hip: p2r_assemble_batch).

The host loader (`dataloader.P2RNet_dataloader`) builds every sample in NumPy, one at a time, in CPU workers:
`augment_sample` + `sample_to_tensors` + `collate_fn`, then copies the batch to the GPU.  Here the raw samples sit in
HBM once and each batch is one launch:

  * `DeviceSampleStore` packs `(joints, votes, instances, name)` samples: the raw frames back to back, per-sample frame
    offset and T0, the use_height floor of each sample in both modes, and for each sample a box table with the 8
    (flip, angle) augmentation variants plus the plain one, computed with augment_sample's own node math.
  * `P2RNet_device_dataloader(cfg, mode, store)` has the sampler of `P2RNet_dataloader`, takes the augmentation draws
    on the host from the reference's generators (`dataloader.draw_augmentation`, one per sample in batch order) and
    yields batch dicts already on the device, equal bit for bit to what the host loader yields for the same seeds.

A sample may come without votes: the store derives them on the device by the reference's contact rule
(net_utils/vote_labels.py, csrc/vote_labels.hip), once at construction, or -- `votes='derive'`, the lean store, which
keeps no votes -- for every gathered item inside the assemble launch (p2r_assemble_batch_lean).

`transform_reference` is the NumPy mirror of the kernel's arithmetic (header comment of csrc/batch_assemble.hip).
"""
import ctypes
import json
import os

import numpy as np
import torch
import torch.utils.data
from torch.utils.data import DataLoader, Dataset
from torch.utils.data.distributed import DistributedSampler

from .. import _lib
from ..net_utils import vote_labels as vl
from . import dataloader as dl

ANGLES = (-np.pi, -0.5 * np.pi, 0, 0.5 * np.pi)     # the choices of draw_augmentation, in order
N_VARIANTS = 9                                      # 4 flip + angle index; 8 = no augmentation
PLAIN = N_VARIANTS - 1
MAX_T0 = 65535                                      # resample_frames' uint16 frame indices


def resample_reference(n_src, num_frames):
    """The kernel's frame index (header comment of csrc/batch_assemble.hip) -- equals dl.resample_frames."""
    if num_frames == 1:
        return np.zeros(1, np.int64)
    t = np.arange(num_frames, dtype=np.float64)
    ids = np.rint(t * (float(n_src - 1) / float(num_frames - 1)) + 0.0).astype(np.int64)
    ids[-1] = n_src - 1
    return ids


def _lin(x, M):
    """(..., 3) f64 @ (3, 3) f64 in the kernel's order: ((0 + x0 M0c) + x1 M1c) + x2 M2c.  The leading +0 is BLAS's
    zeroed accumulator in np.dot: a zero result is -0 only where a sum of -0 terms alone would keep it so, never."""
    return np.stack([((0.0 + x[..., 0] * M[0, c]) + x[..., 1] * M[1, c]) + x[..., 2] * M[2, c] for c in range(3)], -1)


def transform_reference(joints, votes, floor, augment, flip=0, rot=None, off=0.0, use_height=False):
    """NumPy mirror of the kernel's per-frame arithmetic on already gathered frames.  joints (..., 3) f32, votes
    (..., 10) f32, floor = (augmented f64 floor, plain f32 floor) -> (input_joints f32, vote_label f32, mask i64)."""
    joints = np.asarray(joints, np.float32)
    votes = np.asarray(votes, np.float32)
    mask = votes[..., 0].astype(np.int64)
    if not augment:
        j = joints
        if use_height:
            j = np.concatenate([j, (j[..., 1] - np.float32(floor[1]))[..., None]], -1)
        return j.astype(np.float32), votes[..., 1:].astype(np.float32), mask
    F = dl.FLIP_MATRIX.astype(np.float64)
    R = np.asarray(rot, np.float64)
    vs = [votes[..., 1 + 3 * k:4 + 3 * k] for k in range(3)]
    if flip:
        base = _lin(joints.astype(np.float64), F)
        vs = [_lin(v.astype(np.float64), F).astype(np.float32) for v in vs]
        ends = [_lin(base + v.astype(np.float64), R) for v in vs]
    else:
        base = joints
        ends = [_lin((joints + v).astype(np.float64), R) for v in vs]
    q = _lin(base.astype(np.float64), R)
    vote = np.concatenate([(e - q).astype(np.float32) for e in ends], -1)
    q = q + np.array([1., 0., 1.]) * off
    if use_height:
        q = np.concatenate([q, (q[..., 1] - np.float64(floor[0]))[..., None]], -1)
    return q.astype(np.float32), vote, mask


def box_variant(instances, if_flip, rot_angle):
    """augment_sample's node math (dataloader.py:31-80) without the translation: the nodes after flip / rotation."""
    rot_mat = dl.rot_y(rot_angle)
    nodes = [dict(class_id=n['class_id'], centroid=np.array(n['centroid']), R_mat=np.array(n['R_mat']),
                  size=np.array(n['size'])) for n in instances]
    if if_flip:
        for node in nodes:
            node['centroid'] = np.dot(node['centroid'], dl.FLIP_MATRIX)
            R = node['R_mat'].dot(dl.FLIP_MATRIX)
            R[2] = np.cross(R[0], R[1])
            node['R_mat'] = R
    for node in nodes:
        node['centroid'] = np.dot(node['centroid'], rot_mat)
        node['R_mat'] = node['R_mat'].dot(rot_mat)
    return nodes


def box_tables(instances, max_num_obj):
    """-> (center (9, K, 3) f64 before the offset, heading (9, K, 2) f32, size (K, 3) f32, mask (K,) f32, cls (K,) i64),
    the rows sample_to_tensors (dataloader.py:100-147) makes of each variant's nodes."""
    n = len(instances)
    if n > max_num_obj:
        raise ValueError(f"a sample has {n} boxes, more than max_num_obj = {max_num_obj}")
    center = np.zeros((N_VARIANTS, max_num_obj, 3))
    heading = np.zeros((N_VARIANTS, max_num_obj, 2), np.float32)
    size = np.zeros((max_num_obj, 3))
    mask = np.zeros(max_num_obj)
    cls = np.zeros(max_num_obj)
    variants = [box_variant(instances, f, a) for f in (0, 1) for a in ANGLES] + [instances]
    for v, nodes in enumerate(variants):
        for i, inst in enumerate(nodes):
            h = dl.rot2head(inst['R_mat'])
            row = np.hstack([inst['centroid'], np.log(inst['size']), np.sin(h), np.cos(h)])
            center[v, i] = row[0:3]
            heading[v, i] = row[6:8]
            size[i] = row[3:6]
    if n:
        mask[0:n] = 1
        cls[0:n] = [inst['class_id'] for inst in instances]
    return center, heading, size.astype(np.float32), mask.astype(np.float32), cls.astype(np.int64)


def floor_heights(joints):
    """use_height floor (dataloader.py:108-111) of a sample: in f64 after augmentation (augment_sample returns f64
    joints; flip, rotation about y and an x-z offset leave y unchanged) and in f32 without."""
    y = np.asarray(joints, np.float32)[..., 1]
    return float(np.percentile(y.astype(np.float64), 0.99)), float(np.percentile(y, 0.99))


def store_nbytes(N, F, J, K, lean):
    """Device bytes of a store of N samples / F frames: the packed frames, the per-sample rows and box tables, and the
    contact tables of a lean store."""
    return F * J * (3 if lean else 13) * 4 + \
        N * (8 + 4 + 16 + N_VARIANTS * K * (24 + 8) + K * (12 + 4 + 8)) + \
        (vl.ContactBoxes.nbytes(N, K) if lean else 0)


class DeviceSampleStore(object):
    """Raw samples packed once into device memory (layout: include/p2r_hip.h, p2r_sample_store).

    votes='store' (default) keeps a (F, J, 10) vote array next to the joints.  A sample may come without one, as
    `(joints, None, instances, name)`: its votes are then derived on the device at construction from its joints and
    object boxes (net_utils/vote_labels.py, one p2r_vote_labels launch over all such samples).

    votes='derive' is the lean store: it keeps no votes at all -- `self.votes is None` -- but the contact tables of
    the samples (`self.contact`), and `assemble` derives the vote row of every gathered item in the launch
    (p2r_assemble_batch_lean).  It holds 3 of 13 floats per (frame, joint), so 4.3 times as many samples fit under the
    same max_bytes.  It accepts samples with or without a votes array and IGNORES a given one (after checking its type
    and shape): its batches carry the votes the contact rule gives, whatever the array held."""

    def __init__(self, samples, device=None, max_num_obj=10, joint_num=53, max_bytes=None, votes='store',
                 contact_dist=None):
        """samples: iterable of (joints (T0, J, 3), votes (T0, J, 10) or None, instances, name) as `read_sample_hdf5`
        returns them plus a name; joints and votes float32.  max_bytes: refuse a store larger than this (default: half
        of the device's memory).  contact_dist: the contact distance of derived votes (default: the config's
        `dataset_config.contact_dist_thresh`, 1.0)."""
        if votes not in ('store', 'derive'):
            raise ValueError(f"DeviceSampleStore: votes must be 'store' or 'derive', got {votes!r}")
        self.lean = votes == 'derive'
        self.contact_dist = vl.default_contact_dist() if contact_dist is None else float(contact_dist)
        self.max_num_obj, self.joint_num = int(max_num_obj), int(joint_num)
        J, K = self.joint_num, self.max_num_obj
        joints, votes, t0, names, floors, tables, contact = [], [], [], [], [], [], []
        for i, (j, v, inst, name) in enumerate(samples):
            j, v = np.asarray(j), None if v is None else np.asarray(v)
            if j.dtype != np.float32 or (v is not None and v.dtype != np.float32):
                raise ValueError(f"sample {i} ({name}): joints and votes must be float32, got {j.dtype} / "
                                 f"{getattr(v, 'dtype', None)}")
            if j.ndim != 3 or j.shape[1:] != (J, 3) or (v is not None and v.shape != j.shape[:2] + (10,)):
                raise ValueError(f"sample {i} ({name}): joints (T0, {J}, 3) and votes (T0, {J}, 10) expected, got "
                                 f"{j.shape} / {getattr(v, 'shape', None)}")
            if not 1 <= j.shape[0] <= MAX_T0:
                raise ValueError(f"sample {i} ({name}): T0 = {j.shape[0]} frames, outside 1..{MAX_T0} (the "
                                 "reference's frame indices are uint16)")
            joints.append(j)
            votes.append(None if self.lean else v)
            t0.append(j.shape[0])
            names.append(name)
            floors.append(floor_heights(j))
            tables.append(box_tables(inst, K))
            contact.append(vl.contact_tables(inst, K, self.contact_dist, name=f"{i} ({name})")
                           if self.lean or v is None else None)
        if not t0:
            raise ValueError("DeviceSampleStore: no samples")
        N, F = len(t0), int(sum(t0))
        self.nbytes = store_nbytes(N, F, J, K, self.lean)
        if max_bytes is not None and self.nbytes > max_bytes:
            raise MemoryError(f"DeviceSampleStore: {N} samples / {F} frames need {self.nbytes} bytes of device memory, "
                              f"above the cap of {max_bytes} bytes (max_bytes)")
        device = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
        if device.type != 'cuda':
            raise RuntimeError("DeviceSampleStore: the store lives on a GPU")
        if max_bytes is None and self.nbytes > torch.cuda.get_device_properties(device).total_memory // 2:
            raise MemoryError(f"DeviceSampleStore: {N} samples / {F} frames need {self.nbytes} bytes of device memory, "
                              "above half of the device's memory (pass max_bytes to allow more)")
        self.device = device
        off = np.zeros(N, np.int64)
        off[1:] = np.cumsum(t0)[:-1]
        put = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
        self.joints = put(np.concatenate(joints))
        self.frame_offset = put(off)
        self.n_frames = put(np.asarray(t0, np.int32))
        self.contact = vl.ContactBoxes(contact, device) if self.lean else None
        self.votes = None if self.lean else self._votes(votes, contact, off, t0, put)
        self.floor_height = put(np.asarray(floors, np.float64))
        self.box_center, self.box_heading, self.box_size, self.box_mask, self.box_cls = \
            [put(np.stack([t[k] for t in tables])) for k in range(5)]
        self.names = names
        self.T0 = np.asarray(t0)
        self._c = _Store(joints=self.joints.data_ptr(), votes=0 if self.lean else self.votes.data_ptr(),
                         frame_offset=self.frame_offset.data_ptr(), n_frames=self.n_frames.data_ptr(),
                         floor_height=self.floor_height.data_ptr(), box_center=self.box_center.data_ptr(),
                         box_heading=self.box_heading.data_ptr(), box_size=self.box_size.data_ptr(),
                         box_mask=self.box_mask.data_ptr(), box_cls=self.box_cls.data_ptr(), n_frames_total=F,
                         n_samples=N, J=J, K=K)

    def _votes(self, votes, contact, off, t0, put):
        """The packed (F, J, 10) votes: the given arrays copied, the missing ones derived on the device in ONE launch
        over the pack of the samples that came without."""
        missing = [i for i, v in enumerate(votes) if v is None]
        if not missing:
            return put(np.concatenate(votes))
        boxes = vl.ContactBoxes([contact[i] for i in missing], self.device)
        if len(missing) == len(votes):
            return vl.vote_labels(self.joints, self.frame_offset, self.n_frames, boxes)
        J = self.joint_num
        out = put(np.concatenate([np.zeros((t, J, 10), np.float32) if v is None else v for v, t in zip(votes, t0)]))
        sub_t0 = np.asarray([t0[i] for i in missing], np.int32)
        sub_off = np.zeros(len(missing), np.int64)
        sub_off[1:] = np.cumsum(sub_t0)[:-1]
        derived = vl.vote_labels(torch.cat([self.joints[off[i]:off[i] + t0[i]] for i in missing]), put(sub_off),
                                 put(sub_t0), boxes)
        for i, o in zip(missing, sub_off):
            out[off[i]:off[i] + t0[i]] = derived[o:o + t0[i]]
        return out

    def __len__(self):
        return len(self.names)

    @classmethod
    def from_samples(cls, samples, **kw):
        return cls(samples, **kw)

    @classmethod
    def from_split(cls, cfg, mode, **kw):
        """The samples of `<split>/<mode>.json` read with `read_sample_hdf5` (P2RNet_VirtualHome's file list)."""
        with open(os.path.join(cfg.config['data']['split'], mode + '.json')) as f:
            paths = json.load(f)

        def gen():
            for path in paths:
                joints, votes, instances = dl.read_sample_hdf5(path)
                yield joints, votes, instances, '.'.join(os.path.basename(path).split('.')[:-1])
        kw.setdefault('max_num_obj', cfg.config['data']['max_gt_boxes'])
        kw.setdefault('joint_num', cfg.dataset_config.joint_num)
        return cls(gen(), **kw)

    @classmethod
    def from_recordings(cls, recordings, aug_indices=range(8), votes='store', device=None, max_num_obj=10,
                        joint_num=53, max_bytes=None, contact_dist=None, repair=None, on_unrepairable='raise'):
        """The store of the samples that stage 3 of the reference's data preparation makes of raw recordings
        (net_utils/sample_build.py: trim, reject, recentre, the variants `aug_indices`, the votes), built on the device:
        no sample file, no host copy of a frame and no `floor_heights` -- the floors are p2r_floor_percentile's.  Equal,
        tensor for tensor, to `DeviceSampleStore(build_reference(r).samples of every kept r, ...)`.  `recordings`: dicts
        of joints (F, J, 3) float64, room_bbox, object_nodes and name.  `self.rejected` lists the (name, reason) of the
        recordings that gave no sample, `self.kept` the indices of the others.
        max_bytes (default: half of the device's memory) is checked before anything is allocated, against the size the
        store would have if no frame were trimmed and no recording rejected: a store that would fit only after trimming
        is refused.  The packed float64 copy of the recordings that lives during the build (24 bytes per input (frame,
        joint)) is not counted; `self.nbytes` is the size of the finished store.
        repair, on_unrepairable: `build_samples`' -- a `RepairSpec` fills the missing joints of the recordings on the
        device first (net_utils/recording_repair.py); `self.repair` then holds the statistics (R, 4) of every recording
        given, None without."""
        from ..net_utils import sample_build as sb
        if votes not in ('store', 'derive'):
            raise ValueError(f"DeviceSampleStore: votes must be 'store' or 'derive', got {votes!r}")
        device = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
        if device.type != 'cuda':
            raise RuntimeError("DeviceSampleStore: the store lives on a GPU")
        self = cls.__new__(cls)
        self.lean = votes == 'derive'
        self.contact_dist = vl.default_contact_dist() if contact_dist is None else float(contact_dist)
        self.max_num_obj, self.joint_num = int(max_num_obj), int(joint_num)
        J, K = self.joint_num, self.max_num_obj
        recordings, aug_indices = list(recordings), list(aug_indices)
        for i, r in enumerate(recordings):
            if r['joints'].ndim != 3 or tuple(r['joints'].shape[1:]) != (J, 3):
                raise ValueError(f"recording {i} ({r['name']}): joints (F, {J}, 3) expected, got "
                                 f"{tuple(r['joints'].shape)}")
        # what the build would allocate at most (no frame trimmed), before anything is allocated
        N_max = len(recordings) * len(aug_indices)
        F_max = sum(int(r['joints'].shape[0]) for r in recordings) * len(aug_indices)
        size = lambda N, F: store_nbytes(N, F, J, K, self.lean)                         # noqa: E731
        cap = torch.cuda.get_device_properties(device).total_memory // 2 if max_bytes is None else max_bytes
        if size(N_max, F_max) > cap:
            raise MemoryError(f"DeviceSampleStore: {N_max} samples / {F_max} frames need up to {size(N_max, F_max)} "
                              f"bytes of device memory, above the cap of {cap} bytes (max_bytes)")
        built = sb.build_samples(recordings, aug_indices, contact_dist=self.contact_dist, device=device,
                                 votes=not self.lean, max_num_obj=K, repair=repair, on_unrepairable=on_unrepairable)
        self.repair = getattr(built, 'repair', None)
        if not built.names:
            raise ValueError(f"DeviceSampleStore: no samples (every recording was rejected: {built.rejected})")
        N, F = len(built.names), int(built.joints.shape[0])
        self.nbytes = size(N, F)
        self.device = device
        put = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)          # noqa: E731
        self.joints, self.votes = built.joints, built.votes
        self.frame_offset, self.n_frames = built.frame_offset, built.n_frames
        self.contact = built.contact if self.lean else None
        self.floor_height = built.floors
        tables = [box_tables(inst, K) for inst in built.instances]
        self.box_center, self.box_heading, self.box_size, self.box_mask, self.box_cls = \
            [put(np.stack([t[k] for t in tables])) for k in range(5)]
        self.names = built.names
        self.kept, self.rejected = built.kept, built.rejected
        per = len(built.names) // len(built.kept)
        self.T0 = np.repeat([int(recordings[i]['joints'].shape[0]) - f for i, f in zip(built.kept, built.first)], per)
        self._c = _Store(joints=self.joints.data_ptr(), votes=0 if self.lean else self.votes.data_ptr(),
                         frame_offset=self.frame_offset.data_ptr(), n_frames=self.n_frames.data_ptr(),
                         floor_height=self.floor_height.data_ptr(), box_center=self.box_center.data_ptr(),
                         box_heading=self.box_heading.data_ptr(), box_size=self.box_size.data_ptr(),
                         box_mask=self.box_mask.data_ptr(), box_cls=self.box_cls.data_ptr(), n_frames_total=F,
                         n_samples=N, J=J, K=K)
        return self

    def assemble(self, ids, num_frames, augment=False, draws=None, use_height=False):
        """One batch of samples `ids` -> the collate_fn dict on the store's device (sample_idx: list of names).
        draws: one (if_flip, rot_angle, offset_scale) per sample when augment."""
        ids = [int(i) for i in ids]
        N = len(self.names)
        if any(i < 0 or i >= N for i in ids):
            raise RuntimeError(f"assemble_batch: sample ids must lie in 0..{N - 1}, got {ids}")
        B, T, J, K = len(ids), int(num_frames), self.joint_num, self.max_num_obj
        sel = np.zeros((B, 3), np.int64)
        sel[:, 0] = ids
        aug = None
        if augment:
            if draws is None or len(draws) != B:
                raise RuntimeError("assemble_batch: augmentation needs one draw per sample")
            aug = np.zeros((B, 10))
            for b, (flip, angle, off) in enumerate(draws):
                sel[b, 1], sel[b, 2] = int(flip), 4 * int(flip) + ANGLES.index(angle)
                aug[b, 0:9] = dl.rot_y(angle).reshape(9)
                aug[b, 9] = off
        dev = self.device
        out = {'input_joints': torch.empty((B, T, J, 4 if use_height else 3), dtype=torch.float32, device=dev),
               'box_label_mask': torch.empty((B, K), dtype=torch.float32, device=dev),
               'sem_cls_label': torch.empty((B, K), dtype=torch.int64, device=dev),
               'center_label': torch.empty((B, K, 3), dtype=torch.float32, device=dev),
               'size': torch.empty((B, K, 3), dtype=torch.float32, device=dev),
               'heading': torch.empty((B, K, 2), dtype=torch.float32, device=dev),
               'vote_label': torch.empty((B, T, J, 9), dtype=torch.float32, device=dev),
               'vote_label_mask': torch.empty((B, T, J), dtype=torch.int64, device=dev)}
        assemble_batch(self, torch.from_numpy(sel).to(dev, non_blocking=True),
                       None if aug is None else torch.from_numpy(aug).to(dev, non_blocking=True), augment, use_height,
                       T, out)
        out['sample_idx'] = [self.names[i] for i in ids]
        return out


_Store, _Out = _lib.struct('p2r_sample_store'), _lib.struct('p2r_batch_out')


def assemble_batch(store, sel, aug, augment, use_height, num_frames, out):
    """Thin binding of p2r_assemble_batch (p2r_assemble_batch_lean for a lean store): sel (B, 3) i64 and aug (B, 10)
    f64 (or None) on the store's device, out the dict of preallocated outputs.  Ids are the caller's to check (DeviceSampleStore.assemble does)."""
    tensors = [sel] + ([] if aug is None else [aug]) + list(out.values())
    if not all(torch.is_tensor(t) and t.is_cuda and t.device == store.device and t.is_contiguous() for t in tensors):
        raise RuntimeError(f"assemble_batch: every tensor must be contiguous on {store.device}")
    if sel.dtype != torch.int64 or sel.dim() != 2 or sel.shape[1] != 3 or \
            (aug is not None and (aug.dtype != torch.float64 or aug.shape != (sel.shape[0], 10))):
        raise RuntimeError("assemble_batch: sel (B, 3) int64 and aug (B, 10) float64 expected")
    o = _Out(**{f[0]: out[f[0]].data_ptr() for f in _Out._fields_})
    if store.lean:      # no stored votes: the launch derives them from the contact tables
        vl.assemble_batch_lean(store.device, ctypes.byref(store._c), store.contact, int(sel.shape[0]), sel, aug,
                               int(bool(augment)), int(bool(use_height)), int(num_frames), ctypes.byref(o))
        return out
    _lib.launch("p2r_assemble_batch", store.device, ctypes.byref(store._c), int(sel.shape[0]), sel, aug, int(bool(augment)),
                int(bool(use_height)), int(num_frames), ctypes.byref(o))
    return out


class SampleListDataset(Dataset):
    """`P2RNet_VirtualHome.__getitem__` (dataloader.py) over in-memory `(joints, votes, instances, name)` samples: the
    host path the device loader is measured and checked against."""

    def __init__(self, cfg, mode, samples):
        self.samples = list(samples)
        self.aug = mode == 'train'
        self.num_frames = cfg.config['data']['num_frames']
        self.use_height = not cfg.config['data']['no_height']
        self.max_num_obj = cfg.config['data']['max_gt_boxes']

    def __len__(self):
        return len(self.samples)

    def __getitem__(self, idx):
        joints, votes, instances, name = self.samples[idx]
        if self.aug:
            joints, instances, votes = dl.augment_sample(joints, instances, votes, *dl.draw_augmentation())
        return dl.sample_to_tensors(joints, votes, instances, self.num_frames, self.max_num_obj, self.use_height, name)


class _Indices(Dataset):
    def __init__(self, n):
        self.n = n

    def __len__(self):
        return self.n

    def __getitem__(self, idx):
        return idx


class DeviceBatchLoader(object):
    """Iterable of device batch dicts over the batches of `batch_sampler`.  The indices come through a torch DataLoader
    without workers, so the sampler sees the same generator state as the host loader's."""

    def __init__(self, store, batch_sampler, num_frames, augment, use_height):
        self.store, self.num_frames, self.augment, self.use_height = store, num_frames, augment, use_height
        self.batch_sampler = batch_sampler
        self.index_loader = DataLoader(_Indices(len(store)), batch_sampler=batch_sampler, num_workers=0,
                                       collate_fn=list)

    def __len__(self):
        return len(self.index_loader)

    def __iter__(self):
        for ids in self.index_loader:
            draws = [dl.draw_augmentation() for _ in ids] if self.augment else None
            yield self.store.assemble(ids, self.num_frames, self.augment, draws, self.use_height)


def P2RNet_device_dataloader(cfg, mode, store, sampler=None):
    """`P2RNet_dataloader` over a DeviceSampleStore: same sampler choice (DistributedSampler under DDP, random for
    'train', sequential otherwise; `sampler` overrides it), same batch size, augmentation in 'train' mode with the
    reference's draws.  Returns the (dataloader, sampler) pair the epoch loops expect."""
    if cfg.config['data']['dataset'] != 'virtualhome':
        raise NotImplementedError
    if store.max_num_obj != cfg.config['data']['max_gt_boxes']:
        raise ValueError(f"store built for max_num_obj = {store.max_num_obj}, config has max_gt_boxes = "
                         f"{cfg.config['data']['max_gt_boxes']}")
    index = _Indices(len(store))
    if sampler is None:
        if cfg.config['device']['distributed']:
            sampler = DistributedSampler(index, shuffle=(mode == 'train'))
        elif mode == 'train':
            sampler = torch.utils.data.RandomSampler(index)
        else:
            sampler = torch.utils.data.SequentialSampler(index)
    batch_sampler = torch.utils.data.BatchSampler(sampler, batch_size=cfg.config[mode]['batch_size'], drop_last=False)
    loader = DeviceBatchLoader(store, batch_sampler, cfg.config['data']['num_frames'], mode == 'train',
                               not cfg.config['data']['no_height'])
    return dl.Custom_Dataloader(loader, sampler)
