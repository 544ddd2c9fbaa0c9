"""The scene read-out of a batch on the device: object nodes, contact frames and unique frames.

The reference's entry point for the user of a trained model is demo.py (`predict` / `visualize_step`, lines 204-266): a
pose recording goes in, and the objects of the room come out as `object_node` dicts -- centroid, R_mat, size, class_id --
together with the input frames without duplicates (`np.unique(..., axis=0, return_index=True)`) and, for every object, the
frame in which the body is closest to it (`dist_node2bbox`, utils/virtualhome/vis_gt_vh.py:14-22).  There all of it is a
host loop per sample and per object.  Here it is three launches for the whole batch and all hypotheses
(csrc/scene.hip, include/p2r_scene.h):

  * `scene_nodes`    (p2r_scene_nodes): the confident boxes of every sample, compacted to slots 0 .. count-1 in ascending
                     proposal index, with `head2rot` of the heading;
  * `contact_frames` (p2r_contact_frames): `dist_node2bbox` for every node of every sample -- the first frame that attains
                     the minimum over frames of the maximum over joints and box axes of |R (x - c)| - size / 2;
  * `unique_frames`  (p2r_unique_frames): the ascending first-occurrence indices of the distinct frames of every sample,
                     and for every frame its position in that list.

`scenes_from_parsed` chains them behind `parse_predictions(..., return_device=True)` and `mm_device.box_params`;
`P2RNet.predict_scenes` is the public entry.  `SceneBatch` holds the device tensors and crosses to the host once, when a
caller asks for dicts, records or files.  No CPU fallback.
"""
import numpy as np
import torch

from .. import _lib

MAX_K, MAX_T, MAX_J = 1024, 65535, 64      # P2R_SCENE_MAX_K / _T / _J of include/p2r_scene.h
UNIQUE_MAX_T = 4096                        # P2R_UNIQUE_MAX_T: three int tables of T entries in LDS

# The kernels are a library of their own next to libp2r_hip.so (csrc/Makefile), with a header of their own; the binding
# is derived from that header as that of libp2r_hip.so is (_lib.Library).
_library = _lib.extension("scene")
HEADER_PATH, LIB_PATH = _library.header_path, _library.lib_path
lib, _launch = _library.lib, _library.launch


def _want(what, name, t, dtype, shape):
    """shape and dtype first (a ValueError, whatever the device), then the device (no CPU fallback)"""
    if not torch.is_tensor(t) or t.dtype != dtype or tuple(t.shape) != tuple(shape):
        got = f"{t.dtype} {tuple(t.shape)}" if torch.is_tensor(t) else type(t).__name__
        raise ValueError(f"{what}: {name} must be {dtype} of shape {tuple(shape)}, got {got}")
    return t


def _on_gpu(what, **tensors):
    """-> the tensors contiguous; all of them on one GPU"""
    for name, t in tensors.items():
        if not t.is_cuda:
            raise RuntimeError(f"{what}: {name} must be a GPU tensor (no CPU fallback)")
    if len({t.device for t in tensors.values()}) > 1:
        raise RuntimeError(f"{what}: all tensors must be on one device")
    return [t.contiguous() for t in tensors.values()]


def _want_joints(what, joints, max_t):
    if not torch.is_tensor(joints) or joints.dtype != torch.float32 or joints.dim() != 4 or joints.shape[-1] not in (3, 4):
        got = f"{joints.dtype} {tuple(joints.shape)}" if torch.is_tensor(joints) else type(joints).__name__
        raise ValueError(f"{what}: joints must be float32 (B,T,J,3|4), got {got}")
    B, T, J, C = joints.shape
    if not (1 <= T <= max_t and 1 <= J <= MAX_J):
        raise ValueError(f"{what}: 1..{max_t} frames of 1..{MAX_J} joints, got T={T}, J={J}")
    return joints


def scene_nodes(obbs, obj_prob, pred_mask, pred_cls, dump_threshold):
    """obbs (N,K,7) f64 (`mm_device.box_params`), obj_prob (N,K) f32, pred_mask (N,K) u8, pred_cls (N,K) i64, on one GPU
    -> (count (N) i32, inst_idx (N,K) i32, node_obbs (N,K,7) f64, node_rmat (N,K,3,3) f64, node_cls (N,K) i64,
    node_score (N,K) f32): the proposals with (double)obj_prob > dump_threshold and pred_mask == 1, in ascending
    proposal index in slots 0 .. count-1; the other slots are zero with inst_idx = -1.  One launch."""
    what = "scene_nodes"
    if not torch.is_tensor(obbs) or obbs.dim() != 3 or obbs.shape[-1] != 7:
        raise ValueError(f"{what}: obbs must be (N,K,7)")
    N, K = obbs.shape[:2]
    if K > MAX_K or N * K > 0x7fffffff:
        raise ValueError(f"{what}: at most {MAX_K} proposals per sample and 2^31-1 in all, got N={N}, K={K}")
    _want(what, "obbs", obbs, torch.float64, (N, K, 7))
    _want(what, "obj_prob", obj_prob, torch.float32, (N, K))
    _want(what, "pred_mask", pred_mask, torch.uint8, (N, K))
    _want(what, "pred_cls", pred_cls, torch.int64, (N, K))
    obbs, obj_prob, pred_mask, pred_cls = _on_gpu(what, obbs=obbs, obj_prob=obj_prob, pred_mask=pred_mask,
                                                  pred_cls=pred_cls)
    dev = obbs.device
    count = torch.empty((N,), dtype=torch.int32, device=dev)
    inst_idx = torch.empty((N, K), dtype=torch.int32, device=dev)
    node_obbs = torch.empty((N, K, 7), dtype=torch.float64, device=dev)
    node_rmat = torch.empty((N, K, 3, 3), dtype=torch.float64, device=dev)
    node_cls = torch.empty((N, K), dtype=torch.int64, device=dev)
    node_score = torch.empty((N, K), dtype=torch.float32, device=dev)
    _launch("p2r_scene_nodes", dev, N, K, obbs, obj_prob, pred_mask, pred_cls, float(dump_threshold), count, inst_idx,
            node_obbs, node_rmat, node_cls, node_score)
    return count, inst_idx, node_obbs, node_rmat, node_cls, node_score


def contact_frames(joints, node_obbs, node_rmat, count):
    """joints (B,T,J,3|4) f32, node_obbs (N,K,7) f64, node_rmat (N,K,3,3) f64, count (N) i32 as `scene_nodes` returns
    them (or ground-truth nodes with their stored R_mat), N % B == 0 (sample n reads joints row n % B)
    -> (frame (N,K) i32, dist (N,K) f64): for every slot below count the first frame that attains the smallest box
    distance of the body and that distance; -1 and 0 in the other slots.  One launch."""
    what = "contact_frames"
    joints = _want_joints(what, joints, MAX_T)
    if not torch.is_tensor(node_obbs) or node_obbs.dim() != 3 or node_obbs.shape[-1] != 7:
        raise ValueError(f"{what}: node_obbs must be (N,K,7)")
    N, K = node_obbs.shape[:2]
    B, T, J, C = joints.shape
    if B < 1 or N % B != 0:
        raise ValueError(f"{what}: {N} samples over {B} joints rows: N must be a multiple of B")
    if K > MAX_K or N * K > 0x7fffffff:
        raise ValueError(f"{what}: at most {MAX_K} nodes per sample and 2^31-1 in all, got N={N}, K={K}")
    _want(what, "node_obbs", node_obbs, torch.float64, (N, K, 7))
    _want(what, "node_rmat", node_rmat, torch.float64, (N, K, 3, 3))
    _want(what, "count", count, torch.int32, (N,))
    joints, node_obbs, node_rmat, count = _on_gpu(what, joints=joints, node_obbs=node_obbs, node_rmat=node_rmat,
                                                  count=count)
    dev = joints.device
    frame = torch.empty((N, K), dtype=torch.int32, device=dev)
    dist = torch.empty((N, K), dtype=torch.float64, device=dev)
    _launch("p2r_contact_frames", dev, joints, B, T, J, C, N, K, node_obbs, node_rmat, count, frame, dist)
    return frame, dist


def unique_frames(joints):
    """joints (B,T,J,3|4) f32 with T <= 4096 -> (count (B) i32, index (B,T) i32, rank (B,T) i32):
    `np.sort(np.unique(joints[b], axis=0, return_index=True)[1])` of every sample in index[b, :count[b]] (-1 behind it),
    and the position in that list of the first occurrence of every frame's row.  Rows are equal iff all their elements
    are ==: -0.0 equals +0.0, a row with a NaN equals no row.  One launch."""
    what = "unique_frames"
    joints = _want_joints(what, joints, UNIQUE_MAX_T)
    B, T, J, C = joints.shape
    joints, = _on_gpu(what, joints=joints)
    dev = joints.device
    count = torch.empty((B,), dtype=torch.int32, device=dev)
    index = torch.empty((B, T), dtype=torch.int32, device=dev)
    rank = torch.empty((B, T), dtype=torch.int32, device=dev)
    _launch("p2r_unique_frames", dev, joints, B, T, J, C, count, index, rank)
    return count, index, rank


def records_from_nodes(count, inst_idx, node_obbs, node_cls, K=None):
    """Host arrays of `scene_nodes` -> the list `multi_modal_eval.confident_boxes` returns: per sample {'obbs' (M,7) f64,
    'cls' (M,) i64, 'inst_idx' (K,) bool}."""
    out = []
    for n in range(len(count)):
        m = int(count[n])
        keep = np.zeros(inst_idx.shape[1] if K is None else K, dtype=bool)
        keep[inst_idx[n, :m]] = True
        out.append({'obbs': np.array(node_obbs[n, :m], dtype=np.float64), 'cls': np.array(node_cls[n, :m]),
                    'inst_idx': keep})
    return out


class SceneBatch(object):
    """The scenes of N = H * B samples (hypothesis-major: sample n = h * B + b) of K proposals, on the device.
    Tensors: count (N) i32, inst_idx (N,K) i32, node_obbs (N,K,7) f64, node_rmat (N,K,3,3) f64, node_cls (N,K) i64,
    node_score (N,K) f32 (`scene_nodes`); contact_frame (N,K) i32 and contact_dist (N,K) f64 (`contact_frames`), or None;
    unique_count (B) i32, unique_index (B,T) i32, unique_rank (B,T) i32 (`unique_frames`), or None.  Nothing is copied
    to the host before `nodes`, `records` or `save_npz` is called; the first of them copies everything once."""

    _FIELDS = ('count', 'inst_idx', 'node_obbs', 'node_rmat', 'node_cls', 'node_score', 'contact_frame', 'contact_dist',
               'unique_count', 'unique_index', 'unique_rank')

    def __init__(self, H, B, K, count, inst_idx, node_obbs, node_rmat, node_cls, node_score, contact_frame=None,
                 contact_dist=None, unique_count=None, unique_index=None, unique_rank=None):
        self.H, self.B, self.K = int(H), int(B), int(K)
        self.count, self.inst_idx, self.node_obbs, self.node_rmat = count, inst_idx, node_obbs, node_rmat
        self.node_cls, self.node_score = node_cls, node_score
        self.contact_frame, self.contact_dist = contact_frame, contact_dist
        self.unique_count, self.unique_index, self.unique_rank = unique_count, unique_index, unique_rank
        if tuple(count.shape) != (self.H * self.B,) or tuple(inst_idx.shape) != (self.H * self.B, self.K):
            raise ValueError(f"SceneBatch: count ({self.H * self.B},) and inst_idx ({self.H * self.B},{self.K}) expected, "
                             f"got {tuple(count.shape)} and {tuple(inst_idx.shape)}")
        self._host_arrays = None

    def __len__(self):
        return self.H * self.B

    def host(self):
        """-> {field: ndarray} of the tensors that are present (one synchronisation, cached)"""
        if self._host_arrays is None:
            from .ap_helper import _to_host
            names = [f for f in self._FIELDS if getattr(self, f) is not None]
            self._host_arrays = dict(zip(names, _to_host([getattr(self, f) for f in names])))
        return self._host_arrays

    def sample(self, b, h=0):
        """index of sample b of hypothesis h in the stack"""
        if not (0 <= h < self.H and 0 <= b < self.B):
            raise IndexError(f"SceneBatch: hypothesis {h} / sample {b} outside {self.H} x {self.B}")
        return h * self.B + b

    def nodes(self, n):
        """-> the `object_node` dicts of sample n as demo.py:242-254 builds them -- 'centroid' (3,), 'R_mat' (3,3), 'size'
        (3,), 'class_id' [cls] -- each with 'score', 'inst_idx' (its proposal index) and, where they were computed,
        'contact_frame' (a frame of the recording), 'contact_dist' and 'contact_frame_unique' (the same frame's position
        in the de-duplicated sequence that the demo indexes)."""
        z = self.host()
        out = []
        for s in range(int(z['count'][n])):
            node = {'centroid': z['node_obbs'][n, s, 0:3].copy(), 'R_mat': z['node_rmat'][n, s].copy(),
                    'size': z['node_obbs'][n, s, 3:6].copy(), 'class_id': [z['node_cls'][n, s]],
                    'score': float(z['node_score'][n, s]), 'inst_idx': int(z['inst_idx'][n, s])}
            if 'contact_frame' in z:
                t = int(z['contact_frame'][n, s])
                node['contact_frame'], node['contact_dist'] = t, float(z['contact_dist'][n, s])
                if 'unique_rank' in z:
                    node['contact_frame_unique'] = int(z['unique_rank'][n % self.B, t])
            out.append(node)
        return out

    def unique(self, b):
        """-> the ascending first-occurrence frame indices of sample b of the batch (what demo.py:234-235 sorts)"""
        z = self.host()
        if 'unique_index' not in z:
            raise RuntimeError("SceneBatch: the unique frames were not computed (unique=False)")
        return z['unique_index'][b, :int(z['unique_count'][b])].copy()

    def records(self, h=None):
        """-> what `multi_modal_eval.confident_boxes` returns for the same inputs: per sample {'obbs' (M,7) f64, 'cls'
        (M,) i64, 'inst_idx' (K,) bool}; all N samples in stack order, or the B samples of hypothesis h."""
        z = self.host()
        out = records_from_nodes(z['count'], z['inst_idx'], z['node_obbs'], z['node_cls'], self.K)
        return out if h is None else out[self.sample(0, h):self.sample(0, h) + self.B]

    def consensus(self, iou_thresh=0.25, class_aware=True):
        """-> consensus_device.ConsensusBatch: the H scenes of every sample merged into one by greedy-leader clustering of
        their oriented boxes (two launches, nothing crosses to the host).  H = 1 is valid: every cluster has support 1
        unless boxes of the one scene overlap."""
        from . import consensus_device
        return consensus_device.consensus_of(self, iou_thresh, class_aware)

    def occupancy(self, grid, joints=None, gt=None, min_votes=None, owner=False):
        """-> occupancy_device.OccupancyBatch: the voxels of `grid` (an occupancy_device.Grid) that the nodes of every
        sample cover, the votes of the H hypotheses per voxel and the map of the voxels with min_votes (default
        H // 2 + 1) or more; with joints (B,T,J,3|4) the body's voxels, with gt (a SceneBatch of the B ground-truth
        scenes) the scene IoU.  At most 7 launches, nothing crosses to the host."""
        from . import occupancy_device
        return occupancy_device.occupancy_of(self, grid, joints=joints, gt=gt, min_votes=min_votes, owner=owner)

    def interactions(self, joints, contact_thresh=None, merge_gap=0, min_len=1, max_intervals=16, labels=True):
        """-> interaction_device.InteractionBatch: per node the frames of joints (B,T,J,3|4) in which the body is inside
        the node's box enlarged by contact_thresh (default: the distance the training labels use), as bit-packed frames
        and as intervals merged over gaps of at most merge_gap frames and at least min_len long, the joints that touch
        it, and with labels one node per frame.  Three launches (two without labels), nothing crosses to the host."""
        from . import interaction_device
        return interaction_device.interactions_of(self, joints, contact_thresh=contact_thresh, merge_gap=merge_gap,
                                                  min_len=min_len, max_intervals=max_intervals, labels=labels)

    def save_npz(self, path, n):
        """Sample n in the layout of the reference's `%06d_pred_confident_nms_bbox.npz` (testing.py:132-134: obbs, cls,
        inst_idx), which its `read_pred` reads.  -> True, or False for a sample without nodes: the reference writes no
        file for it."""
        rec = self.records()[n]
        if not rec['inst_idx'].any():
            return False
        np.savez(path, obbs=rec['obbs'], cls=rec['cls'], inst_idx=rec['inst_idx'])
        return True


def scenes_from_parsed(pred_corners_3d, obj_prob, pred_mask, pred_sem_cls, joints, dump_threshold=0.5, contact=True,
                       unique=True, num_hypotheses=1):
    """The device results of `parse_predictions(..., return_device=True)` for N = H * B samples -- pred_corners_3d
    (N,K,8,3) f64, obj_prob (N,K) f32, pred_mask (N,K) u8, pred_sem_cls (N,K) i64 -- and the batch's joints (B,T,J,3|4)
    f32 -> SceneBatch.  Four launches (box parameters, nodes, contact frames, unique frames), no copy to the host."""
    from . import mm_device
    what = "scenes_from_parsed"
    if not torch.is_tensor(pred_corners_3d) or pred_corners_3d.dim() != 4:
        raise ValueError(f"{what}: pred_corners_3d must be (N,K,8,3)")
    N, K = pred_corners_3d.shape[:2]
    H = int(num_hypotheses)
    if H < 1 or N % H != 0:
        raise ValueError(f"{what}: {N} samples are no stack of {H} hypotheses")
    B = N // H
    if (contact or unique) and (not torch.is_tensor(joints) or joints.dim() != 4 or joints.shape[0] != B):
        raise ValueError(f"{what}: joints must be ({B},T,J,3|4), one row per sample of the batch")
    obbs = mm_device.box_params(pred_corners_3d)
    nodes = scene_nodes(obbs, obj_prob, pred_mask.to(torch.uint8), pred_sem_cls.to(torch.int64), dump_threshold)
    count, _, node_obbs, node_rmat = nodes[:4]
    frame = dist = ucount = uindex = urank = None
    if contact:
        frame, dist = contact_frames(joints, node_obbs, node_rmat, count)
    if unique:
        ucount, uindex, urank = unique_frames(joints)
    return SceneBatch(H, B, K, *nodes, frame, dist, ucount, uindex, urank)
