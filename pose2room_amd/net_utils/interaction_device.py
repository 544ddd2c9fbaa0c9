"""The interaction timeline of predicted scenes, on the device: during which frames the body is in contact with which
object node, and with which joints.

Everything else a trained model reports is spatial -- boxes (`predict_scenes`), an agreed scene (`predict_consensus`),
voxels (`predict_occupancy`) -- and the one temporal fact is a single frame per node (`contact_frame`).  This module
applies the project's rule for "in contact", the enlarged-box test of the reference's `get_votes`
(utils/virtualhome/3_generate_samples.py:56-64, the expression of include/p2r_vote_labels.h), to every node of a
`SceneBatch` in every frame, and turns the per-frame answer into intervals:

  * `contact_bits`      (p2r_contact_bits): per node the frames in which a joint is inside the enlarged box, bit-packed,
                        per frame how many joints are, and over the recording which joints ever are;
  * `contact_intervals` (p2r_contact_intervals): the runs of those frames, merged over gaps of at most `merge_gap`
                        frames, then without the runs shorter than `min_len`;
  * `frame_labels`      (p2r_frame_labels): per frame the node the body is most in contact with.

`interaction_reference` is the DEFINITION (NumPy, float64, explicit element-wise operations in the order the kernels use,
no `np.dot` / `@`, runs found frame by frame); the kernels are csrc/interaction.hip behind include/p2r_interaction.h.  No
CPU fallback: a missing library is an error.

The rules.  W = ceil(T / 64); frame t is bit t % 64 of word t // 64 of an int64 row; the bits at T and beyond are 0.
Sample n of an N = H * B stack reads joints row n % B.  Slot s of sample n is a node iff s < count[n].
  bits       joint p (float32, widened first) is in node (c, size, R) iff, with d = p - c,
             |((0.0 + d0 R[a][0]) + d1 R[a][1]) + d2 R[a][2]| <= size[a] / 2.0 + contact_thresh for a = 0, 1, 2;
             a NaN coordinate is inside nothing.  Frame t is a contact frame iff any of its joints is in.
  intervals  (1) the raw runs [start, end) of contact frames; (2) neighbouring runs are merged while start_next -
             end_prev <= merge_gap; (3) merged runs with end - start < min_len are dropped.  `clean` holds the frames of
             the surviving runs, merged gaps included.
  labels     label[n, t] = among the nodes whose clean bit t is set the one with most joints in, ties to the lowest slot;
             -1 without one.
"""
import collections

import numpy as np
import torch

from .. import _lib
from .occupancy_device import pack_bits, unpack_bits
from .scene_device import _on_gpu, _want, _want_joints

MAX_K, MAX_T, MAX_J, MAX_M = 1024, 65535, 64, 64           # P2R_INTERACTION_MAX_K / _T / _J / _M of the header
MAX_ELEMS = 0x7fffffff

_library = _lib.extension("interaction")
HEADER_PATH, LIB_PATH = _library.header_path, _library.lib_path
lib, _launch = _library.lib, _library.launch


def words_of(T):
    return (int(T) + 63) // 64


def _want_nk(what, t, name, tail):
    if not torch.is_tensor(t) or t.dim() != 2 + len(tail) or tuple(t.shape[2:]) != tuple(tail):
        raise ValueError(f"{what}: {name} must be (N,K{''.join(',%d' % v for v in tail)})")
    N, K = t.shape[:2]
    if K > MAX_K:
        raise ValueError(f"{what}: at most {MAX_K} nodes per sample, got K={K}")
    return N, K


def _want_sizes(what, N, K, T, M=1):
    if not 1 <= T <= MAX_T:
        raise ValueError(f"{what}: 1..{MAX_T} frames, got T={T}")
    if N * K * T > MAX_ELEMS or N * K * M * 2 > MAX_ELEMS:
        raise ValueError(f"{what}: N * K * T and N * K * M * 2 must fit 2^31-1, got N={N}, K={K}, T={T}, M={M}")


# ---- the device path ---------------------------------------------------------------------------------------------------
def contact_bits(joints, node_obbs, node_rmat, count, contact_thresh, njoint=True):
    """joints (B,T,J,3|4) f32, node_obbs (N,K,7) f64, node_rmat (N,K,3,3) f64, count (N) i32 as `scene_nodes` returns them
    (or ground-truth nodes with their stored R_mat), N % B == 0, on one GPU -> (bits (N,K,W) i64, njoint (N,K,T) u8 or None,
    joint_mask (N,K) i64, n_raw (N,K) i32): the frames in which a joint lies inside the node's box enlarged by
    contact_thresh, how many joints do, which joints ever do, and the number of such frames.  One launch."""
    what = "contact_bits"
    joints = _want_joints(what, joints, MAX_T)
    N, K = _want_nk(what, node_obbs, "node_obbs", (7,))
    B, T, J, C = joints.shape
    if B < 1 or N % B != 0:
        raise ValueError(f"{what}: {N} samples over {B} joints rows: N must be a multiple of B")
    _want_sizes(what, N, K, T)
    _want(what, "node_obbs", node_obbs, torch.float64, (N, K, 7))
    _want(what, "node_rmat", node_rmat, torch.float64, (N, K, 3, 3))
    _want(what, "count", count, torch.int32, (N,))
    joints, node_obbs, node_rmat, count = _on_gpu(what, joints=joints, node_obbs=node_obbs, node_rmat=node_rmat,
                                                  count=count)
    dev = joints.device
    bits = torch.empty((N, K, words_of(T)), dtype=torch.int64, device=dev)
    nj = torch.empty((N, K, T), dtype=torch.uint8, device=dev) if njoint else None
    joint_mask = torch.empty((N, K), dtype=torch.int64, device=dev)
    n_raw = torch.empty((N, K), dtype=torch.int32, device=dev)
    _launch("p2r_contact_bits", dev, joints, B, T, J, C, N, K, node_obbs, node_rmat, count, float(contact_thresh), bits,
            nj, joint_mask, n_raw)
    return bits, nj, joint_mask, n_raw


def _want_run_args(what, T, merge_gap, min_len, max_intervals):
    merge_gap, min_len, M = int(merge_gap), int(min_len), int(max_intervals)
    if not 0 <= merge_gap <= T:
        raise ValueError(f"{what}: merge_gap must be in 0..{T}, got {merge_gap}")
    if not 1 <= min_len <= T:
        raise ValueError(f"{what}: min_len must be in 1..{T}, got {min_len}")
    if not 1 <= M <= MAX_M:
        raise ValueError(f"{what}: max_intervals must be in 1..{MAX_M}, got {M}")
    return merge_gap, min_len, M


def contact_intervals(bits, count, T, merge_gap=0, min_len=1, max_intervals=16):
    """bits (N,K,W) i64 of T frames, count (N) i32, on one GPU -> (clean (N,K,W) i64, n_intervals (N,K) i32, intervals
    (N,K,M,2) i32, n_frames (N,K) i32, first (N,K) i32, last (N,K) i32): the runs of set bits merged over gaps of at most
    merge_gap frames, then without those shorter than min_len; the first M = max_intervals of them as (start, end), -1
    beyond.  One launch."""
    what = "contact_intervals"
    T = int(T)
    if not torch.is_tensor(bits) or bits.dim() != 3:
        raise ValueError(f"{what}: bits must be (N,K,W)")
    N, K = bits.shape[:2]
    if K > MAX_K:
        raise ValueError(f"{what}: at most {MAX_K} nodes per sample, got K={K}")
    if not 1 <= T <= MAX_T:
        raise ValueError(f"{what}: 1..{MAX_T} frames, got T={T}")
    merge_gap, min_len, M = _want_run_args(what, T, merge_gap, min_len, max_intervals)
    _want_sizes(what, N, K, T, M)
    _want(what, "bits", bits, torch.int64, (N, K, words_of(T)))
    _want(what, "count", count, torch.int32, (N,))
    bits, count = _on_gpu(what, bits=bits, count=count)
    dev = bits.device
    clean = torch.empty((N, K, words_of(T)), dtype=torch.int64, device=dev)
    n_intervals, n_frames, first, last = (torch.empty((N, K), dtype=torch.int32, device=dev) for _ in range(4))
    intervals = torch.empty((N, K, M, 2), dtype=torch.int32, device=dev)
    _launch("p2r_contact_intervals", dev, bits, count, N, K, T, merge_gap, min_len, M, clean, n_intervals, intervals,
            n_frames, first, last)
    return clean, n_intervals, intervals, n_frames, first, last


def frame_labels(clean, njoint, count):
    """clean (N,K,W) i64, njoint (N,K,T) u8, count (N) i32, on one GPU -> (label (N,T) i32, n_active (N,T) u8, n_labelled
    (N) i32): per frame the node with the clean bit and most joints in contact (ties: the lowest slot; -1: none), the
    number of nodes with the bit (saturating at 255), and per sample the number of labelled frames.  One launch behind
    one clear."""
    what = "frame_labels"
    if not torch.is_tensor(njoint) or njoint.dim() != 3:
        raise ValueError(f"{what}: njoint must be (N,K,T) uint8 (contact_bits(..., njoint=True))")
    N, K, T = njoint.shape
    if K > MAX_K:
        raise ValueError(f"{what}: at most {MAX_K} nodes per sample, got K={K}")
    _want_sizes(what, N, K, T)
    _want(what, "njoint", njoint, torch.uint8, (N, K, T))
    _want(what, "clean", clean, torch.int64, (N, K, words_of(T)))
    _want(what, "count", count, torch.int32, (N,))
    clean, njoint, count = _on_gpu(what, clean=clean, njoint=njoint, count=count)
    dev = clean.device
    label = torch.empty((N, T), dtype=torch.int32, device=dev)
    n_active = torch.empty((N, T), dtype=torch.uint8, device=dev)
    n_labelled = torch.empty((N,), dtype=torch.int32, device=dev)
    _launch("p2r_frame_labels", dev, clean, njoint, count, N, K, T, label, n_active, n_labelled)
    return label, n_active, n_labelled


# ---- the definition ----------------------------------------------------------------------------------------------------
Interaction = collections.namedtuple(
    'Interaction', 'bits njoint joint_mask n_raw clean n_intervals intervals n_frames first last label n_active n_labelled')


def reference_inside(joints, count, node_obbs, node_rmat, contact_thresh, *, strict=False, thresh_on_size=False):
    """The box rule -> bool (N,K,T,J): joint j of frame t is in node s of sample n.  The keyword-only switches turn it
    into a WRONG definition, for the tests: strict=True (< for <=), thresh_on_size=True (the threshold added to the size,
    not to the half size)."""
    joints, count = np.asarray(joints), np.asarray(count)
    node_obbs, node_rmat = np.asarray(node_obbs), np.asarray(node_rmat)
    assert joints.dtype == np.float32 and joints.ndim == 4 and joints.shape[3] in (3, 4)
    assert node_obbs.dtype == np.float64 and node_rmat.dtype == np.float64
    N, K = node_obbs.shape[:2]
    B, T, J = joints.shape[:3]
    assert B >= 1 and N % B == 0
    thr = np.float64(contact_thresh)
    inside = np.zeros((N, K, T, J), dtype=bool)
    for n in range(N):
        p = joints[n % B, :, :, 0:3].astype(np.float64)
        for s in range(min(max(int(count[n]), 0), K)):
            c, size, R = node_obbs[n, s, 0:3], node_obbs[n, s, 3:6], node_rmat[n, s]
            with np.errstate(over='ignore', invalid='ignore'):
                d0, d1, d2 = p[..., 0] - c[0], p[..., 1] - c[1], p[..., 2] - c[2]
                ok = np.ones((T, J), dtype=bool)
                for a in range(3):
                    local = ((0.0 + d0 * R[a, 0]) + d1 * R[a, 1]) + d2 * R[a, 2]
                    half = (size[a] + thr) / 2.0 if thresh_on_size else size[a] / 2.0 + thr
                    ok &= (np.abs(local) < half) if strict else (np.abs(local) <= half)
            inside[n, s] = ok
    return inside


def runs_of(row):
    """bool (T,) -> the list of the runs of True as [start, end), found frame by frame"""
    runs, start = [], None
    for t, v in enumerate(row.tolist()):
        if v and start is None:
            start = t
        elif not v and start is not None:
            runs.append([start, t])
            start = None
    if start is not None:
        runs.append([start, len(row)])
    return runs


def clean_runs(runs, merge_gap, min_len, *, filter_first=False):
    """steps (2) and (3) on a list of [start, end); filter_first=True is the WRONG order"""
    def merge(rs):
        out = []
        for a, b in rs:
            if out and a - out[-1][1] <= merge_gap:
                out[-1][1] = b
            else:
                out.append([a, b])
        return out

    def keep(rs):
        return [[a, b] for a, b in rs if b - a >= min_len]

    runs = [list(r) for r in runs]
    return merge(keep(runs)) if filter_first else keep(merge(runs))


def reference_intervals(dense, count, merge_gap, min_len, M, *, filter_first=False, end_inclusive=False):
    """dense bool (N,K,T) -> (clean bool (N,K,T), n_intervals, intervals (N,K,M,2), n_frames, first, last); the switches:
    filter_first (drop short runs before merging), end_inclusive (the end of an interval is its last frame)."""
    N, K, T = dense.shape
    clean = np.zeros((N, K, T), dtype=bool)
    n_intervals, n_frames = np.zeros((N, K), np.int32), np.zeros((N, K), np.int32)
    first, last = np.full((N, K), -1, np.int32), np.full((N, K), -1, np.int32)
    intervals = np.full((N, K, M, 2), -1, np.int32)
    for n in range(N):
        for s in range(min(max(int(count[n]), 0), K)):
            if not dense[n, s].any():
                continue
            runs = clean_runs(runs_of(dense[n, s]), merge_gap, min_len, filter_first=filter_first)
            for a, b in runs:
                clean[n, s, a:b] = True
            n_intervals[n, s] = len(runs)
            for i, (a, b) in enumerate(runs[:M]):
                intervals[n, s, i] = (a, b - 1 if end_inclusive else b)
            n_frames[n, s] = sum(b - a for a, b in runs)
            if runs:
                first[n, s], last[n, s] = runs[0][0], runs[-1][1] - 1
    return clean, n_intervals, intervals, n_frames, first, last


def reference_labels(clean, njoint, count, *, tie='low'):
    """clean bool (N,K,T), njoint uint8 (N,K,T) -> (label (N,T) i32, n_active (N,T) u8, n_labelled (N) i32); tie='high' is
    the WRONG rule (equal counts: the higher slot)."""
    N, K, T = clean.shape
    label = np.full((N, T), -1, np.int32)
    n_active = np.zeros((N, T), np.uint8)
    for n in range(N):
        best = np.full(T, -1, np.int64)
        active = np.zeros(T, np.int64)
        for s in range(min(max(int(count[n]), 0), K)):
            nj = njoint[n, s].astype(np.int64)
            take = clean[n, s] & ((nj >= best) if tie == 'high' else (nj > best))
            label[n][take] = s
            best[take] = nj[take]
            active += clean[n, s]
        n_active[n] = np.minimum(active, 255).astype(np.uint8)
    return label, n_active, (label >= 0).sum(1).astype(np.int32)


def interaction_reference(joints, count, node_obbs, node_rmat, contact_thresh, merge_gap=0, min_len=1, max_intervals=16,
                          *, strict=False, thresh_on_size=False, filter_first=False, end_inclusive=False, tie='low'):
    """The definition of everything `SceneBatch.interactions` returns, on host arrays: joints (B,T,J,3|4) float32 and the
    node arrays of N = H * B samples -> Interaction of int64 / uint8 / int32 arrays in the layouts of the header.  The
    keyword-only switches are the wrong definitions of the parts."""
    inside = reference_inside(joints, count, node_obbs, node_rmat, contact_thresh, strict=strict,
                              thresh_on_size=thresh_on_size)
    N, K, T, J = inside.shape
    njoint = inside.sum(3).astype(np.uint8)                   # J <= 64
    dense = njoint > 0
    joint_mask = pack_bits(inside.any(2))[..., 0] if N * K else np.zeros((N, K), np.int64)
    clean, n_intervals, intervals, n_frames, first, last = reference_intervals(
        dense, count, int(merge_gap), int(min_len), int(max_intervals), filter_first=filter_first,
        end_inclusive=end_inclusive)
    label, n_active, n_labelled = reference_labels(clean, njoint, count, tie=tie)
    return Interaction(pack_bits(dense), njoint, joint_mask, dense.sum(2).astype(np.int32), pack_bits(clean), n_intervals,
                       intervals, n_frames, first, last, label, n_active, n_labelled)


# ---- the batch ---------------------------------------------------------------------------------------------------------
class InteractionBatch(object):
    """The interaction timelines of the N = H * B samples of a `SceneBatch` (`.scenes`) over T frames, on the device: the
    tensors of `Interaction` as attributes (njoint, label, n_active, n_labelled: None with labels=False).  Nothing is
    copied to the host before `host`, `timeline` or `labels` is called; `host` copies everything once and caches."""

    _FIELDS = Interaction._fields

    def __init__(self, scenes, T, tensors, contact_thresh, merge_gap, min_len, max_intervals):
        self.scenes, self.T = scenes, int(T)
        self.H, self.B, self.K = scenes.H, scenes.B, scenes.K
        self.contact_thresh, self.merge_gap = float(contact_thresh), int(merge_gap)
        self.min_len, self.max_intervals = int(min_len), int(max_intervals)
        for name, t in zip(self._FIELDS, tensors):
            setattr(self, name, t)
        if tuple(self.bits.shape) != (self.H * self.B, self.K, words_of(self.T)):
            raise ValueError(f"InteractionBatch: bits {(self.H * self.B, self.K, words_of(self.T))} expected, got "
                             f"{tuple(self.bits.shape)}")
        self._host_arrays = None

    def __len__(self):
        return self.H * self.B

    def tensors(self):
        """-> Interaction of the device tensors"""
        return Interaction(*[getattr(self, f) for f in self._FIELDS])

    def host(self):
        """-> {field: ndarray} of the tensors that are present (one synchronisation, cached)"""
        if self._host_arrays is None:
            from .ap_helper import _to_host
            names = [f for f in self._FIELDS if getattr(self, f) is not None]
            self._host_arrays = dict(zip(names, _to_host([getattr(self, f) for f in names])))
        return self._host_arrays

    def timeline(self, b, h=0):
        """-> per node of sample b of hypothesis h: {'inst_idx', 'class_id', 'score', 'intervals': [(start, end), ...] (at
        most max_intervals of them, end exclusive), 'n_intervals', 'n_frames', 'first', 'last', 'joints': the indices of
        the joints that touch the node in any frame}"""
        n = self.scenes.sample(b, h)
        z, sc = self.host(), self.scenes.host()
        out = []
        for s in range(min(max(int(sc['count'][n]), 0), self.K)):
            m = min(int(z['n_intervals'][n, s]), self.max_intervals)
            mask = int(z['joint_mask'][n, s]) & 0xffffffffffffffff
            out.append({'inst_idx': int(sc['inst_idx'][n, s]), 'class_id': int(sc['node_cls'][n, s]),
                        'score': float(sc['node_score'][n, s]),
                        'intervals': [(int(a), int(e)) for a, e in z['intervals'][n, s, :m]],
                        'n_intervals': int(z['n_intervals'][n, s]), 'n_frames': int(z['n_frames'][n, s]),
                        'first': int(z['first'][n, s]), 'last': int(z['last'][n, s]),
                        'joints': [j for j in range(64) if (mask >> j) & 1]})
        return out

    def labels(self, b, h=0):
        """-> int32 (T,): per frame the slot of the node the body is most in contact with, -1 for none"""
        z = self.host()
        if 'label' not in z:
            raise RuntimeError("InteractionBatch: the frame labels were not computed (labels=False)")
        return z['label'][self.scenes.sample(b, h)].copy()

    def dense(self, n, clean=True):
        """-> bool (K,T): the contact frames of every slot of sample n of the stack (clean: after merging and filtering)"""
        z = self.host()
        if not 0 <= n < len(self):
            raise IndexError(f"InteractionBatch: sample {n} outside {len(self)}")
        return unpack_bits(z['clean' if clean else 'bits'][n], self.T)


def interactions_of(scenes, joints, contact_thresh=None, merge_gap=0, min_len=1, max_intervals=16, labels=True):
    """SceneBatch and the batch's joints (B,T,J,3|4) f32 -> InteractionBatch (what `SceneBatch.interactions` calls).
    contact_thresh=None is `vote_labels.default_contact_dist()`, the distance the training labels are made with (it is
    not `SceneBatch.contact_dist`, the distance at the contact frame).  Three launches -- bits, intervals, labels -- or
    two with labels=False, when njoint is not allocated either; nothing is copied to the host."""
    from . import scene_device
    what = "SceneBatch.interactions"
    if not isinstance(scenes, scene_device.SceneBatch):
        raise TypeError(f"{what}: a SceneBatch expected, got {type(scenes).__name__}")
    if not torch.is_tensor(joints) or joints.dim() != 4 or joints.shape[0] != scenes.B:
        raise ValueError(f"{what}: joints must be ({scenes.B},T,J,3|4), one row per sample of the batch")
    if contact_thresh is None:
        from .vote_labels import default_contact_dist
        contact_thresh = default_contact_dist()
    T = joints.shape[1]
    _want_joints(what, joints, MAX_T)
    _want_run_args(what, T, merge_gap, min_len, max_intervals)
    bits, njoint, joint_mask, n_raw = contact_bits(joints, scenes.node_obbs, scenes.node_rmat, scenes.count,
                                                   contact_thresh, njoint=labels)
    runs = contact_intervals(bits, scenes.count, T, merge_gap, min_len, max_intervals)
    lab = frame_labels(runs[0], njoint, scenes.count) if labels else (None, None, None)
    return InteractionBatch(scenes, T, Interaction(bits, njoint, joint_mask, n_raw, *runs, *lab), contact_thresh,
                            merge_gap, min_len, max_intervals)
