"""Vote labels of a pose sequence, derived on the device (csrc/vote_labels.hip, include/p2r_vote_labels.h).

The reference makes `skeleton_joint_votes (T0, J, 10)` when it writes its sample files
(utils/virtualhome/3_generate_samples.py:56-79,176-187, `get_votes`): column 0 is the vote mask, columns 1..9 three
offsets to object centres.  A joint votes for the boxes whose contact space -- the box enlarged by
`contact_dist_thresh` on every side -- contains it, in list order: the first hit fills all three slots, the second
slot 1, every later one slot 2.  The reference tests containment with a Delaunay hull; for a box with orthonormal axes
that is `|R (p - c)| <= size / 2 + contact_dist` per axis, which is what the kernel and its NumPy mirror compute.

  * `vote_labels_reference`  the NumPy mirror of the kernel's arithmetic, one sample
  * `contact_tables`         the f64 table rows of one sample (p2r_contact_boxes) and the checks on its boxes
  * `ContactBoxes`           the tables of N samples on the device
  * `vote_labels`            p2r_vote_labels: the votes of a whole packed store in one launch
  * `generate_votes`         one sample through the device op

No CPU fallback: the mirror is what the tests compare against, not a second implementation behind the op.
"""
import ctypes

import numpy as np
import torch

from .. import _lib

MAX_K = 256                     # box slots per sample (include/p2r_vote_labels.h)
ORTHONORMAL_TOL = 1e-6          # |R R^T - I| above this: the hull test and the closed form need not agree

# The kernels are a fourth library next to libp2r_hip.so (csrc/Makefile), with a header of their own; the binding is
# derived from that header as that of libp2r_hip.so is (_lib.Library).
_library = _lib.extension("vote_labels")
HEADER_PATH, LIB_PATH = _library.header_path, _library.lib_path
lib, _launch = _library.lib, _library.launch
_Boxes = _library.struct('p2r_contact_boxes')


def default_contact_dist():
    """`dataset_config.contact_dist_thresh` of P2RConfig (configs/dataset_config.py:56)."""
    from ..p2rnet.config import DatasetConfig
    return float(DatasetConfig.contact_dist_thresh)


# ---- the contract in NumPy ------------------------------------------------------------------------------------------
def vote_labels_reference(joints, instances, contact_dist):
    """joints (T0, J, 3) f32, instances: list of dicts with centroid, R_mat, size -> votes (T0, J, 10) f32 by the
    kernel's arithmetic (header comment of csrc/vote_labels.hip), f64 in the kernel's operation order."""
    joints = np.asarray(joints)
    if joints.dtype != np.float32:
        raise ValueError(f"vote_labels_reference: float32 joints expected, got {joints.dtype}")
    p = joints.astype(np.float64)
    out = np.zeros(p.shape[:-1] + (10,), np.float32)
    hits = np.zeros(p.shape[:-1], np.int64)
    for node in instances:
        c = np.asarray(node['centroid'], np.float64)
        R = np.asarray(node['R_mat'], np.float64)
        h = np.array(node['size']) / 2. + contact_dist
        d = p - c
        local = np.stack([((0.0 + d[..., 0] * R[a, 0]) + d[..., 1] * R[a, 1]) + d[..., 2] * R[a, 2] for a in range(3)],
                         -1)
        inside = (np.abs(local) <= h).all(-1)
        vote = (c - p).astype(np.float32)
        slot = np.minimum(hits, 2)
        for s in range(3):
            m = inside & ((slot == s) | (hits == 0))
            out[..., 1 + 3 * s:4 + 3 * s][m] = vote[m]
        out[..., 0][inside] = 1
        hits += inside
    return out


def contact_tables(instances, max_num_obj, contact_dist, name=None):
    """The rows of p2r_contact_boxes for one sample -> (centroid (K, 3), R_mat (K, 9), half (K, 3)) f64 with K =
    max_num_obj, and the number of boxes.  half = size / 2 + contact_dist exactly as the reference computes it.
    Raises ValueError, naming the sample (`name`) and the box, for more than max_num_obj boxes, a non-finite size,
    centroid or contact_dist, and an R_mat whose rows are not orthonormal (|R R^T - I| > 1e-6)."""
    who = "a sample" if name is None else f"sample {name}"
    n, K = len(instances), int(max_num_obj)
    if not 0 <= K <= MAX_K:
        raise ValueError(f"contact_tables: max_num_obj = {K}, outside 0..{MAX_K}")
    if n > K:
        raise ValueError(f"{who} has {n} boxes, more than max_num_obj = {K}")
    if not np.isfinite(contact_dist):
        raise ValueError(f"contact_tables: contact_dist = {contact_dist} is not finite")
    centroid, R_mat, half = np.zeros((K, 3)), np.zeros((K, 9)), np.zeros((K, 3))
    for i, node in enumerate(instances):
        c = np.asarray(node['centroid'], np.float64)
        R = np.asarray(node['R_mat'], np.float64)
        h = np.array(node['size']) / 2. + contact_dist
        if c.shape != (3,) or R.shape != (3, 3) or h.shape != (3,):
            raise ValueError(f"{who}, box {i}: centroid (3,), R_mat (3, 3) and size (3,) expected, got {c.shape}, "
                             f"{R.shape}, {h.shape}")
        if not (np.isfinite(c).all() and np.isfinite(h).all()):
            raise ValueError(f"{who}, box {i}: centroid {c.tolist()} / size {np.asarray(node['size']).tolist()} is "
                             "not finite")
        err = np.abs(R.dot(R.T) - np.eye(3)).max()
        if not err <= ORTHONORMAL_TOL:
            raise ValueError(f"{who}, box {i}: the rows of R_mat are not orthonormal (|R R^T - I| = {err:.3g} > "
                             f"{ORTHONORMAL_TOL}); the contact test holds for boxes with orthonormal axes only")
        centroid[i], R_mat[i], half[i] = c, R.reshape(9), h
    return (centroid, R_mat, half), n


class ContactBoxes(object):
    """The contact tables of N samples on the device (p2r_contact_boxes): centroid (N, K, 3), R_mat (N, K, 9), half
    (N, K, 3) f64 and n_boxes (N,) i32.  `c` is the struct the entry points take."""

    def __init__(self, tables, device):
        """tables: one `contact_tables` result per sample"""
        tables = list(tables)
        if not tables:
            raise ValueError("ContactBoxes: no samples")
        put = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)       # noqa: E731
        self.centroid, self.R_mat, self.half = [put(np.stack([t[0][k] for t in tables])) for k in range(3)]
        self.n_boxes = put(np.asarray([t[1] for t in tables], np.int32))
        self.N, self.K = self.centroid.shape[0], self.centroid.shape[1]
        self.device = self.n_boxes.device
        self.c = _Boxes(centroid=self.centroid.data_ptr(), R_mat=self.R_mat.data_ptr(), half=self.half.data_ptr(),
                        n_boxes=self.n_boxes.data_ptr(), K=self.K)

    @staticmethod
    def nbytes(N, K):
        return N * (K * (3 + 9 + 3) * 8 + 4)


# ---- the device op --------------------------------------------------------------------------------------------------
def vote_labels(joints, frame_offset, n_frames, tables):
    """joints (F, J, 3) f32, frame_offset (N,) i64 ascending, n_frames (N,) i32 -- the packed layout of
    DeviceSampleStore -- and `tables` the ContactBoxes of the N samples, all on one GPU -> votes (F, J, 10) f32, every
    element written, in one launch."""
    for name, t in (('joints', joints), ('frame_offset', frame_offset), ('n_frames', n_frames)):
        if not (torch.is_tensor(t) and t.is_cuda):
            raise RuntimeError(f"vote_labels: {name} must be a GPU tensor (no CPU fallback)")
    if not isinstance(tables, ContactBoxes):
        raise TypeError("vote_labels: tables must be a ContactBoxes")
    if joints.dtype != torch.float32 or frame_offset.dtype != torch.int64 or n_frames.dtype != torch.int32:
        raise RuntimeError("vote_labels: joints float32, frame_offset int64 and n_frames int32 expected, got "
                           f"{joints.dtype}, {frame_offset.dtype}, {n_frames.dtype}")
    N = tables.N
    if joints.dim() != 3 or joints.shape[2] != 3 or joints.shape[0] < 1 or joints.shape[1] < 1 or \
            frame_offset.shape != (N,) or n_frames.shape != (N,):
        raise ValueError(f"vote_labels: joints (F, J, 3) and frame_offset, n_frames ({N},) expected, got "
                         f"{tuple(joints.shape)}, {tuple(frame_offset.shape)}, {tuple(n_frames.shape)}")
    dev = joints.device
    if frame_offset.device != dev or n_frames.device != dev or tables.device != dev:
        raise RuntimeError(f"vote_labels: every tensor must be on {dev}")
    F, J = joints.shape[:2]
    votes = torch.empty((F, J, 10), dtype=torch.float32, device=dev)
    _launch("p2r_vote_labels", dev, joints.contiguous(), frame_offset.contiguous(), n_frames.contiguous(), N, J, F,
            ctypes.byref(tables.c), votes)
    return votes


def assemble_batch_lean(device, store, boxes, B, sel, aug, augment, use_height, num_frames, out):
    """Thin binding of p2r_assemble_batch_lean for p2rnet/device_loader.py: `store` and `out` are byref(struct) of
    p2r_sample_store (votes = NULL) and p2r_batch_out, `boxes` the ContactBoxes of the store's samples, sel and aug
    device tensors (aug may be None without augmentation)."""
    _launch("p2r_assemble_batch_lean", device, store, ctypes.byref(boxes.c), B, sel, aug, augment, use_height,
            num_frames, out)


def generate_votes(joints, instances, contact_dist=None, device=None):
    """The vote labels of one sample, the stage the reference runs when it writes a sample file: joints (T0, J, 3) f32
    (array or tensor) and its room's object boxes -> (T0, J, 10) f32 tensor on `device` (default: the current GPU).
    contact_dist defaults to the config's `dataset_config.contact_dist_thresh`."""
    contact_dist = default_contact_dist() if contact_dist is None else contact_dist
    device = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
    if device.type != 'cuda':
        raise RuntimeError("generate_votes: the votes are derived on a GPU (no CPU fallback)")
    j = joints if torch.is_tensor(joints) else torch.from_numpy(np.ascontiguousarray(joints))
    if j.dtype != torch.float32 or j.dim() != 3 or j.shape[2] != 3 or j.shape[0] < 1:
        raise ValueError(f"generate_votes: float32 joints (T0, J, 3) expected, got {j.dtype} {tuple(j.shape)}")
    tables = ContactBoxes([contact_tables(instances, len(instances), contact_dist)], device)
    return vote_labels(j.to(device), torch.zeros(1, dtype=torch.int64, device=device),
                       torch.full((1,), j.shape[0], dtype=torch.int32, device=device), tables)
