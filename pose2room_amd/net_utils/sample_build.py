"""Trainable samples made of raw recordings on the device (csrc/sample_build.hip, include/p2r_sample_build.h).

Stage 3 of the reference's data preparation (utils/virtualhome/3_generate_samples.py, `run()`, lines 96-187) turns a raw
recording into eight trainable samples.  A recording here is a dict

    joints        (F, J, 3) float64, world coordinates, 1 <= F <= 65535 (a NumPy array or a tensor, on any device)
    room_bbox     {centroid, size, R_mat}
    object_nodes  list of {class_id, centroid, R_mat, size}, float64, class ids already mapped
    name          the reference's `base_name`

and the stage: drop the frames before the first one whose origin joint is in the room (`check_in_box`), reject the
recording when there is none ("never in the room") or when no remaining frame has its origin joint inside an object box
enlarged by the contact distance on every side ("near no object"), move the origin to the room's floor centre, and
write the variants a = 0..7 -- a > 3: swap x and z; then a % 4 quarter turns (x, y, z) <- (z, y, -x) -- each with the
float32 joints, the votes derived from the FLOAT64 joints (the rule of include/p2r_vote_labels.h) and the nodes turned
the same way, under the name `name + '_%d' % a`.

  * `build_reference`   the NumPy mirror of that contract, one recording
  * `floor_reference`   the two `np.percentile(y, 0.99)` mirrors the floor kernel computes
  * `recording_scan`, `floor_percentile`   the entry points on tensors
  * `build_samples`     recordings -> packed device tensors (joints, votes, frame_offset, n_frames, floors); with
                        `repair=` the recordings' missing joints are filled on the device first (recording_repair.py)

The host computes the per-box rows, O(boxes), with the reference's own expressions; every per-frame pass is a kernel.
Between the scan and the build the host reads back `first` and `status`, 8 bytes per recording, to size the output.
No CPU fallback: the mirror is what the tests compare against, not a second implementation behind the op.
"""
import collections
import ctypes

import numpy as np
import torch

from .. import _lib
from . import vote_labels as vl

MAX_FRAMES, MAX_J = 65535, 256          # P2R_SB_MAX_FRAMES / P2R_SB_MAX_J of include/p2r_sample_build.h
NEVER_IN_ROOM, NEAR_NO_OBJECT = "never in the room", "near no object"
UNREPAIRABLE = "not finite after the repair"        # only with build_samples(repair=..., on_unrepairable='skip')
STATUS_NO_ROOM, STATUS_NO_OBJECT, STATUS_NON_FINITE = 1, 2, 4

FLIP = np.array([[0, 0, 1], [0, 1, 0], [1, 0, 0]])           # swaps x and z
ROT90 = np.array([[0, 0, -1], [0, 1, 0], [1, 0, 0]])         # (x, y, z) -> (z, y, -x) as a row vector times it

_library = _lib.extension("sample_build")
HEADER_PATH, LIB_PATH = _library.header_path, _library.lib_path
lib, _launch = _library.lib, _library.launch
_Recordings = _library.struct('p2r_recordings')
_Plan = _library.struct('p2r_sample_plan')


def _config():
    from ..p2rnet.config import DatasetConfig
    return DatasetConfig


# ---- the contract in NumPy ------------------------------------------------------------------------------------------
def _inside(p, c, R, half):
    """(..., 3) f64 positions inside the box: |((0 + d0 R[a,0]) + d1 R[a,1]) + d2 R[a,2]| <= half_a for every a"""
    d = p - c
    local = np.stack([((0.0 + d[..., 0] * R[a, 0]) + d[..., 1] * R[a, 1]) + d[..., 2] * R[a, 2] for a in range(3)], -1)
    return (np.abs(local) <= half).all(-1)


def room_row(room_bbox):
    """-> the 15 doubles of a room: centroid, R_mat row-major, half = size / 2 (check_in_box's `size/2.`)"""
    c = np.array(room_bbox['centroid'], np.float64)
    R = np.array(room_bbox['R_mat'], np.float64)
    size = np.array(room_bbox['size'], np.float64)
    if c.shape != (3,) or R.shape != (3, 3) or size.shape != (3,):
        raise ValueError(f"room_bbox: centroid (3,), R_mat (3, 3) and size (3,) expected, got {c.shape}, {R.shape}, "
                         f"{size.shape}")
    return np.concatenate([c, R.reshape(9), size / 2.])


def enlarged_nodes(object_nodes, contact_dist):
    """The dummy nodes of 3_generate_samples.py:112-115: size + 2 * contact.  contact_tables adds 0 to size / 2."""
    return [dict(node, size=np.array(node['size']) + 2 * contact_dist) for node in object_nodes]


def floor_shift(room_bbox):
    """3_generate_samples.py:127-128: the room's floor centre"""
    shift = np.array(room_bbox['centroid'], np.float64)
    shift[1] = shift[1] - room_bbox['size'][1] / 2
    return shift


def variant_nodes(object_nodes, shift, aug_idx):
    """augment_sample's node math on the recentred nodes: centroid and R_mat times flip, R[2] = cross(R[0], R[1]), then
    times rot90^k."""
    rot = np.linalg.matrix_power(ROT90, aug_idx % 4)
    nodes = []
    for node in object_nodes:
        c = np.array(node['centroid'], np.float64) - shift
        R = np.array(node['R_mat'], np.float64)
        if aug_idx > 3:
            c = np.matmul(c, FLIP)
            R = R.dot(FLIP)
            R[2] = np.cross(R[0], R[1])
        nodes.append(dict(class_id=node['class_id'], centroid=np.matmul(c, rot), R_mat=R.dot(rot),
                          size=np.array(node['size'], np.float64)))
    return nodes


def variant_joints(q, aug_idx):
    """(..., 3) f64 -> the signed permutation of variant aug_idx"""
    x, y, z = q[..., 0], q[..., 1], q[..., 2]
    if aug_idx > 3:
        x, z = z, x
    for _ in range(aug_idx % 4):
        x, z = z, -x
    return np.stack([x, y, z], -1)


def votes_reference(q, nodes, contact_dist):
    """The vote rows of f64 positions q (..., 3) by the rule of include/p2r_vote_labels.h with p = q -> (..., 10) f32."""
    out = np.zeros(q.shape[:-1] + (10,), np.float32)
    hits = np.zeros(q.shape[:-1], np.int64)
    for node in nodes:
        c = np.asarray(node['centroid'], np.float64)
        inside = _inside(q, c, np.asarray(node['R_mat'], np.float64), np.array(node['size']) / 2. + contact_dist)
        vote = (c - q).astype(np.float32)
        slot = np.minimum(hits, 2)
        for s in range(3):
            m = inside & ((slot == s) | (hits == 0))
            out[..., 1 + 3 * s:4 + 3 * s][m] = vote[m]
        out[..., 0][inside] = 1
        hits += inside
    return out


def scan_reference(joints, room_bbox, object_nodes, contact_dist, origin_joint):
    """-> (first, status) as p2r_recording_scan defines them"""
    joints = np.asarray(joints, np.float64)
    hip = joints[:, origin_joint]
    room = room_row(room_bbox)
    in_room = _inside(hip, room[0:3], room[3:12].reshape(3, 3), room[12:15])
    status = 0 if np.isfinite(joints).all() else STATUS_NON_FINITE
    if not in_room.any():
        return -1, status | STATUS_NO_ROOM | STATUS_NO_OBJECT
    first = int(np.argmax(in_room))
    near = np.zeros(len(hip) - first, bool)
    for node in enlarged_nodes(object_nodes, contact_dist):
        near |= _inside(hip[first:], np.asarray(node['centroid'], np.float64), np.asarray(node['R_mat'], np.float64),
                        np.array(node['size']) / 2.)
    return first, status | (0 if near.any() else STATUS_NO_OBJECT)


Built = collections.namedtuple("Built", "samples first reason")
Built.__doc__ = """build_reference's result: samples = [(joints f32, votes f32, nodes, name)] or None when the recording
is rejected; first = the first frame in the room (-1: none); reason = None or the rejection reason."""


def build_reference(recording, aug_indices=range(8), contact_dist=None, origin_joint=None):
    """The NumPy mirror of the stage (module docstring) for one recording -> Built."""
    cfg = _config()
    contact_dist = float(cfg.contact_dist_thresh) if contact_dist is None else contact_dist
    origin_joint = cfg.origin_joint_id if origin_joint is None else origin_joint
    joints = np.asarray(recording['joints'].cpu() if torch.is_tensor(recording['joints']) else recording['joints'])
    if joints.dtype != np.float64 or joints.ndim != 3 or joints.shape[2] != 3:
        raise ValueError(f"recording {recording['name']}: float64 joints (F, J, 3) expected, got {joints.dtype} "
                         f"{joints.shape}")
    first, status = scan_reference(joints, recording['room_bbox'], recording['object_nodes'], contact_dist, origin_joint)
    if status & STATUS_NON_FINITE:
        raise ValueError(f"recording {recording['name']} has a coordinate that is not finite")
    if status & STATUS_NO_ROOM:
        return Built(None, first, NEVER_IN_ROOM)
    if status & STATUS_NO_OBJECT:
        return Built(None, first, NEAR_NO_OBJECT)
    shift = floor_shift(recording['room_bbox'])
    q = joints[first:] - shift
    samples = []
    for a in aug_indices:
        nodes = variant_nodes(recording['object_nodes'], shift, a)
        qa = variant_joints(q, a)
        samples.append((qa.astype(np.float32), votes_reference(qa, nodes, contact_dist), nodes,
                        recording['name'] + '_%d' % a))
    return Built(samples, first, None)


def percentile_reference(y):
    """The two mirrors of np.percentile(y, 0.99) of include/p2r_sample_build.h for a float32 array y -> (f64 form,
    f32 form) as Python floats."""
    y = np.sort(np.asarray(y, np.float32).ravel())
    n = y.size
    v = (n - 1) * (0.99 / 100.0)
    k = int(np.floor(v))
    g = v - k
    a, b = np.float64(y[k]), np.float64(y[min(k + 1, n - 1)])
    d = b - a
    r64 = a + d * g
    if g >= 0.5:
        r64 = b - d * (1 - g)
    f = np.float32
    v = f(n - 1) * (f(0.99) / f(100))
    k = int(np.floor(v))
    g = v - f(k)
    a, b = y[k], y[min(k + 1, n - 1)]
    d = b - a
    r32 = a + d * g
    if g >= f(0.5):
        r32 = b - d * (f(1) - g)
    assert r32.dtype == np.float32
    return float(r64), float(r32)


def floor_reference(joints):
    """`device_loader.floor_heights` by the mirrors: joints (T0, J, 3) f32 -> (f64 floor, f32 floor)"""
    return percentile_reference(np.asarray(joints, np.float32)[..., 1])


# ---- the device ops -------------------------------------------------------------------------------------------------
class Recordings(object):
    """R recordings packed on the device (p2r_recordings): joints (F_total, J, 3) f64, frame_offset (R,) i64, n_frames
    (R,) i32.  `c` is the struct the entry points take."""

    def __init__(self, joints, device):
        """joints: one (F, J, 3) float64 array or tensor per recording"""
        joints = list(joints)
        if not joints:
            raise ValueError("Recordings: no recordings")
        J = joints[0].shape[1] if joints[0].ndim == 3 else 0
        frames = []
        for i, j in enumerate(joints):
            dtype = j.dtype if torch.is_tensor(j) else torch.from_numpy(np.empty(0, j.dtype)).dtype
            if dtype != torch.float64 or j.ndim != 3 or tuple(j.shape[1:]) != (J, 3) or not 1 <= J <= MAX_J:
                raise ValueError(f"recording {i}: float64 joints (F, J, 3) with one J in 1..{MAX_J} expected, got "
                                 f"{j.dtype} {tuple(j.shape)}")
            if not 1 <= j.shape[0] <= MAX_FRAMES:
                raise ValueError(f"recording {i}: {j.shape[0]} frames, outside 1..{MAX_FRAMES}")
            frames.append(int(j.shape[0]))
        put = lambda j: (j if torch.is_tensor(j) else torch.from_numpy(np.ascontiguousarray(j))).to(device)  # noqa: E731
        self.joints = torch.cat([put(j) for j in joints]).contiguous()
        self.frames = np.asarray(frames, np.int32)
        off = np.zeros(len(frames), np.int64)
        off[1:] = np.cumsum(self.frames)[:-1]
        self.frame_offset = torch.from_numpy(off).to(device)
        self.n_frames = torch.from_numpy(self.frames).to(device)
        self.R, self.J, self.device = len(frames), int(J), self.joints.device
        self.c = _Recordings(joints=self.joints.data_ptr(), frame_offset=self.frame_offset.data_ptr(),
                             n_frames=self.n_frames.data_ptr(), n_frames_total=int(self.joints.shape[0]), R=self.R,
                             J=self.J, max_frames=int(self.frames.max()))

    @classmethod
    def from_packed(cls, joints, frame_offset, n_frames, frames):
        """The Recordings of tensors that are packed on one GPU already: joints (F_total, J, 3) f64, frame_offset (R,)
        i64 ascending, n_frames (R,) i32, and `frames`, the HOST's copy of the frame counts (R,) -- nothing is read
        back.  The tensors are kept, not copied."""
        frames = np.asarray(frames, np.int32)
        R = int(frames.shape[0]) if frames.ndim == 1 else 0
        for name, t, dtype, shape in (('joints', joints, torch.float64, None), ('frame_offset', frame_offset, torch.int64, (R,)),
                                      ('n_frames', n_frames, torch.int32, (R,))):
            if not (torch.is_tensor(t) and t.is_cuda and t.dtype == dtype and t.is_contiguous()
                    and t.device == joints.device and (shape is None or tuple(t.shape) == shape)):
                raise RuntimeError(f"Recordings.from_packed: {name} must be a contiguous {dtype} GPU tensor"
                                   + (f" of shape {shape}" if shape else "") + " (no CPU fallback)")
        if joints.dim() != 3 or joints.shape[2] != 3 or not 1 <= joints.shape[1] <= MAX_J or joints.shape[0] < 1:
            raise ValueError(f"Recordings.from_packed: joints (F_total, J, 3) with J in 1..{MAX_J} expected, got "
                             f"{tuple(joints.shape)}")
        if R < 1 or frames.min() < 1 or frames.max() > MAX_FRAMES or int(frames.sum(dtype=np.int64)) > joints.shape[0]:
            raise ValueError(f"Recordings.from_packed: frames must hold R >= 1 counts in 1..{MAX_FRAMES} that sum to at "
                             f"most the {joints.shape[0]} packed frames, got {frames.tolist()}")
        self = cls.__new__(cls)
        self.joints, self.frames, self.frame_offset, self.n_frames = joints, frames, frame_offset, n_frames
        self.R, self.J, self.device = R, int(joints.shape[1]), joints.device
        self.c = _Recordings(joints=joints.data_ptr(), frame_offset=frame_offset.data_ptr(),
                             n_frames=n_frames.data_ptr(), n_frames_total=int(joints.shape[0]), R=R, J=self.J,
                             max_frames=int(frames.max()))
        return self


def recording_scan(rec, room, objects, origin_joint):
    """p2r_recording_scan: rec a Recordings, room (R, 15) f64 tensor (`room_row` per recording), objects the
    ContactBoxes of the enlarged object boxes -> (first (R,) i32, status (R,) i32) on the device."""
    if not isinstance(rec, Recordings) or not isinstance(objects, vl.ContactBoxes):
        raise TypeError("recording_scan: a Recordings and a ContactBoxes expected")
    if not (torch.is_tensor(room) and room.is_cuda and room.dtype == torch.float64 and room.shape == (rec.R, 15)
            and room.is_contiguous() and room.device == rec.device == objects.device and objects.N == rec.R):
        raise RuntimeError(f"recording_scan: room must be a contiguous float64 ({rec.R}, 15) tensor on {rec.device}, "
                           "the device of the object boxes, which have one row per recording (no CPU fallback)")
    first = torch.empty(rec.R, dtype=torch.int32, device=rec.device)
    status = torch.empty(rec.R, dtype=torch.int32, device=rec.device)
    _launch("p2r_recording_scan", rec.device, ctypes.byref(rec.c), int(origin_joint), room, ctypes.byref(objects.c),
            first, status)
    return first, status


def build_packed(rec, recording, first, variant, out_offset, shift, n_frames_out, boxes, votes=True):
    """p2r_build_samples: rec a Recordings; recording, first, variant (S,) i32, out_offset (S,) i64, shift (S, 3) f64
    device tensors (p2r_sample_plan); boxes the ContactBoxes of the S samples (None without votes) -> (joints
    (n_frames_out, J, 3) f32, votes (n_frames_out, J, 10) f32 or None)."""
    S = recording.shape[0]
    want = ((recording, torch.int32, (S,)), (first, torch.int32, (S,)), (variant, torch.int32, (S,)),
            (out_offset, torch.int64, (S,)), (shift, torch.float64, (S, 3)))
    for t, dtype, shape in want:
        if not (torch.is_tensor(t) and t.device == rec.device and t.dtype == dtype and tuple(t.shape) == shape
                and t.is_contiguous()):
            raise RuntimeError(f"build_packed: a contiguous {dtype} {shape} tensor on {rec.device} expected")
    if votes and not (isinstance(boxes, vl.ContactBoxes) and boxes.N == S and boxes.device == rec.device):
        raise RuntimeError(f"build_packed: votes need the ContactBoxes of the {S} samples on {rec.device}")
    plan = _Plan(recording=recording.data_ptr(), first=first.data_ptr(), variant=variant.data_ptr(),
                 out_offset=out_offset.data_ptr(), shift=shift.data_ptr(), n_frames_out=int(n_frames_out), S=int(S))
    joints = torch.empty((int(n_frames_out), rec.J, 3), dtype=torch.float32, device=rec.device)
    out_votes = torch.empty((int(n_frames_out), rec.J, 10), dtype=torch.float32, device=rec.device) if votes else None
    _launch("p2r_build_samples", rec.device, ctypes.byref(rec.c), ctypes.byref(plan),
            ctypes.byref(boxes.c) if votes else None, joints, out_votes)
    return joints, out_votes


def floor_percentile(joints, frame_offset, n_frames, max_frames=MAX_FRAMES):
    """p2r_floor_percentile of a packed store: joints (F, J, 3) f32, frame_offset (N,) i64, n_frames (N,) i32 on one
    GPU -> floors (N, 2) f64: `device_loader.floor_heights` of every sample."""
    for name, t, dtype in (('joints', joints, torch.float32), ('frame_offset', frame_offset, torch.int64),
                           ('n_frames', n_frames, torch.int32)):
        if not (torch.is_tensor(t) and t.is_cuda and t.dtype == dtype and t.is_contiguous()
                and t.device == joints.device):
            raise RuntimeError(f"floor_percentile: {name} must be a contiguous {dtype} GPU tensor (no CPU fallback)")
    N = frame_offset.shape[0]
    if joints.dim() != 3 or joints.shape[2] != 3 or joints.shape[0] < 1 or n_frames.shape != (N,) or N < 1:
        raise ValueError(f"floor_percentile: joints (F, J, 3) and frame_offset, n_frames (N,) expected, got "
                         f"{tuple(joints.shape)}, {tuple(frame_offset.shape)}, {tuple(n_frames.shape)}")
    floors = torch.empty((N, 2), dtype=torch.float64, device=joints.device)
    _launch("p2r_floor_percentile", joints.device, joints, frame_offset, n_frames, N, int(joints.shape[1]),
            int(max_frames), int(joints.shape[0]), floors)
    return floors


BuiltSamples = collections.namedtuple(
    "BuiltSamples", "joints votes frame_offset n_frames floors names instances kept rejected first contact")
BuiltSamples.__doc__ = """build_samples' result.  Device tensors: joints (F, J, 3) f32, votes (F, J, 10) f32 or None,
frame_offset (N,) i64, n_frames (N,) i32, floors (N, 2) f64.  Host: names and instances (the augmented nodes) per sample,
kept = the indices of the recordings that gave samples, rejected = (name, reason) pairs, first = the first frame in the
room of every kept recording, contact = the ContactBoxes of the samples (K = max_num_obj slots)."""


def build_samples(recordings, aug_indices=range(8), contact_dist=None, device=None, votes=True, max_num_obj=None,
                  origin_joint=None, repair=None, on_unrepairable='raise'):
    """Recordings (module docstring) -> BuiltSamples: the samples of every kept recording, variant by variant in the
    order of aug_indices, packed on `device` (default: the current GPU).  contact_dist and origin_joint default to the
    config's; max_num_obj = the box slots of `contact` (default: the largest object count).  Raises ValueError, naming
    the recording, for a coordinate that is not finite.  Three launches and one read-back of 8 bytes per recording.

    repair: a `recording_repair.RepairSpec` conditions the recordings in front of the scan (missing joints filled over
    short gaps, optionally low-passed: net_utils/recording_repair.py); its statistics ride in the same read-back, 24
    bytes per recording then.  What is still not finite afterwards raises the same ValueError (on_unrepairable='raise')
    or rejects the recording with the reason UNREPAIRABLE ('skip').  The result is then a `RepairedSamples`: the same
    tuple with the attribute `repair`, the statistics (R, 4) of every recording given."""
    if on_unrepairable not in ('raise', 'skip'):
        raise ValueError(f"build_samples: on_unrepairable must be 'raise' or 'skip', got {on_unrepairable!r}")
    if repair is not None:
        from . import recording_repair as rr
        if not isinstance(repair, rr.RepairSpec):
            raise TypeError(f"build_samples: repair must be a RepairSpec or None, got {type(repair).__name__}")
    cfg = _config()
    contact_dist = float(cfg.contact_dist_thresh) if contact_dist is None else float(contact_dist)
    origin_joint = int(cfg.origin_joint_id if origin_joint is None else origin_joint)
    device = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
    if device.type != 'cuda':
        raise RuntimeError("build_samples: the samples are built on a GPU (no CPU fallback)")
    recordings, aug_indices = list(recordings), [int(a) for a in aug_indices]
    if any(a < 0 or a > 7 for a in aug_indices):
        raise ValueError(f"build_samples: aug_indices must lie in 0..7, got {aug_indices}")
    rec = Recordings([r['joints'] for r in recordings], device)
    if not 0 <= origin_joint < rec.J:
        raise ValueError(f"build_samples: origin joint {origin_joint} outside 0..{rec.J - 1}")
    K = max([len(r['object_nodes']) for r in recordings] + [0]) if max_num_obj is None else int(max_num_obj)
    objects = vl.ContactBoxes([vl.contact_tables(enlarged_nodes(r['object_nodes'], contact_dist), K, 0.0,
                                                 name=r['name']) for r in recordings], device)
    room = torch.from_numpy(np.stack([room_row(r['room_bbox']) for r in recordings])).to(device)
    repair_stats = None
    if repair is not None:
        rec, _, stats_d = rr.repair_packed(rec, repair)
        first_d, status_d = recording_scan(rec, room, objects, origin_joint)
        # still the one crossing: first, status and the four statistics of every recording
        back = torch.cat([torch.stack([first_d, status_d], 1), stats_d], 1).cpu().numpy()
        first, status, repair_stats = back[:, 0], back[:, 1], np.ascontiguousarray(back[:, 2:])
    else:
        first_d, status_d = recording_scan(rec, room, objects, origin_joint)
        first, status = torch.stack([first_d, status_d]).cpu().numpy()      # the one crossing: 8 bytes per recording
    bad = [r['name'] for r, s in zip(recordings, status) if s & STATUS_NON_FINITE]
    if bad and (repair is None or on_unrepairable == 'raise'):
        raise ValueError(f"build_samples: recording {bad[0]} has a coordinate that is not finite"
                         + (f" (and {len(bad) - 1} more: {bad[1:]})" if len(bad) > 1 else ""))
    drop = STATUS_NO_ROOM | STATUS_NO_OBJECT | STATUS_NON_FINITE           # the last only with on_unrepairable='skip'
    kept = [i for i, s in enumerate(status) if not s & drop]
    rejected = [(r['name'], UNREPAIRABLE if s & STATUS_NON_FINITE else NEVER_IN_ROOM if s & STATUS_NO_ROOM
                 else NEAR_NO_OBJECT) for r, s in zip(recordings, status) if s & drop]
    done = (lambda built: built) if repair is None else (lambda built: rr.RepairedSamples(built, repair_stats))  # noqa: E731
    names, instances, tables, plan, shifts = [], [], [], [], []
    for i in kept:
        r, shift = recordings[i], floor_shift(recordings[i]['room_bbox'])
        for a in aug_indices:
            nodes = variant_nodes(r['object_nodes'], shift, a)
            names.append(r['name'] + '_%d' % a)
            instances.append(nodes)
            tables.append(vl.contact_tables(nodes, K, contact_dist, name=names[-1]))
            plan.append((i, first[i], a, rec.frames[i] - first[i]))
            shifts.append(shift)
    empty = lambda *shape, dtype: torch.zeros(shape, dtype=dtype, device=device)       # noqa: E731
    if not plan:
        return done(BuiltSamples(empty(0, rec.J, 3, dtype=torch.float32),
                                 empty(0, rec.J, 10, dtype=torch.float32) if votes else None,
                                 empty(0, dtype=torch.int64), empty(0, dtype=torch.int32),
                                 empty(0, 2, dtype=torch.float64), names, instances, kept, rejected, [], None))
    plan = np.asarray(plan, np.int64)
    out_off = np.zeros(len(plan), np.int64)
    out_off[1:] = np.cumsum(plan[:, 3])[:-1]
    F_out = int(plan[:, 3].sum())
    # one upload for the four integer columns of the plan
    cols = torch.from_numpy(np.ascontiguousarray(plan.T.astype(np.int32))).to(device)
    out_offset = torch.from_numpy(out_off).to(device)
    contact = vl.ContactBoxes(tables, device)
    joints, out_votes = build_packed(rec, cols[0], cols[1], cols[2], out_offset,
                                     torch.from_numpy(np.stack(shifts)).to(device), F_out, contact, votes=votes)
    n_frames = cols[3].contiguous()
    floors = floor_percentile(joints, out_offset, n_frames, max_frames=int(plan[:, 3].max()))
    return done(BuiltSamples(joints, out_votes, out_offset, n_frames, floors, names, instances, kept, rejected,
                             [int(first[i]) for i in kept], contact))
