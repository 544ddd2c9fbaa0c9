"""Prediction parsing in one HIP launch.

`ap_helper.parse_predictions` turns the network's heads into what the NMS and the AP kernels consume with several dozen
ATen launches in float64; its far-box filter (`_far_box_mask`) materialises three (B,K,T,3) float64 tensors to answer one
bit per box.  `parse_boxes` is the same arithmetic as one kernel (csrc/parse_boxes.hip: p2r_parse_boxes,
include/p2r_parse.h): corners, the rows `p2r_nms3d` reads, objectness probability, predicted class and the far-box mask.
Its footprint does not depend on T, and it reads the batch's joints in place -- once for all hypotheses of a stacked
H * B batch (`joints_repeat`), which then needs no H-fold copy of the joints.

`parse_predictions_device` is `parse_predictions(..., return_device=True)` on that kernel plus the one `p2r_nms3d`
launch; `parse_predictions(..., impl='kernel')` and `test.parse_impl: 'kernel'` route through it.  The two paths differ
by the device's `exp` / `atan2` / `cos` / `sin` against ATen's, nothing else.  No CPU fallback.
"""
import torch

from .. import _lib
from . import nms as nms_hip

NMS_3D, NMS_3D_CLS, NMS_2D = 0, 1, 2       # nms_mode of p2r_parse_boxes: rows of 7, rows of 8 with the class, 2-D rows
CHUNK_FRAMES = 256                         # frames the kernel stages per pass through LDS (csrc/parse_boxes.hip: CH)
GROUP_BOXES = 16                           # proposals per workgroup (PB)

# The kernel is a library of its own next to libp2r_hip.so (csrc/Makefile), with a header of its own; the binding is
# derived from that header as that of libp2r_hip.so is (_lib.Library).
_library = _lib.extension("parse")
HEADER_PATH, LIB_PATH = _library.header_path, _library.lib_path
lib = _library.lib


def _want(what, name, t, dtype, shape):
    if not (torch.is_tensor(t) and t.is_cuda):
        raise RuntimeError(f"{what}: {name} must be a GPU tensor (no CPU fallback)")
    if t.dtype != dtype or tuple(t.shape) != tuple(shape):
        raise ValueError(f"{what}: {name} must be {dtype} of shape {tuple(shape)}, got {t.dtype} {tuple(t.shape)}")
    return t.contiguous()


def parse_boxes(center, size_log, heading_sc, objectness, sem_scores, joints=None, cls_in=None, origin_joint=0,
                contact_dist=1.0, remove_far_box=True, nms_mode=NMS_3D):
    """center (N,K,3) f32, size_log (N,K,3) f32, heading_sc (N,K,2) f64 (sin, cos), objectness (N,K,2) f32, sem_scores
    (N,K,C) f32, cls_in (N,K) i64 or None, joints (Bj,T,J,>=3) f32 with N % Bj == 0 (sample n reads row n % Bj; None
    only without the filter), all on one GPU -> (corners (N,K,8,3) f64, boxes (N,K,7|8) f64: the rows of `p2r_nms3d`,
    obj_prob (N,K) f32, pred_cls (N,K) i64, nonempty (N,K) u8).  One launch; include/p2r_parse.h has the arithmetic."""
    what = "parse_boxes"
    if not torch.is_tensor(center) or center.dim() != 3 or center.shape[-1] != 3:
        raise ValueError(f"{what}: center must be (N,K,3)")
    N, K = center.shape[0], center.shape[1]
    if N < 1 or K < 1:
        raise ValueError(f"{what}: N and K must be at least 1, got {N} and {K}")
    if nms_mode not in (NMS_3D, NMS_3D_CLS, NMS_2D):
        raise ValueError(f"{what}: nms_mode must be 0 (3-D), 1 (3-D with the class) or 2 (2-D), got {nms_mode!r}")
    if not torch.is_tensor(sem_scores) or sem_scores.dim() != 3 or sem_scores.shape[-1] < 1:
        raise ValueError(f"{what}: sem_scores must be (N,K,C) with C >= 1")
    C = sem_scores.shape[-1]
    center = _want(what, "center", center, torch.float32, (N, K, 3))
    size_log = _want(what, "size_log", size_log, torch.float32, (N, K, 3))
    heading_sc = _want(what, "heading_sc", heading_sc, torch.float64, (N, K, 2))
    objectness = _want(what, "objectness", objectness, torch.float32, (N, K, 2))
    sem_scores = _want(what, "sem_scores", sem_scores, torch.float32, (N, K, C))
    if cls_in is not None:
        cls_in = _want(what, "cls_in", cls_in, torch.int64, (N, K))
    dev = center.device
    Bj = T = J = 0
    if remove_far_box:
        if not (torch.is_tensor(joints) and joints.is_cuda):
            raise RuntimeError(f"{what}: joints must be a GPU tensor when remove_far_box is set (no CPU fallback)")
        if joints.dtype != torch.float32 or joints.dim() != 4 or joints.shape[-1] < 3 or min(joints.shape[:3]) < 1:
            raise ValueError(f"{what}: joints must be float32 (Bj,T,J,>=3), got {joints.dtype} {tuple(joints.shape)}")
        if not 0 <= origin_joint < joints.shape[2]:
            raise ValueError(f"{what}: origin_joint {origin_joint} outside the {joints.shape[2]} joints")
        if N % joints.shape[0] != 0:
            raise ValueError(f"{what}: {N} samples over {joints.shape[0]} joints rows: N must be a multiple of Bj")
        if joints.shape[-1] != 3 or not joints.is_contiguous():
            # joints with a height column, or a view: the kernel reads rows of 3 floats, so it gets the hip track alone
            joints, origin_joint = joints[:, :, origin_joint:origin_joint + 1, 0:3].contiguous(), 0
        Bj, T, J = joints.shape[:3]
    else:
        joints = None
    tensors = [center, size_log, heading_sc, objectness, sem_scores] + [t for t in (cls_in, joints) if t is not None]
    if any(t.device != dev for t in tensors):
        raise RuntimeError(f"{what}: all tensors must be on one device")
    corners = torch.empty((N, K, 8, 3), dtype=torch.float64, device=dev)
    boxes = torch.empty((N, K, 8 if nms_mode == NMS_3D_CLS else 7), dtype=torch.float64, device=dev)
    obj_prob = torch.empty((N, K), dtype=torch.float32, device=dev)
    pred_cls = torch.empty((N, K), dtype=torch.int64, device=dev)
    nonempty = torch.empty((N, K), dtype=torch.uint8, device=dev)
    _library.launch("p2r_parse_boxes", dev, center, size_log, heading_sc, objectness, sem_scores, cls_in, joints, N, K, C,
                    Bj, T, J, int(origin_joint), float(contact_dist), int(bool(remove_far_box)), int(nms_mode), corners,
                    boxes, obj_prob, pred_cls, nonempty)
    return corners, boxes, obj_prob, pred_cls, nonempty


def parse_predictions_device(est_data, gt_data, config_dict, joints_repeat=1):
    """`ap_helper.parse_predictions(est_data, gt_data, config_dict, return_device=True)` with one `p2r_parse_boxes` and
    one `p2r_nms3d` launch: the same keys, dtypes and shapes.  joints_repeat = H: est_data is an H * B hypothesis-major
    stack and gt_data['input_joints'] the B rows of the batch, unexpanded."""
    dataset_config = config_dict['dataset_config']
    center = est_data['center'].detach()
    sem_scores = est_data['sem_cls_scores'].detach()
    cls_in = None
    if config_dict['sample_cls']:
        cls_in = torch.distributions.Categorical(torch.softmax(sem_scores, dim=-1)).sample()
    if not config_dict['use_3d_nms']:
        mode, same_cls = NMS_2D, False
    elif not config_dict['cls_nms']:
        mode, same_cls = NMS_3D, False
    else:
        mode, same_cls = NMS_3D_CLS, True
    joints = None
    if config_dict['remove_far_box']:
        joints = gt_data['input_joints'].detach().to(center.device)
        if joints.shape[0] * joints_repeat != center.shape[0]:
            raise ValueError(f"parse_predictions_device: {joints.shape[0]} joints rows x joints_repeat {joints_repeat} "
                             f"for {center.shape[0]} samples")
    corners, boxes, obj_prob, pred_cls, nonempty = parse_boxes(
        center, est_data['size'].detach(), est_data['heading'].detach(), est_data['objectness_scores'].detach(),
        sem_scores, joints=joints, cls_in=cls_in, origin_joint=dataset_config.origin_joint_id,
        contact_dist=dataset_config.contact_dist_thresh, remove_far_box=config_dict['remove_far_box'], nms_mode=mode)
    keep, _, npick = nms_hip.nms_3d_batched(boxes, config_dict['nms_iou'], config_dict['use_old_type_nms'], same_cls,
                                            valid=nonempty, return_pick=True)
    assert bool((npick > 0).all()), "NMS kept no box for some sample (reference: assert len(pick) > 0)"
    return {'pred_mask': keep}, {'pred_corners_3d': corners, 'obj_prob': obj_prob, 'pred_sem_cls': pred_cls,
                                 'sem_cls_scores': sem_scores}
