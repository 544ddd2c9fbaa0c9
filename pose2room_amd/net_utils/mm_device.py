"""Multi-modal evaluation with its state on the device: best-of-N mAP, TMD and the dump records.

`testing.test_multi_modal(impl='host')` evaluates the hypotheses of `P2RNet.generate_hypotheses` as the reference
evaluates its runs: H x T host `APCalculator`s, every hypothesis' predictions copied to the host,
`multi_modal_eval.confident_boxes` per sample and `multi_modal_eval.tmd` over a Python dict of every
(sample, proposal, run).  `DeviceMultiModalEvaluator` computes the same numbers from the device tensors
`generate_hypotheses(..., return_device=True)` returns:

  * the H hypotheses of a batch are H * B scans of ONE `obb_iou` and ONE `ap_match` launch (ap_device.match_tensors,
    the ground truth expanded over H); hypothesis h's `DeviceAPCalculator` gets its slice of the result;
  * `box_params` (csrc/mm_eval.hip: p2r_box_params, include/p2r_mm_eval.h) is `multi_modal_eval.corners_to_params`
    for every proposal of every hypothesis in one launch;
  * `tmd_values` (p2r_tmd) is the TMD value of every (sample, proposal) over the hypotheses that kept it, and their
    number, in one launch -- the dense form of `multi_modal_eval.tmd`: a (sample, proposal) is present iff at least
    one hypothesis kept it;
  * `step_tensors` makes no device->host copy and no synchronisation; `compute` crosses to the host once per
    calculator and once for the two TMD scalars; `records` rebuilds the host dump records on demand.

No CPU fallback.
"""
import numpy as np
import torch

from .. import _lib
from . import ap_device
from .ap_device import DeviceAPCalculator, _need_cuda

MAX_H, MAX_K = 64, 1024        # limits of p2r_tmd (include/p2r_mm_eval.h)

# The two kernels are a third library next to libp2r_hip.so and libp2r_ap_eval.so (csrc/Makefile), with a header of
# their own; the binding is derived from that header as that of libp2r_hip.so is (_lib.Library).
_library = _lib.extension("mm_eval")
HEADER_PATH, LIB_PATH = _library.header_path, _library.lib_path
lib, _launch = _library.lib, _library.launch


def box_params(corners):
    """corners (..., 8, 3) CUDA float64 in the order of get_box_corners -> (..., 7) float64 centre, size, heading:
    `multi_modal_eval.corners_to_params` of every box in one launch."""
    _need_cuda("box_params", corners=corners)
    if corners.dtype != torch.float64:
        raise RuntimeError("box_params: float64 corners required (the host code computes the parameters in fp64)")
    if corners.dim() < 2 or corners.shape[-2:] != (8, 3):
        raise ValueError(f"box_params: corners (..., 8, 3) expected, got {tuple(corners.shape)}")
    corners = corners.contiguous()
    obbs = torch.empty(corners.shape[:-2] + (7,), dtype=torch.float64, device=corners.device)
    _launch("p2r_box_params", corners.device, obbs.numel() // 7, corners, obbs)
    return obbs


def tmd_values(obbs, keep, cls):
    """obbs (H,B,K,7) f64 box parameters, keep (H,B,K) bool / u8 (non-zero: hypothesis h kept proposal k of sample b),
    cls (H,B,K) integer labels, all on the GPU -> (value (B,K) f64, count (B,K) i32): the number of hypotheses that
    kept each (sample, proposal) and its TMD value over them, 0 where none did."""
    _need_cuda("tmd_values", obbs=obbs, keep=keep, cls=cls)
    if obbs.dtype != torch.float64:
        raise RuntimeError("tmd_values: float64 box parameters required (the host code computes the TMD in fp64)")
    if obbs.dim() != 4 or obbs.shape[3] != 7 or keep.shape != obbs.shape[:3] or cls.shape != obbs.shape[:3]:
        raise ValueError(f"tmd_values: obbs (H,B,K,7), keep (H,B,K), cls (H,B,K) expected, got {tuple(obbs.shape)}, "
                         f"{tuple(keep.shape)}, {tuple(cls.shape)}")
    H, B, K = keep.shape
    if not (1 <= H <= MAX_H and K <= MAX_K):
        raise ValueError(f"tmd_values: 1..{MAX_H} hypotheses and at most {MAX_K} proposals, got H={H}, K={K}")
    dev = obbs.device
    value = torch.empty((B, K), dtype=torch.float64, device=dev)
    count = torch.empty((B, K), dtype=torch.int32, device=dev)
    _launch("p2r_tmd", dev, H, B, K, obbs.contiguous(), (keep != 0).to(torch.uint8).contiguous(),
            cls.to(torch.int64).contiguous(), value, count)
    return value, count


class DeviceMultiModalEvaluator(object):
    """Best-of-N mAP, TMD and dump records of `num_hypotheses` hypotheses, accumulated on the device.
    ap_iou_thresholds: the IoU thresholds (a sequence); class2type_map, num_class, per_class_proposal, conf_thresh: as
    `DeviceAPCalculator`; dump_threshold: a proposal is in hypothesis h's dump record iff the NMS mask is 1 and its
    objectness exceeds it (multi_modal_eval.confident_boxes)."""

    def __init__(self, num_hypotheses, ap_iou_thresholds, class2type_map=None, num_class=None, per_class_proposal=True,
                 conf_thresh=0.05, dump_threshold=0.5):
        if not 1 <= num_hypotheses <= MAX_H:
            raise ValueError(f"DeviceMultiModalEvaluator: 1..{MAX_H} hypotheses, got {num_hypotheses}")
        self.num_hypotheses = int(num_hypotheses)
        self.dump_threshold = dump_threshold
        self.calculators = [DeviceAPCalculator(list(ap_iou_thresholds), class2type_map, num_class, per_class_proposal,
                                               conf_thresh) for _ in range(self.num_hypotheses)]
        self.reset()

    def reset(self):
        for calc in self.calculators:
            calc.reset()
        self._value, self._count = [], []                  # per step: (B,K) f64, (B,K) i32
        self._obbs, self._keep, self._cls = [], [], []     # per step: (H,B,K,7) f64, (H,B,K) bool, (H,B,K) i64

    def step_tensors(self, pred_corners, pred_mask, obj_prob, sem_cls_scores, pred_sem_cls, gt_corners, gt_cls, gt_mask):
        """One batch: pred_corners (H,B,K,8,3) f64, pred_mask (H,B,K), obj_prob (H,B,K), sem_cls_scores (H,B,K,C) or
        None, pred_sem_cls (H,B,K), and the batch's ground truth gt_corners (B,G,8,3) f64, gt_cls (B,G), gt_mask (B,G):
        device tensors.  Nothing leaves the device."""
        _need_cuda("DeviceMultiModalEvaluator.step_tensors", pred_corners=pred_corners, pred_mask=pred_mask,
                   obj_prob=obj_prob, sem_cls_scores=sem_cls_scores, pred_sem_cls=pred_sem_cls, gt_corners=gt_corners,
                   gt_cls=gt_cls, gt_mask=gt_mask)
        H = self.num_hypotheses
        if pred_corners.dim() != 5 or pred_corners.shape[0] != H or gt_corners.shape[0] != pred_corners.shape[1]:
            raise ValueError(f"DeviceMultiModalEvaluator: pred_corners ({H},B,K,8,3) and gt_corners (B,G,8,3) expected, "
                             f"got {tuple(pred_corners.shape)} and {tuple(gt_corners.shape)}")
        B = pred_corners.shape[1]
        flat = lambda t: None if t is None else t.reshape(H * B, *t.shape[2:])                      # noqa: E731
        over_h = lambda t: t.unsqueeze(0).expand(H, *t.shape).reshape(H * B, *t.shape[1:])          # noqa: E731
        first = self.calculators[0]
        score, tp, npos = ap_device.match_tensors(
            flat(pred_corners), flat(pred_mask), flat(obj_prob), flat(sem_cls_scores), flat(pred_sem_cls),
            over_h(gt_corners), over_h(gt_cls), over_h(gt_mask), first._thresholds(pred_corners.device),
            first.num_class, first.per_class_proposal, first.conf_thresh)
        for h, calc in enumerate(self.calculators):
            sl = slice(h * B, (h + 1) * B)
            calc.append(score[sl], tp[:, sl], npos[sl])
        keep = (pred_mask == 1) & (obj_prob.to(torch.float32) > self.dump_threshold)                # (H,B,K)
        obbs = box_params(pred_corners)
        value, count = tmd_values(obbs, keep, pred_sem_cls)
        self._value.append(value)
        self._count.append(count)
        self._obbs.append(obbs)
        self._keep.append(keep)
        self._cls.append(pred_sem_cls.to(torch.int64))

    def compute(self):
        """-> {'metrics': [h][t] metric dicts of `APCalculator.compute_metrics`, 'best_map': (T,) max over hypotheses
        of each threshold's mAP, 'tmd': the mean TMD value over every (sample, proposal) kept by at least one
        hypothesis -- NaN when there is none (np.mean([]), what the host code returns)}."""
        from .multi_modal_eval import best_of_n_map
        metrics = [calc.compute_metrics() for calc in self.calculators]
        total, present = 0.0, 0.0
        if self._value:
            sums = torch.stack([torch.cat([v.reshape(-1) for v in self._value]).sum(),
                                torch.cat([c.reshape(-1) for c in self._count]).gt(0).sum().to(torch.float64)])
            total, present = sums.cpu().tolist()                                                    # the one transfer
        return {'metrics': metrics, 'best_map': best_of_n_map(metrics),
                'tmd': total / present if present > 0 else float('nan')}

    def records(self):
        """-> [h][sample] {'obbs' (M,7) f64, 'cls' (M,) i64, 'inst_idx' (K,) bool}: the dump records of
        `multi_modal_eval.confident_boxes`, hypothesis by hypothesis, samples in the order they were fed."""
        out = [[] for _ in range(self.num_hypotheses)]
        for obbs_d, keep_d, cls_d in zip(self._obbs, self._keep, self._cls):
            obbs, keep, cls = obbs_d.cpu().numpy(), keep_d.cpu().numpy(), cls_d.cpu().numpy()
            for h in range(self.num_hypotheses):
                for b in range(keep.shape[1]):
                    k = keep[h, b]
                    out[h].append({'obbs': obbs[h, b][k, :], 'cls': cls[h, b][k], 'inst_idx': k})
        return out
