"""Detection AP with its state on the device.

`APCalculator` (ap_helper.py) is the reference's calculator: per-scan Python lists on the host, one IoU pass per class
and per IoU threshold, a Python sweep over the sorted detections.  `DeviceAPCalculator` computes the same metric from
the device tensors `parse_predictions(..., return_device=True)` returns:

  * the IoU of proposal k with ground truth g of the same scan depends neither on the class nor on the threshold, so
    it is computed once per batch (`obb_iou`, csrc/ap_eval.hip: p2r_obb_iou, include/p2r_ap_eval.h);
  * one launch of p2r_ap_match turns it into true-positive flags for every class and every threshold -- the greedy
    sweep of eval_det.eval_det_cls_wo_mesh in its parallel form (a detection is a true positive iff its best IoU
    exceeds the threshold and no earlier-ranked detection of the same (scan, class) with the same best ground truth
    does);
  * `step_tensors` (`match_tensors`, then `append`) adds scores, flags and ground-truth counts to device-side state
    without a device->host copy or a synchronisation; `compute_metrics` sorts per class on the device, crosses to
    the host once with one flag byte per (detection slot, threshold), and finishes with the host expressions
    `APCalculator` uses (eval_det.curve_from_flags, ap_helper.metrics_from_curves).

Equal scores: within one (scan, class) the lower proposal index goes first; across scans the earlier scan.  The
reference's `np.argsort(-score)` is not stable and defines no order there.  No CPU fallback.
"""
import numpy as np
import torch

from .. import _lib
from .ap_helper import boxes_to_corners, metrics_from_curves, parse_predictions
from .eval_det import curve_from_flags

NOT_A_DETECTION = 255      # flag byte of a (proposal, class) slot that holds no detection
MAX_K, MAX_G, MAX_C, MAX_T = 1024, 256, 64, 8      # limits of the entry points (include/p2r_ap_eval.h)

# The two kernels are a library of their own next to libp2r_hip.so (csrc/Makefile), with a header of their own; the
# binding is derived from that header as that of libp2r_hip.so is (_lib.Library).
_library = _lib.extension("ap_eval")
HEADER_PATH, LIB_PATH = _library.header_path, _library.lib_path
lib, _launch = _library.lib, _library.launch


def _need_cuda(what, **tensors):
    for name, t in tensors.items():
        if t is not None and not (torch.is_tensor(t) and t.is_cuda):
            raise RuntimeError(f"{what}: {name} must be a GPU tensor (no CPU fallback)")


def obb_iou(det, gt, want_2d=True):
    """det (B,K,8,3), gt (B,G,8,3) CUDA float64 corners (order of get_box_corners) -> (iou_3d (B,K,G), iou_2d (B,K,G)
    or None) float64: every proposal against every ground truth of its scan.  K = G = 1 is the pair-list form."""
    _need_cuda("obb_iou", det=det, gt=gt)
    if det.dtype != torch.float64 or gt.dtype != torch.float64:
        raise RuntimeError("obb_iou: float64 corners required (the reference computes the IoU in fp64)")
    if det.dim() != 4 or gt.dim() != 4 or det.shape[2:] != (8, 3) or gt.shape[2:] != (8, 3) or det.shape[0] != gt.shape[0]:
        raise ValueError(f"obb_iou: det (B,K,8,3) and gt (B,G,8,3) expected, got {tuple(det.shape)} and {tuple(gt.shape)}")
    det, gt = det.contiguous(), gt.contiguous()
    B, K, G = det.shape[0], det.shape[1], gt.shape[1]
    iou3d = torch.empty((B, K, G), dtype=torch.float64, device=det.device)
    iou2d = torch.empty((B, K, G), dtype=torch.float64, device=det.device) if want_2d else None
    _launch("p2r_obb_iou", det.device, B, K, G, det, gt, iou3d, iou2d)
    return iou3d, iou2d


def ap_match(iou3d, score, valid, gt_cls, gt_mask, thr):
    """iou3d (N,K,G) f64, score (N,K,C) f32, valid (N,K,C) u8, gt_cls (N,G) i64, gt_mask (N,G) u8, thr (T) f64, all
    on the GPU -> (tp (T,N,K,C) u8: 1 true positive / 0 false positive / 255 not a detection, npos (N,C) i32)."""
    _need_cuda("ap_match", iou3d=iou3d, score=score, valid=valid, gt_cls=gt_cls, gt_mask=gt_mask, thr=thr)
    N, K, G = iou3d.shape
    C, T = score.shape[2], thr.shape[0]
    want = ((iou3d, torch.float64, (N, K, G)), (score, torch.float32, (N, K, C)), (valid, torch.uint8, (N, K, C)),
            (gt_cls, torch.int64, (N, G)), (gt_mask, torch.uint8, (N, G)), (thr, torch.float64, (T,)))
    for t, dtype, shape in want:
        if t.dtype != dtype or tuple(t.shape) != shape:
            raise ValueError(f"ap_match: {dtype} tensor of shape {shape} expected, got {t.dtype} {tuple(t.shape)}")
    dev = iou3d.device
    tp = torch.empty((T, N, K, C), dtype=torch.uint8, device=dev)
    npos = torch.empty((N, C), dtype=torch.int32, device=dev)
    _launch("p2r_ap_match", dev, N, K, G, C, T, iou3d.contiguous(), score.contiguous(), valid.contiguous(),
                gt_cls.contiguous(), gt_mask.contiguous(), thr.contiguous(), tp, npos)
    return tp, npos


def sort_flags(score, tp):
    """score (M,C) f32, tp (T,M,C) u8 -> tp with every class column in descending score order, the slots that hold no
    detection last (stable: equal scores keep their (scan, proposal) order).  Any device."""
    key = torch.where(tp[0] != NOT_A_DETECTION, score, torch.full_like(score, float('-inf')))
    order = torch.sort(key, dim=0, descending=True, stable=True).indices
    return torch.gather(tp, 1, order.unsqueeze(0).expand(tp.shape[0], -1, -1))


def curves_from_sorted_flags(flags, npos):
    """One threshold on the host: flags (M,C) u8 sorted as by `sort_flags`, npos (C,) ground-truth counts ->
    ({class: rec}, {class: prec}, {class: ap}) with the class-presence rule of eval_det_multiprocessing_wo_mesh: a
    class appears iff it has a ground truth or a detection anywhere; ground truths but no detection gives 0."""
    rec, prec, ap = {}, {}, {}
    for c in range(flags.shape[1]):
        col = flags[:, c]
        nd = int(np.count_nonzero(col != NOT_A_DETECTION))
        if nd == 0:
            if npos[c] > 0:
                rec[c] = prec[c] = ap[c] = 0
            continue
        tp = (col[:nd] == 1).astype(np.float64)
        rec[c], prec[c], ap[c] = curve_from_flags(tp, 1.0 - tp, int(npos[c]))
    return rec, prec, ap


def match_tensors(pred_corners, pred_mask, obj_prob, sem_cls_scores, pred_sem_cls, gt_corners, gt_cls, gt_mask, thr,
                  num_class=None, per_class_proposal=True, conf_thresh=0.05):
    """One step's tensors -> (score (N,K,C) f32, tp (T,N,K,C) u8, npos (N,C) i32), one `obb_iou` and one `ap_match`
    launch for all N scans: what `DeviceAPCalculator.step_tensors` appends.  The scans are independent, so a slice
    along N is the result of that slice of the inputs (mm_device.py feeds H calculators from one call).
    pred_corners (N,K,8,3) f64, pred_mask (N,K), obj_prob (N,K), sem_cls_scores (N,K,C) or None, pred_sem_cls (N,K),
    gt_corners (N,G,8,3) f64, gt_cls (N,G), gt_mask (N,G), thr (T,) f64: device tensors.  Nothing leaves the device."""
    _need_cuda("DeviceAPCalculator.step_tensors", pred_corners=pred_corners, pred_mask=pred_mask, obj_prob=obj_prob,
               sem_cls_scores=sem_cls_scores, pred_sem_cls=pred_sem_cls, gt_corners=gt_corners, gt_cls=gt_cls,
               gt_mask=gt_mask)
    dev = pred_corners.device
    C = num_class if num_class is not None else (None if sem_cls_scores is None else sem_cls_scores.shape[-1])
    if C is None:
        raise ValueError("DeviceAPCalculator: num_class is unknown (pass num_class, class2type_map or sem_cls_scores)")
    obj = obj_prob.to(torch.float32)
    keep = (pred_mask == 1) & (obj > conf_thresh)                                      # (N,K)
    if per_class_proposal:
        if sem_cls_scores is None or sem_cls_scores.shape[-1] != C:
            raise ValueError(f"DeviceAPCalculator: per-class proposals need sem_cls_scores (B,K,{C})")
        x = sem_cls_scores.to(torch.float32)
        e = torch.exp(x - x.max(dim=-1, keepdim=True).values)                          # ap_helper.softmax
        score = (e / e.sum(dim=-1, keepdim=True)) * obj.unsqueeze(-1)
        valid = keep.unsqueeze(-1).expand(-1, -1, C)
    else:
        own = pred_sem_cls.unsqueeze(-1) == torch.arange(C, device=dev)                # (N,K,C)
        score = obj.unsqueeze(-1) * own.to(torch.float32)
        valid = keep.unsqueeze(-1) & own
    iou3d, _ = obb_iou(pred_corners, gt_corners, want_2d=False)
    score = score.contiguous()
    tp, npos = ap_match(iou3d, score, valid.to(torch.uint8).contiguous(), gt_cls.to(torch.int64),
                        (gt_mask == 1).to(torch.uint8), thr)
    return score, tp, npos


class DeviceAPCalculator(object):
    """AP, mAP, recall and AR of `APCalculator` for one or several IoU thresholds, accumulated on the device.
    ap_iou_thresh: a float (compute_metrics -> one dict) or a sequence of floats (-> a list of dicts, one per
    threshold).  num_class: needed only when neither class scores nor `class2type_map` give it."""

    def __init__(self, ap_iou_thresh=0.25, class2type_map=None, num_class=None, per_class_proposal=True,
                 conf_thresh=0.05):
        self.single = not isinstance(ap_iou_thresh, (list, tuple, np.ndarray))
        self.ap_iou_thresh = [float(ap_iou_thresh)] if self.single else [float(t) for t in ap_iou_thresh]
        if not 1 <= len(self.ap_iou_thresh) <= MAX_T:
            raise ValueError(f"DeviceAPCalculator: 1..{MAX_T} IoU thresholds, got {len(self.ap_iou_thresh)}")
        self.class2type_map = class2type_map
        self.num_class = num_class if num_class is not None else (len(class2type_map) if class2type_map else None)
        self.per_class_proposal = per_class_proposal
        self.conf_thresh = conf_thresh
        self._thr = {}      # device -> (T,) f64
        self.reset()

    def reset(self):
        self._score, self._tp, self._npos = [], [], None
        self.scan_cnt = 0

    def _thresholds(self, dev):
        if dev not in self._thr:        # fill kernels with a scalar argument: no host->device copy to wait for
            self._thr[dev] = torch.stack([torch.full((), t, dtype=torch.float64, device=dev) for t in self.ap_iou_thresh])
        return self._thr[dev]

    def step_tensors(self, pred_corners, pred_mask, obj_prob, sem_cls_scores, pred_sem_cls, gt_corners, gt_cls, gt_mask):
        """pred_corners (B,K,8,3) f64, pred_mask (B,K), obj_prob (B,K), sem_cls_scores (B,K,C) or None, pred_sem_cls
        (B,K), gt_corners (B,G,8,3) f64, gt_cls (B,G), gt_mask (B,G): device tensors.  Detections are formed as
        assembly_pred_map_cls forms them; ground truths are the slots with gt_mask == 1.  Nothing leaves the device."""
        _need_cuda("DeviceAPCalculator.step_tensors", pred_corners=pred_corners)       # its device keys the thresholds
        self.append(*match_tensors(pred_corners, pred_mask, obj_prob, sem_cls_scores, pred_sem_cls, gt_corners, gt_cls,
                                   gt_mask, self._thresholds(pred_corners.device), self.num_class,
                                   self.per_class_proposal, self.conf_thresh))

    def append(self, score, tp, npos):
        """one step's (score (N,K,C), tp (T,N,K,C), npos (N,C)) of `match_tensors`, or a slice of it along N, joins the
        state: N more scans"""
        C = score.shape[-1]
        self._score.append(score.reshape(-1, C))
        self._tp.append(tp.reshape(tp.shape[0], -1, C))
        total = npos.sum(dim=0, dtype=torch.int64)
        self._npos = total if self._npos is None else self._npos + total
        self.scan_cnt += score.shape[0]

    def step_end_points(self, est_data, data, eval_config):
        """est_data: end points of `P2RNet.generate` (or its result tuple); data: the batch, on the device."""
        if isinstance(est_data, tuple):
            est_data = est_data[0]
        eval_dict, parsed = parse_predictions(est_data, data, eval_config, return_device=True)
        mask = data['box_label_mask'].detach()
        gt_heading = torch.atan2(data['heading'][..., 0], data['heading'][..., 1]).detach()
        corners = boxes_to_corners(torch.exp(data['size']).detach(), gt_heading.to(torch.float64),
                                   data['center_label'][:, :, 0:3].detach())
        corners = corners * (mask != 0).to(torch.float64)[:, :, None, None]                # as parse_groundtruths
        self.step_tensors(parsed['pred_corners_3d'], eval_dict['pred_mask'], parsed['obj_prob'], parsed['sem_cls_scores'],
                          parsed['pred_sem_cls'], corners, data['sem_cls_label'].detach(), mask)

    def compute_metrics(self):
        """-> the dict of `APCalculator.compute_metrics` (a list of them for a sequence of thresholds)."""
        T = len(self.ap_iou_thresh)
        if not self._tp:
            flags, npos = np.zeros((T, 0, self.num_class or 0), dtype=np.uint8), np.zeros(self.num_class or 0, dtype=np.int64)
        else:
            flags_d = sort_flags(torch.cat(self._score, 0), torch.cat(self._tp, 1))      # (T,M,C)
            C = flags_d.shape[2]
            packed = torch.cat([flags_d.reshape(-1), self._npos.view(torch.uint8)]).cpu().numpy()      # the one transfer
            flags = packed[:flags_d.numel()].reshape(flags_d.shape)
            npos = packed[flags_d.numel():].copy().view(np.int64)
            assert npos.shape == (C,)
        out = []
        for t in range(T):
            rec, _, ap = curves_from_sorted_flags(flags[t], npos)
            out.append(metrics_from_curves(rec, ap, self.class2type_map))
        return out[0] if self.single else out
