/* p2r_ap_eval.h -- C ABI of libp2r_ap_eval.so: detection AP on the device (MI355X / gfx950).
 *
 * An extension library next to libp2r_hip.so, built from pose2room_amd/csrc/ap_eval.hip with the same flags
 * (floating-point contraction off).  libp2r_hip.so and its header are unchanged by it: ABI version 3, the same
 * entry points.  Conventions are those of p2r_hip.h: all pointers are DEVICE pointers unless noted, tensors are
 * contiguous row-major, `stream` is a hipStream_t (NULL = default stream), every function returns P2R_OK (0), a
 * hipError_t code, or P2R_EINVAL for sizes outside its limits -- before it touches the device.
 */
#ifndef P2R_AP_EVAL_H
#define P2R_AP_EVAL_H

#include "p2r_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- net_utils/box_util.py, net_utils/eval_det.py: detection AP on the device ---- */

/* replaces box3d_iou (box_util.py:90-118) for every (detection, ground truth) pair of B scans in one launch.
 * det (B,K,8,3), gt (B,G,8,3) f64 corners in the order of get_box_corners (utils/tools.py:33-51) ->
 * iou3d (B,K,G) f64, iou2d (B,K,G) f64 or NULL.  K = G = 1 is the pair-list form.  One lane per pair; footprint
 * corners 3,2,6,7 on (x,z), Sutherland-Hodgman clipping with the strict `inside` predicate (box_util.py:37-38)
 * and the line-intersection expression of :40-46, shoelace area (0 below 3 vertices), height overlap from
 * corners 7 and 4, volumes from three edge lengths -- the operation order of net_utils/box_util.py here,
 * contraction off.  Every loop has a compile-time bound (4 clip edges x 16 vertex slots, surplus vertices are
 * dropped), so NaN and degenerate boxes are ordinary data: their IoU is unspecified, as in the reference.
 * B*K*G must fit in int, K <= 1024, G <= 256 (P2R_EINVAL otherwise). */
int p2r_obb_iou(int B, int K, int G, const double *det, const double *gt, double *iou3d, double *iou2d,
                void *stream);

/* replaces the greedy matching of eval_det_cls_wo_mesh (eval_det.py:259-343) for N scans, C classes and T IoU
 * thresholds in one launch.  iou3d (N,K,G) f64; score (N,K,C) f32 and valid (N,K,C) u8: entry (n,k,c) is a
 * detection of class c iff valid != 0; gt_cls (N,G) i64, gt_mask (N,G) u8 (non-zero = a ground truth);
 * thr (T) f64 ->
 *   tp (T,N,K,C) u8: 1 true positive, 0 false positive, 255 not a detection (every element is written);
 *   npos (N,C) i32: unmasked ground truths of class c in scan n.
 * Per (scan, class) detections are taken in descending score order; each takes the ground truth of its class with
 * the highest IoU (the first index on equal IoU, NaN never wins) and is a true positive iff that IoU > thr and the
 * ground truth is still free.  A detection's best ground truth does not depend on the match state, so the sweep is
 * evaluated in parallel: true positive iff its best IoU > thr and no earlier-ranked detection of the same
 * (scan, class) with the same best ground truth also has its IoU > thr.
 * Equal scores within one (scan, class): the LOWER proposal index goes first (the reference's np.argsort(-score)
 * is not stable and defines no order there).
 * K <= 1024, G <= 256, C <= 64, T <= 8 (P2R_EINVAL otherwise). */
int p2r_ap_match(int N, int K, int G, int C, int T, const double *iou3d, const float *score,
                 const unsigned char *valid, const long long *gt_cls, const unsigned char *gt_mask,
                 const double *thr, unsigned char *tp, int *npos, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* P2R_AP_EVAL_H */
