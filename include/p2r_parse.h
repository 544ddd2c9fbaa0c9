/* p2r_parse.h -- C ABI of libp2r_parse.so: prediction parsing on the device (MI355X / gfx950).
 *
 * An extension library next to libp2r_hip.so, libp2r_ap_eval.so, libp2r_mm_eval.so and libp2r_vote_labels.so, built
 * from pose2room_amd/csrc/parse_boxes.hip with the same flags (floating-point contraction off).  The other libraries
 * and their headers are unchanged by it.  Conventions are those of p2r_hip.h: all pointers are DEVICE pointers, tensors
 * are contiguous row-major, `stream` is a hipStream_t (NULL = default stream), every function returns P2R_OK (0), a
 * hipError_t code, or P2R_EINVAL for arguments outside its limits -- before it touches the device.
 */
#ifndef P2R_PARSE_H
#define P2R_PARSE_H

#include "p2r_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- net_utils/ap_helper.py:133-214 (parse_predictions up to the NMS): heads -> corners, NMS rows, far-box mask ---- */

/* N samples of K proposals in one launch.
 * Inputs: center (N, K, 3) f32, size_log (N, K, 3) f32 (the size head: log of the extents), heading_sc (N, K, 2) f64
 * (sin, cos), objectness (N, K, 2) f32 logits, sem_scores (N, K, C) f32 class scores, cls_in (N, K) i64 or NULL,
 * joints (Bj, T, J, 3) f32, read in place: sample n takes the positions of joint `origin_joint` of row n % Bj (N = H * Bj
 * hypothesis-major stacks read the batch's joints without a copy).  joints may be NULL when remove_far_box = 0 (Bj, T, J
 * and origin_joint are then ignored); sem_scores may be NULL when cls_in is given.
 *
 * Arithmetic, never contracted; f32 where it says so, f64 elsewhere:
 *   size = expf(size_log) (f32);  theta = atan2(sc0, sc1), c = cos theta, s = sin theta;  half = f64(size / 2) with the
 *   division in f32;  R0 = (c, 0, -s), R1 = (0, 1, 0), R2 = (s, 0, c);
 *   corner i = ((f64(centre) + g0 * (half0 * R0)) + g1 * (half1 * R1)) + g2 * (half2 * R2), (g0, g1, g2) the i-th of
 *     (-1,-1,-1) (+1,-1,-1) (+1,+1,-1) (-1,+1,-1) (-1,-1,+1) (+1,-1,+1) (+1,+1,+1) (-1,+1,+1);
 *   mins / maxs = min / max over the eight corners (a NaN stays);
 *   obj_prob = e1 / (e0 + e1) in f32 with e_i = expf(logit_i - max(logit_0, logit_1));
 *   pred_cls = cls_in, or without it the index of the first maximum of the C scores (a NaN counts as the maximum);
 *   far-box test (remove_far_box != 0): ok = no size component < 0.01f or > 10f;
 *     hf = f64(f32(size / 2) + f32(contact_dist)), both in f32;  for the position p of every frame: r = f64(p) -
 *     f64(centre), l0 = r.x * c + r.z * (-s), l1 = r.y, l2 = r.x * s + r.z * c, inside iff |l_i| <= hf_i for i = 0, 1, 2;
 *     nonempty = ok and some frame is inside.  remove_far_box = 0: nonempty = 1.
 * Outputs, every element written by every call: corners (N, K, 8, 3) f64, obj_prob (N, K) f32, pred_cls (N, K) i64,
 * nonempty (N, K) u8, and boxes, the rows p2r_nms3d reads, by nms_mode:
 *   0: (N, K, 7) f64 [mins, maxs, f64(obj_prob)];  1: (N, K, 8) f64, the same and f64(pred_cls);
 *   2: (N, K, 7) f64 [mins.x, 0, mins.z, maxs.x, 1, maxs.z, f64(obj_prob)] (the 2-D NMS on x and z as a 3-D one).
 *
 * One workgroup owns one sample and 16 consecutive proposals; the positions of the sample pass through LDS in chunks of
 * 256 frames, so the footprint does not depend on T.  No atomics, no scratch buffer; every loop is bounded by T, K or C.
 * N, K >= 1, C >= 1 when cls_in is NULL, nms_mode 0..2, N * ceil(K / 16) < 2^31; with remove_far_box also Bj, T, J >= 1,
 * 0 <= origin_joint < J and Bj * T * J < 2^40 (P2R_EINVAL otherwise, and for a NULL pointer that is needed). */
int p2r_parse_boxes(const float *center, const float *size_log, const double *heading_sc, const float *objectness,
                    const float *sem_scores, const long long *cls_in, const float *joints, int N, int K, int C, int Bj,
                    int T, int J, int origin_joint, double contact_dist, int remove_far_box, int nms_mode,
                    double *corners, double *boxes, float *obj_prob, long long *pred_cls, unsigned char *nonempty,
                    void *stream);

#ifdef __cplusplus
}
#endif
#endif /* P2R_PARSE_H */
