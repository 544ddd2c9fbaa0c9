/* p2r_mm_eval.h -- C ABI of libp2r_mm_eval.so: multi-modal evaluation on the device (MI355X / gfx950).
 *
 * An extension library next to libp2r_hip.so and libp2r_ap_eval.so, built from pose2room_amd/csrc/mm_eval.hip with the
 * same flags (floating-point contraction off).  The other two libraries and their headers are unchanged by it.
 * Conventions are those of p2r_hip.h: all pointers are DEVICE pointers unless noted, tensors are contiguous
 * row-major, `stream` is a hipStream_t (NULL = default stream), every function returns P2R_OK (0), a hipError_t
 * code, or P2R_EINVAL for sizes outside its limits -- before it touches the device.  An empty problem returns 0 and
 * launches nothing.
 */
#ifndef P2R_MM_EVAL_H
#define P2R_MM_EVAL_H

#include "p2r_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- net_utils/multi_modal_eval.py: dump-record box parameters and TMD on the device ---- */

/* replaces multi_modal_eval.corners_to_params (corners2params, box_util.py:174-204, plus rot2head) for N boxes in one
 * launch, one lane per box, fp64, in that function's operation order: corners (N,8,3) f64 in the order of
 * get_box_corners -> obbs (N,7) f64 = centre, size, heading.  centre = (max + min) / 2 over the corners; half-edge
 * vectors from the corners 0-1, 1-2, 0-4; size = 2 |v|, R = v / (size / 2); row 1 is negated if R[1,1] < 0, row 2 if
 * (R0 x R1) . R2 < 0; heading = atan2(-R[0,2], R[0,0]).  Every output element is written.  Degenerate and NaN boxes
 * are ordinary data: their parameters are unspecified, nothing traps or loops.
 * N >= 0 (P2R_EINVAL otherwise). */
int p2r_box_params(int N, const double *corners, double *obbs, void *stream);

/* replaces multi_modal_eval.tmd's per-(sample, proposal) value (utils/eval/multi_modal_eval.py) for H hypotheses of B
 * samples with K proposals in one launch.  obbs (H,B,K,7) f64 box parameters, keep (H,B,K) u8 (non-zero = hypothesis h
 * kept proposal k of sample b), cls (H,B,K) i64 ->
 *   count (B,K) i32: the number n of hypotheses that kept (b,k);
 *   value (B,K) f64: 0 for n = 0, else (entropy + 1) * (shape + 1) over the kept hypotheses in ascending h:
 *     corners of each kept box as multi_modal_eval.params_to_corners builds them (R rows (cos, 0, -sin), (0, 1, 0),
 *     (sin, 0, cos); vectors size / 2 * R; ((centre +- v0) +- v1) +- v2 in the order of get_box_corners);
 *     pair[i][j] = mean over the 8 corners of the Euclidean distance; shape = sum_ij pair[i][j] / n;
 *     entropy = -sum_c p_c ln p_c / ln 2 over the distinct class labels of the kept entries.
 * Every element of value and count is written.  One wave per (b,k); all arithmetic is fp64, no floating-point atomics,
 * partial sums are combined in a fixed order (two runs give identical bits), every loop has a compile-time bound.
 * 1 <= H <= 64, 0 <= K <= 1024, B >= 0, B*K must fit in int (P2R_EINVAL otherwise). */
int p2r_tmd(int H, int B, int K, const double *obbs, const unsigned char *keep, const long long *cls, double *value,
            int *count, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* P2R_MM_EVAL_H */
