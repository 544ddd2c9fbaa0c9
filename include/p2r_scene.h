/* p2r_scene.h -- C ABI of libp2r_scene.so: the scene read-out on the device (MI355X / gfx950).
 *
 * An extension library next to libp2r_hip.so, libp2r_ap_eval.so, libp2r_mm_eval.so, libp2r_vote_labels.so and
 * libp2r_parse.so, built from pose2room_amd/csrc/scene.hip with the same flags (floating-point contraction off).  The
 * other libraries and their headers are unchanged by it.  Conventions are those of p2r_hip.h: all pointers are DEVICE
 * pointers, tensors are contiguous row-major, `stream` is a hipStream_t (NULL = default stream), every function returns
 * P2R_OK (0), a hipError_t code, or P2R_EINVAL for arguments outside its limits -- before it touches the device.  A
 * problem without an output element returns 0 and launches nothing.  No floating-point atomics: two runs give identical
 * bits.  Every loop is bounded by K, T, J or C.
 */
#ifndef P2R_SCENE_H
#define P2R_SCENE_H

#include "p2r_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define P2R_SCENE_MAX_K 1024          /* proposals per sample */
#define P2R_SCENE_MAX_T 65535         /* frames of p2r_contact_frames (the reference indexes frames with uint16) */
#define P2R_SCENE_MAX_J 64            /* joints per frame */
#define P2R_UNIQUE_MAX_T 4096         /* frames of p2r_unique_frames: three int tables of T entries in LDS (48 KB) */

/* ---- demo.py:204-256 (visualize_step): the confident boxes of every sample as object nodes, compacted ---- */

/* N samples of K proposals in one launch, one workgroup per sample.
 * Inputs: obbs (N,K,7) f64 box parameters centre, size, heading (p2r_box_params), obj_prob (N,K) f32, pred_mask (N,K)
 * u8 (the NMS keep mask), pred_cls (N,K) i64.  Proposal k of sample n is kept iff
 *   (double)obj_prob[n,k] > dump_threshold && pred_mask[n,k] == 1.
 * Outputs, capacity K per sample, every element written by every call: count (N) i32 the number of kept proposals;
 * the kept proposals in ascending proposal index in slots 0 .. count-1: inst_idx (N,K) i32 the proposal index,
 * node_obbs (N,K,7) f64 bit copies of the input rows, node_rmat (N,K,3,3) f64 = head2rot(heading) with rows
 * (cos h, 0, -sin h), (0, 1, 0), (sin h, 0, cos h), node_cls (N,K) i64, node_score (N,K) f32 the objectness
 * probability.  Slots count .. K-1 hold zeros and inst_idx = -1.
 * Slots come from wave ballots and a prefix over the waves of the workgroup: no atomics, no device-wide offset.
 * N >= 0, 0 <= K <= P2R_SCENE_MAX_K, N * K fits int (P2R_EINVAL otherwise, and for a NULL pointer to a tensor that has
 * elements).  N = 0 launches nothing; K = 0 writes count = 0. */
int p2r_scene_nodes(int N, int K, const double *obbs, const float *obj_prob, const unsigned char *pred_mask,
                    const long long *pred_cls, double dump_threshold, int *count, int *inst_idx, double *node_obbs,
                    double *node_rmat, long long *node_cls, float *node_score, void *stream);

/* ---- utils/virtualhome/vis_gt_vh.py:14-22 (dist_node2bbox): the frame in which the body is closest to each node ---- */

/* Inputs: joints (B,T,J,C) f32, C = 3 or 4, only the first three channels are read; node_obbs (N,K,7) f64, node_rmat
 * (N,K,3,3) f64 and count (N) i32 as p2r_scene_nodes writes them (the matrix is READ, not rebuilt from the heading: a
 * caller may pass ground-truth nodes with their stored R_mat).  Sample n reads joints row n % B (N = H * B
 * hypothesis-major stacks read the batch's joints in place).
 * For every slot s < count[n], in fp64, never contracted, with x the f32 coordinates of a joint converted first:
 *   v = x - centroid;  g_a = |(v_0 R[a,0] + v_1 R[a,1]) + v_2 R[a,2]| - size_a / 2 for a = 0, 1, 2;
 *   d(t) = max over the J joints of frame t and the three axes of g_a;
 *   frame[n,s] = the FIRST t that attains min_t d(t), dist[n,s] = that minimum.
 * Slots s >= count[n] get frame = -1 and dist = 0.  Outputs frame (N,K) i32 and dist (N,K) f64, every element written.
 * NaN coordinates are ordinary data: the result of that node is unspecified, nothing traps or loops.
 * One workgroup owns four consecutive slots of a sample, one per wave; the frames pass through LDS in chunks of 64 (one
 * per lane), so a sample's joints are fetched once per four nodes; the minimum over lanes is a fixed-order
 * (value, index) reduction.
 * N >= 0, B >= 1, N % B == 0, 1 <= T <= P2R_SCENE_MAX_T, 1 <= J <= P2R_SCENE_MAX_J, C in {3, 4}, 0 <= K <=
 * P2R_SCENE_MAX_K, N * K fits int (P2R_EINVAL otherwise, and for a NULL pointer when N * K > 0).  N * K = 0 launches
 * nothing. */
int p2r_contact_frames(const float *joints, int B, int T, int J, int C, int N, int K, const double *node_obbs,
                       const double *node_rmat, const int *count, int *frame, double *dist, void *stream);

/* ---- demo.py:234-235: np.sort(np.unique(joints[b], axis=0, return_index=True)[1]) ---- */

/* Input: joints (B,T,J,C) f32; the whole row of J * C values of a frame takes part.  Two rows are equal iff all their
 * elements compare equal with ==: -0.0 equals +0.0, and a row that holds a NaN equals no row, not even itself (NumPy's
 * rule).  Equal rows need not be adjacent.
 * Outputs, every element written: count (B) i32 the number of distinct rows; index (B,T) i32 the ascending indices of
 * the frames that are the first occurrence of their row, -1 from count on; rank (B,T) i32 the position in `index` of
 * the first occurrence of frame t's row (rank translates a frame number into the de-duplicated sequence).
 * One workgroup per sample: a 32-bit hash per row (-0 mapped to +0) in LDS, frame t scans the hashes of the frames
 * before it and confirms an equal hash by comparing the rows, the first occurrences are compacted by ballots.
 * B >= 0, 1 <= T <= P2R_UNIQUE_MAX_T, 1 <= J <= P2R_SCENE_MAX_J, C in {3, 4} (P2R_EINVAL otherwise, and for a NULL
 * pointer when B > 0).  B = 0 launches nothing. */
int p2r_unique_frames(const float *joints, int B, int T, int J, int C, int *count, int *index, int *rank, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* P2R_SCENE_H */
