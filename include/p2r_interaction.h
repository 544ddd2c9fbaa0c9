/* p2r_interaction.h -- C ABI of libp2r_interaction.so: the interaction timeline of a scene on the device (MI355X /
 * gfx950): in which frames the body is in contact with which object node, and with which joints.
 *
 * An extension library next to libp2r_hip.so and the read-out libraries (libp2r_scene.so, libp2r_consensus.so,
 * libp2r_occupancy.so, ...), built from pose2room_amd/csrc/interaction.hip with the same flags (floating-point
 * contraction off).  The other libraries and their headers are unchanged by it.  Conventions are those of p2r_scene.h:
 * all pointers are DEVICE pointers, tensors are contiguous row-major, `stream` is a hipStream_t (NULL = default stream),
 * every function returns P2R_OK (0), a hipError_t code, or P2R_EINVAL for arguments outside its limits -- before it
 * touches the device.  Every element of every output is written by every call.  A problem without an output element
 * returns 0 and launches nothing.  No floating-point atomics: two runs give identical bits.  Every loop is bounded by K,
 * T, J, W or M.
 *
 * Frames are bit-packed: W = (T + 63) / 64 words of 64 bits per node, frame t is bit t % 64 of word t / 64, the bits at T
 * and beyond in the last word are 0.  Sample n reads joints row n % B (N = H * B hypothesis-major stacks read the batch's
 * joints in place).  Slot s of sample n holds a node iff s < count[n] (and s < K).
 */
#ifndef P2R_INTERACTION_H
#define P2R_INTERACTION_H

#include "p2r_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define P2R_INTERACTION_MAX_K 1024    /* nodes per sample (P2R_SCENE_MAX_K) */
#define P2R_INTERACTION_MAX_T 65535   /* frames (P2R_SCENE_MAX_T) */
#define P2R_INTERACTION_MAX_J 64      /* joints per frame: joint_mask is one word */
#define P2R_INTERACTION_MAX_M 64      /* intervals stored per node */

/* ---- utils/virtualhome/3_generate_samples.py:56-64 (get_votes): the enlarged-box test, per node and frame ---- */

/* Inputs: joints (B,T,J,C) f32, C = 3 or 4, only the first three channels are read; node_obbs (N,K,7) f64, node_rmat
 * (N,K,3,3) f64 and count (N) i32 as p2r_scene_nodes writes them (the matrix is READ, not rebuilt from the heading: a
 * caller may pass ground-truth nodes with their stored R_mat); contact_thresh f64.
 * Joint p (f32, widened to f64 first) is IN node (c, size, R), all arithmetic f64 and never contracted, iff
 *   d = p - c;  local_a = ((0.0 + d0 R[a][0]) + d1 R[a][1]) + d2 R[a][2];  half_a = size_a / 2.0 + contact_thresh;
 *   |local_a| <= half_a for a = 0, 1, 2
 * -- the expression of p2r_vote_labels.h.  A NaN coordinate is inside nothing.
 * Outputs: bits (N,K,W) i64: bit t is set iff any joint of frame t is in; njoint (N,K,T) u8 how many joints of frame t
 * are in, may be NULL (not written then); joint_mask (N,K) i64: bit j is set iff joint j is in during any frame; n_raw
 * (N,K) i32 the number of set bits of the node.  Slots s >= count[n] get zeros everywhere.
 * One workgroup owns four consecutive slots of a sample, one per wave; the frames pass through LDS in chunks of 64 (one
 * per lane); one ballot per chunk is one word of `bits`, stored by one lane; the joint mask is an OR across the lanes.
 * N >= 0, B >= 1, N % B == 0, 1 <= T <= P2R_INTERACTION_MAX_T, 1 <= J <= P2R_INTERACTION_MAX_J, C in {3, 4}, 0 <= K <=
 * P2R_INTERACTION_MAX_K, N * K * T fits int (P2R_EINVAL otherwise, and for a NULL pointer other than njoint
 * when N * K > 0).  N * K = 0 launches nothing.  One launch. */
int p2r_contact_bits(const float *joints, int B, int T, int J, int C, int N, int K, const double *node_obbs,
                     const double *node_rmat, const int *count, double contact_thresh, long long *bits,
                     unsigned char *njoint, long long *joint_mask, int *n_raw, void *stream);

/* ---- per-frame contact into intervals ---- */

/* Inputs: bits (N,K,W) i64 as p2r_contact_bits writes them (bits at T and beyond are ignored), count (N) i32.  Per node,
 * in this order: (1) the raw runs of set bits as [start, end); (2) neighbouring runs are merged while start_next -
 * end_prev <= merge_gap; (3) merged runs with end - start < min_len are dropped.
 * Outputs: clean (N,K,W) i64 the bits of the surviving runs, merged gaps filled; n_intervals (N,K) i32 the number of
 * surviving runs, also when it exceeds M; intervals (N,K,M,2) i32 the first M of them in ascending order as (start, end),
 * -1 beyond; n_frames (N,K) i32 the number of set bits of clean; first, last (N,K) i32 the first and the last frame of
 * clean, -1 if there is none.  A slot s >= count[n] is a node without contact: zeros, -1 in intervals, first and last; its
 * bits are not read.
 * One wave per node, lane = word, a carry between chunks of 64 words; the neighbours of a run across word boundaries are
 * found with clz / ctz; slots come from popcounts and a prefix over the lanes.  No atomics.
 * N, K, T as above, 0 <= merge_gap <= T, 1 <= min_len <= T, 1 <= M <= P2R_INTERACTION_MAX_M, N * K * T and N * K * M * 2
 * fit int (P2R_EINVAL otherwise, and for a NULL pointer when N * K > 0).  N * K = 0 launches nothing.  One launch. */
int p2r_contact_intervals(const long long *bits, const int *count, int N, int K, int T, int merge_gap, int min_len,
                          int M, long long *clean, int *n_intervals, int *intervals, int *n_frames, int *first,
                          int *last, void *stream);

/* ---- one label per frame: the node the body is most in contact with ---- */

/* Inputs: clean (N,K,W) i64, njoint (N,K,T) u8 (required), count (N) i32.
 * Outputs: label (N,T) i32: among the slots s < count[n] whose clean bit t is set the one with the largest
 * njoint[n,s,t], ties to the lowest slot, -1 if there is none; n_active (N,T) u8 how many slots have the bit, saturating
 * at 255; n_labelled (N) i32 the number of frames with a label.
 * One thread per (n, t): the word of a slot is uniform over the wave.  n_labelled is cleared on the stream and summed with
 * one integer atomicAdd of a ballot's popcount per wave.
 * N, K, T as above (P2R_EINVAL otherwise, and for a NULL pointer: count, label, n_active, n_labelled when
 * N > 0; clean, njoint when N * K > 0).  N = 0 launches nothing; K = 0 writes -1, 0, 0.  One clear and one launch. */
int p2r_frame_labels(const long long *clean, const unsigned char *njoint, const int *count, int N, int K, int T,
                     int *label, unsigned char *n_active, int *n_labelled, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* P2R_INTERACTION_H */
