/* p2r_vote_labels.h -- C ABI of libp2r_vote_labels.so: vote labels derived on the device (MI355X / gfx950).
 *
 * An extension library next to libp2r_hip.so, libp2r_ap_eval.so and libp2r_mm_eval.so, built from
 * pose2room_amd/csrc/vote_labels.hip with the same flags (floating-point contraction off).  The other libraries and
 * their headers are unchanged by it.  Conventions are those of p2r_hip.h: all pointers are DEVICE pointers unless
 * noted, tensors are contiguous row-major, `stream` is a hipStream_t (NULL = default stream), every function returns
 * P2R_OK (0), a hipError_t code, or P2R_EINVAL for arguments outside its limits -- before it touches the device.
 */
#ifndef P2R_VOTE_LABELS_H
#define P2R_VOTE_LABELS_H

#include "p2r_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- utils/virtualhome/3_generate_samples.py:56-79,176-187 (get_votes): the vote rows of a pose sequence ---- */

/* The contact boxes of N samples, K slots each, of which sample i uses the first n_boxes[i] (clamped to 0..K) in list
 * order: centroid (N, K, 3) f64, R_mat (N, K, 9) f64 row-major with orthonormal rows, half (N, K, 3) f64 = size / 2 +
 * contact distance as the host computes it, n_boxes (N) i32.  0 <= K <= 256; the three tables may be NULL when K = 0.
 *
 * The vote row of a joint p (f32, widened to f64), all arithmetic f64 and never contracted; for box i = 0 .. n-1:
 *   d = p - c;  local_a = ((0.0 + d0 R[a][0]) + d1 R[a][1]) + d2 R[a][2];  inside_i = |local_a| <= half_a for a = 0, 1, 2;
 *   vote_i = f32(c - p);  with hits = the number of earlier boxes that contain p, on inside_i: column 0 = 1, slot
 *   min(hits, 2) (columns 1 + 3 slot .. 3 + 3 slot) = vote_i, and slots 1 and 2 = vote_i too when hits = 0.
 * A joint inside no box has ten +0.0f.  A NaN coordinate is inside nothing. */
typedef struct p2r_contact_boxes {
  const double *centroid, *R_mat, *half;
  const int *n_boxes;
  int K;
} p2r_contact_boxes;

/* The vote rows of a whole packed store in one launch: joints (F, J, 3) f32, frame_offset (N) i64 ascending, n_frames
 * (N) i32 (the layout of p2r_sample_store; F = n_frames_total) -> votes (F, J, 10) f32.  Every element of votes is
 * written; a frame that belongs to no sample gets zeros.  A workgroup owns 256 consecutive (frame, joint) items of the
 * packed store and finds the samples they belong to by a search of frame_offset (the host need not know the frame
 * counts); no atomics, the box loop is bounded by K.  `boxes` is a HOST struct of device pointers.
 * n_samples >= 1, J >= 1, n_frames_total >= 1, F * J < 2^39 (P2R_EINVAL otherwise, and for a NULL pointer). */
int p2r_vote_labels(const float *joints, const long long *frame_offset, const int *n_frames, int n_samples, int J,
                    long long n_frames_total, const p2r_contact_boxes *boxes, float *votes, void *stream);

/* p2r_assemble_batch for a store without votes (store->votes must be NULL, P2R_EINVAL otherwise): the vote row of each
 * gathered (frame, joint) item is derived in registers from the stored joint and the contact boxes of its sample
 * (boxes: one table row per store sample), in the sample's stored frame, and then goes through exactly the transform
 * p2r_assemble_batch applies to a loaded row.  Arguments, limits and outputs as p2r_assemble_batch; B = 0 returns
 * P2R_OK and launches nothing. */
int p2r_assemble_batch_lean(const p2r_sample_store *store, const p2r_contact_boxes *boxes, int B, const long long *sel,
                            const double *aug, int augment, int use_height, int num_frames, const p2r_batch_out *out,
                            void *stream);

#ifdef __cplusplus
}
#endif
#endif /* P2R_VOTE_LABELS_H */
