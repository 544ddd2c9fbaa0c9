/* p2r_sample_build.h -- C ABI of libp2r_sample_build.so: trainable samples made of raw recordings on the device
 * (MI355X / gfx950).
 *
 * An extension library next to libp2r_hip.so, libp2r_ap_eval.so, libp2r_mm_eval.so, libp2r_vote_labels.so,
 * libp2r_parse.so and libp2r_scene.so, built from pose2room_amd/csrc/sample_build.hip with the same flags
 * (floating-point contraction off).  The other libraries and their headers are unchanged by it.  Conventions are those of
 * p2r_vote_labels.h: all pointers are DEVICE pointers unless noted, tensors are contiguous row-major, `stream` is a
 * hipStream_t (NULL = default stream), every function returns P2R_OK (0), a hipError_t code, or P2R_EINVAL for
 * arguments outside its limits -- before it touches the device.  Every output element is written by every call.  No
 * floating-point atomics (the only atomics are integer counts in LDS): two runs give identical bits.  Every loop is
 * bounded by max_frames, J, K (<= 256), the 256 bins of a radix pass, or the samples that the 256 items of a workgroup
 * span: at most 256 for a plan whose out_offset ascends strictly, at most S when out_offset repeats.
 *
 * This is stage 3 of the reference's data preparation (utils/virtualhome/3_generate_samples.py, run(), lines 96-187):
 * a raw recording -- a pose sequence in world coordinates, the box of its room, the boxes of its objects -- loses the
 * leading frames in which the body is not yet in the room, is rejected when it never comes near an object, moves to the
 * room's floor centre and leaves as 8 flip / quarter-turn variants, each with its vote labels.  The host computes the
 * per-box rows (O(boxes)); all per-frame work is here.  Between p2r_recording_scan and p2r_build_samples the host reads
 * back `first` and `status` (8 bytes per recording) to size the output: that one crossing is part of the design.
 */
#ifndef P2R_SAMPLE_BUILD_H
#define P2R_SAMPLE_BUILD_H

#include "p2r_vote_labels.h"

#ifdef __cplusplus
extern "C" {
#endif

#define P2R_SB_MAX_FRAMES 65535       /* frames of a recording or a sample (the reference's uint16 frame indices) */
#define P2R_SB_MAX_J 256              /* joints per frame: frames * J < 2^24, so float32(n - 1) below is exact */

/* R recordings packed back to back: joints (n_frames_total, J, 3) f64 world coordinates, recording r holds the frames
 * frame_offset[r] .. frame_offset[r] + n_frames[r] - 1.  max_frames is the HOST's bound on the frame counts: a
 * recording whose count lies outside 1 .. max_frames, or whose frames do not lie inside 0 .. n_frames_total - 1, is
 * treated as one without frames (it reads nothing).  A HOST struct of device pointers.
 * R >= 1, 1 <= J <= P2R_SB_MAX_J, 1 <= max_frames <= P2R_SB_MAX_FRAMES, n_frames_total >= 1. */
typedef struct p2r_recordings {
  const double *joints;
  const long long *frame_offset;
  const int *n_frames;
  long long n_frames_total;
  int R, J, max_frames;
} p2r_recordings;

/* ---- 3_generate_samples.py:96-124: where the body enters the room, and whether it ever comes near an object ---- */

/* room (R, 15) f64: per recording the room's centroid (3), R_mat (9, row-major) and half = size / 2 (3).  objects: a
 * p2r_contact_boxes of R rows, the object boxes of each recording with half = (size + 2 * contact distance) / 2.
 * With p the origin joint (0 <= origin_joint < J) of a frame, all arithmetic f64 and never contracted:
 *   d = p - c;  local_a = ((0.0 + d0 R[a][0]) + d1 R[a][1]) + d2 R[a][2];  inside = |local_a| <= half_a for a = 0, 1, 2
 * (vhome_utils.py:274-283, check_in_box).  first[r] = the smallest frame whose origin joint is inside the room, -1 if
 * there is none.  status[r]: bit 0 = never in the room; bit 1 = near no object: no frame f >= first[r] has its origin
 * joint inside one of the recording's object boxes (set as well when there is no such frame or no object); bit 2 = a
 * coordinate of ANY joint of ANY frame of the recording is not finite.  A NaN coordinate is inside nothing.
 * One workgroup per recording; the minimum over frames is a fixed-order reduction (wave shuffles, then LDS).
 * P2R_EINVAL for a NULL pointer, an origin joint outside 0 .. J-1 and a `rec` or `objects` outside its limits. */
int p2r_recording_scan(const p2r_recordings *rec, int origin_joint, const double *room,
                       const p2r_contact_boxes *objects, int *first, int *status, void *stream);

/* ---- 3_generate_samples.py:126-187: recentre, the flip / quarter-turn variants, the votes ---- */

/* S output samples: sample s is recording recording[s] from frame first[s] on, in variant variant[s] (0 .. 7), and
 * occupies the output frames out_offset[s] .. out_offset[s] + n_frames[recording[s]] - first[s] - 1 (out_offset
 * ascending); shift (S, 3) f64 is subtracted from every joint.  A HOST struct of device pointers.
 * S >= 1, n_frames_out >= 1. */
typedef struct p2r_sample_plan {
  const int *recording, *first, *variant;
  const long long *out_offset;
  const double *shift;
  long long n_frames_out;
  int S;
} p2r_sample_plan;

/* One launch for all samples.  For a joint p of a source frame, f64 throughout, never contracted:
 *   q = p - shift;  variant a > 3: swap q_x and q_z;  then (q_x, q_y, q_z) <- (q_z, q_y, -q_x) exactly a % 4 times
 * (augment_sample's two matmuls are this signed permutation; the sign of a zero is not part of the contract).
 * joints (n_frames_out, J, 3) f32 = f32(q).  votes (n_frames_out, J, 10) f32 = the vote row of p2r_vote_labels.h with
 * p = q IN F64 -- not the rounded joint -- against `boxes`, one row of the table per output sample: the sample's
 * already augmented object boxes, half = size / 2 + contact distance.  votes = NULL skips the votes (`boxes` may then be
 * NULL too).  An output frame that belongs to no sample, or whose sample names no valid source frame or variant, gets
 * zeros.  A workgroup owns 256 consecutive (frame, joint) items of the packed output and finds their samples by a
 * search of out_offset; box rows come through uniform loads; rows are staged in LDS and leave as consecutive dwords.
 * n_frames_out * J < 2^39.  P2R_EINVAL for a NULL pointer and a struct outside its limits. */
int p2r_build_samples(const p2r_recordings *rec, const p2r_sample_plan *plan, const p2r_contact_boxes *boxes,
                      float *joints, float *votes, void *stream);

/* ---- dataloader.py:108-111: np.percentile(y, 0.99) of a sample's heights, in f64 and in f32 ---- */

/* A packed store: joints (n_frames_total, J, 3) f32, frame_offset (N) i64, n_frames (N) i32 (the layout of
 * p2r_sample_store) -> floors (N, 2) f64.  With y the n = n_frames * J heights (coordinate 1) of a sample in ascending
 * order (-0.0 and +0.0 tied):
 *   column 0, every quantity f64:  v = (n - 1) * (0.99 / 100.0);  k = floor(v);  g = v - k;  a = y[k];
 *     b = y[min(k + 1, n - 1)];  d = b - a;  r = a + d * g;  if g >= 0.5: r = b - d * (1 - g)
 *   column 1, every quantity f32, widened at the end:  the same from q = 0.99f / 100.0f and v = (float)(n - 1) * q.
 * The two forms can ask for different ranks, so up to four order statistics are selected -- exactly: monotone integer
 * keys of the heights, counted into LDS histograms of 256 bins over four radix passes, one workgroup per sample.  A
 * sample with a NaN height, without frames, with more than max_frames frames or with frames outside the store gets two
 * NaN.  N >= 1, 1 <= J <= P2R_SB_MAX_J, 1 <= max_frames <= P2R_SB_MAX_FRAMES, n_frames_total >= 1 (P2R_EINVAL
 * otherwise, and for a NULL pointer). */
int p2r_floor_percentile(const float *joints, const long long *frame_offset, const int *n_frames, int n_samples, int J,
                         int max_frames, long long n_frames_total, double *floors, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* P2R_SAMPLE_BUILD_H */
