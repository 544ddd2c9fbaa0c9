/* p2r_recording_repair.h -- C ABI of libp2r_recording_repair.so: raw recordings with missing joints conditioned on the
 * device (MI355X / gfx950): which (frame, joint) items are measured, short gaps filled per joint by linear
 * interpolation in time, an optional binomial low-pass along time.
 *
 * An extension library next to libp2r_hip.so and the other extension libraries, built from
 * pose2room_amd/csrc/recording_repair.hip with the same flags (floating-point contraction off).  The other libraries
 * and their headers are unchanged by it.  Conventions are those of p2r_sample_build.h, whose p2r_recordings it takes:
 * all pointers are DEVICE pointers unless noted, tensors are contiguous row-major, `stream` is a hipStream_t (NULL =
 * default stream), every function returns P2R_OK (0), a hipError_t code, or P2R_EINVAL for arguments outside its limits
 * -- before it touches the device.  Every output element is written by every call.  No floating-point atomics (the only
 * atomics are integer counts and maxima, which do not depend on their order): two runs give identical bits.  Every loop
 * is bounded by J, the log2 of R, the words a gap search may visit (below) or the 17 taps of the widest filter.
 *
 * The reference never meets a missing joint (its poses come out of a simulator); recordings from motion capture or a
 * pose estimator drop single joints for a few frames.  pose2room_amd/net_utils/recording_repair.py's
 * `repair_reference` is the definition in NumPy, in the operation order of the kernels.
 *
 * A frame of joint j is VALID iff its three coordinates are finite.  A WORD is 64 consecutive frames of one recording:
 * recording r owns the words word_offset[r] .. word_offset[r] + ceil(n_frames[r] / 64) - 1 of n_words_total.
 * word_offset (R) i64 is made by the host.  frame_offset and word_offset ascend with r.  A recording outside the limits
 * of p2r_recordings, or whose words do not lie inside 0 .. n_words_total - 1, is one without frames.
 */
#ifndef P2R_RECORDING_REPAIR_H
#define P2R_RECORDING_REPAIR_H

#include "p2r_sample_build.h"

#ifdef __cplusplus
extern "C" {
#endif

#define P2R_RR_MAX_GAP 4096           /* the longest gap, in frames, that p2r_gap_fill can be asked to fill */
#define P2R_RR_MAX_HALF 8             /* the widest filter of p2r_smooth_frames: 2 * 8 + 1 taps */

/* bits (n_words_total, J) u64: bit i of word w of recording r = frame 64 * (w - word_offset[r]) + i of joint j is
 * valid.  Bits past the last frame of a recording, and the words of no recording, are 0.  A workgroup owns a word: its
 * 64 frames are J * 3 * 64 consecutive doubles, which arrive as consecutive loads and leave one flag each in LDS; a wave
 * then forms each (word, joint) with one ballot.  1 <= n_words_total < 2^31.
 * P2R_EINVAL for a NULL pointer, n_words_total outside its range and a `rec` outside its limits. */
int p2r_joint_valid_bits(const p2r_recordings *rec, const long long *word_offset, long long n_words_total,
                         unsigned long long *bits, void *stream);

/* out (n_frames_total, J, 3) f64 (must not alias rec->joints), how (n_frames_total, J) u8, stats (R, 4) i32.
 * For an invalid frame f of joint j in a recording of n frames, with a the nearest valid frame before f and b the
 * nearest valid frame after f (as `bits` has them):
 *   interior gap, g = b - a - 1, filled iff g <= max_gap, per coordinate in f64 and never contracted
 *       slope = (p_b - p_a) / ((double)b - (double)a);  out = slope * ((double)f - (double)a) + p_a      how = 1
 *   leading gap (no a), g = b, filled with p_b iff hold_ends and g <= max_gap                              how = 2
 *   trailing gap (no b), g = n - 1 - a, filled with p_a iff hold_ends and g <= max_gap                     how = 2
 *   anything else (a longer gap, an end with hold_ends == 0, a joint that is never valid): all three coordinates
 *   become the quiet NaN 0x7ff8000000000000, so that p2r_recording_scan still flags the recording         how = 3
 * A valid item is copied bit for bit, how = 0.  An invalid item has all three coordinates replaced, the finite ones
 * too.  A frame of no recording gets zeros and how = 0.
 * The search for a and b reads `bits`: the item's own word and at most max_gap / 64 + 1 words to either side; a
 * neighbour that far away or further makes the gap longer than max_gap whatever its place.
 * stats[r] = {invalid items, filled items, items left (how = 3), the longest run of invalid frames of any joint capped
 * at max_gap + 1 (max_gap + 1: some gap is too long)}; integer atomics.
 * A workgroup owns 256 consecutive (frame, joint) items; their coordinates come in and leave through LDS as
 * consecutive doubles.  0 <= max_gap <= P2R_RR_MAX_GAP, n_frames_total * J < 2^39.
 * P2R_EINVAL for a NULL pointer, max_gap or n_words_total outside its range and a `rec` outside its limits. */
int p2r_gap_fill(const p2r_recordings *rec, const long long *word_offset, long long n_words_total,
                 const unsigned long long *bits, int max_gap, int hold_ends, double *out, unsigned char *how,
                 int *stats, void *stream);

/* out (n_frames_total, J, 3) f64 (must not alias rec->joints): per (joint, coordinate) the track x of a recording
 * under the binomial filter of half width h = half_width, w_k = C(2h, k + h) / 4^h for k = -h .. h (exact in f64):
 *   acc = 0.0; ws = 0.0;  for k ascending over the frames f + k inside the recording:
 *   acc = acc + w_k * x[f + k];  ws = ws + w_k;  out[f] = acc / ws
 * f64, never contracted.  In the interior ws is exactly 1; at the ends the window is truncated and renormalised.
 * Values that are not finite are ordinary data.  A frame of no recording gets zeros.  A workgroup owns 112 packed
 * frames by 32 columns; the frames and a halo of 8 to either side go through LDS.
 * 1 <= half_width <= P2R_RR_MAX_HALF.  P2R_EINVAL otherwise, for a NULL pointer and a `rec` outside its limits. */
int p2r_smooth_frames(const p2r_recordings *rec, int half_width, double *out, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* P2R_RECORDING_REPAIR_H */
