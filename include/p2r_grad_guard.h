/* p2r_grad_guard.h -- C ABI of libp2r_grad_guard.so: the gradients of one train step measured and clipped on the
 * device (MI355X / gfx950).
 *
 * An extension library next to libp2r_hip.so and its sisters, built from pose2room_amd/csrc/grad_guard.hip with the same
 * flags (floating-point contraction off).  The other libraries and their headers are unchanged by it.  Conventions are
 * those of p2r_hip.h: `stream` is a hipStream_t (NULL = default stream), every function returns P2R_OK (0), a hipError_t
 * code, or P2R_EINVAL for arguments outside its limits -- before it touches the device.  Every output element is written
 * by every call.  No floating-point atomics and no atomics at all: two runs give identical bits.  No call synchronises.
 *
 * The gradients come as a HOST table of p2r_grad_entry.  The table is read during the call and travels to the device by
 * value, inside the kernel arguments of the launches it describes (groups of P2R_GG_GROUP entries): nothing is staged in
 * memory that a later call could overwrite, so two calls may be enqueued back to back with other tables, and the table
 * may be freed or rewritten as soon as the call returns.
 *
 * What is computed, with e the elements of gradient i and every quantity float64 unless noted:
 *   S_i   = sum over the FINITE e of (double)e * (double)e          c_i = number of e that are +inf, -inf or NaN (i32)
 *   norm  = sqrt(S_0 + S_1 + ... ), added in table order              found = sum_i c_i > 0 ? 1.0f : 0.0f
 *   scale = max_norm > 0 ? (float)max(1.0, (norm + 1e-6) / max_norm) : 1.0f
 * `scale` is a DIVISOR: the clipped gradient is g / scale, which is torch's clip_grad_norm_ coefficient
 * clamp(max_norm / (norm + 1e-6), max = 1) written the other way round.
 *
 * The order of every sum is fixed by the (numel, dtype) of the entries alone.  A gradient is cut into chunks of
 * P2R_GG_CHUNK elements.  Inside a chunk, element j belongs to 16-byte group j / v (v = 4 for f32, 2 for f64), group m
 * to thread m % 256 and to that thread's accumulator j % v; a thread adds its groups in ascending order, then its
 * accumulators in ascending order; the 256 threads are combined by a xor butterfly over the 64 lanes of a wave and the
 * four waves in ascending order.  The chunks of a gradient are added in ascending order, the gradients in table order.
 * Neither an address nor the timing of a launch enters.
 */
#ifndef P2R_GRAD_GUARD_H
#define P2R_GRAD_GUARD_H

#include "p2r_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define P2R_GG_F32 0                  /* p2r_grad_entry.dtype */
#define P2R_GG_F64 1
#define P2R_GG_CHUNK 16384            /* elements per chunk: one workgroup, one (sum, count) partial */
#define P2R_GG_GROUP 160              /* table entries that travel in the arguments of one launch */

/* One gradient: `data` a DEVICE pointer to numel contiguous elements, aligned to its element size (any element offset
 * inside an allocation is fine).  An absent gradient keeps its slot as data = NULL, numel = 0. */
typedef struct p2r_grad_entry {
  const void *data;
  long long numel;
  int dtype;
} p2r_grad_entry;

/* Entry i owns max(1, ceil(numel_i / P2R_GG_CHUNK)) chunks; n_chunks must be their sum (the caller sizes the partial
 * buffers by it, so it is checked).
 * Work buffers, written completely: part_sumsq (n_chunks) f64, part_count (n_chunks) i32, first_chunk (n) i32.
 * Outputs: sumsq (n) f64 = S_i, nonfinite (n) i32 = c_i, norm (1) f64, scale (1) f32, found (1) f32.
 * Counters, read and written: steps (1) i64 += 1; skipped (1) i64 += 1 iff found and count_skips != 0.
 * Launches: one streaming pass per group of P2R_GG_GROUP entries -- one workgroup per chunk, 16 bytes per lane and load,
 * a dword-aligned 16-byte load where the gradient does not start on a 16-byte boundary, single elements behind the last
 * whole group of a gradient -- then one workgroup that adds the partials.  n = 0 runs the second launch alone (norm = 0,
 * found = 0).  The gradients are not modified.
 * P2R_EINVAL: n < 0, table = NULL with n > 0, a NULL output, counter or work buffer that has elements, numel < 0, a
 * dtype other than the two above, data = NULL with numel > 0, data not aligned to its element size, a wrong n_chunks,
 * a sum of chunks that does not fit int, max_norm NaN. */
int p2r_grad_measure(const p2r_grad_entry *table, int n, double max_norm, int count_skips, int n_chunks,
                     double *part_sumsq, int *part_count, int *first_chunk, double *sumsq, int *nonfinite,
                     double *norm, float *scale, float *found, long long *steps, long long *skipped, void *stream);

/* g = g / scale in place for every element of every entry, in the gradient's own precision: (float)g / scale for f32,
 * g / (double)scale for f64.  `scale` (1) f32 is read on the device; every workgroup returns at once when it is 1.
 * For optimisers that cannot take the divisor themselves.  One launch per group of P2R_GG_GROUP entries, one workgroup
 * per chunk; a table without elements launches nothing.  P2R_EINVAL as above, and for scale = NULL. */
int p2r_grad_scale(const p2r_grad_entry *table, int n, const float *scale, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* P2R_GRAD_GUARD_H */
