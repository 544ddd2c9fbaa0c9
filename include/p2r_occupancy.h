/* p2r_occupancy.h -- C ABI of libp2r_occupancy.so: occupancy maps of predicted scenes on the device (MI355X / gfx950).
 *
 * An extension library next to libp2r_hip.so and its sisters, built from pose2room_amd/csrc/occupancy.hip with the same
 * flags (floating-point contraction off).  The other libraries and their headers are unchanged by it.  Conventions are
 * those of p2r_consensus.h: all pointers are DEVICE pointers, tensors are contiguous row-major, `stream` is a hipStream_t
 * (NULL = default stream), every function returns P2R_OK (0), a hipError_t code, or P2R_EINVAL for arguments outside its
 * limits -- before it touches the device.  A problem without an output element returns 0 and launches nothing.  Every
 * output element is written by every call.  No floating-point atomics (the one atomic is an integer OR, whose result
 * does not depend on order): two runs give identical bits.  No call synchronises, and no workgroup waits for another.
 * Every loop is bounded by the arguments.  The C side never allocates.
 *
 * Element counts are `unsigned long long` where C would say size_t: the binding is derived from this header by a parser
 * that maps no size_t, and on the LP64 hosts this library is built for the two are the same 64-bit type.
 *
 * GRID.  origin (ox, oy, oz), voxel > 0 and (nx, ny, nz).  The centre of voxel (i, j, k) is, per axis,
 * origin + ((double)index + 0.5) * voxel.  Dense tensors are (.., nz, ny, nx), x fastest.  Bit-packed tensors are
 * (.., nz, ny, W) 64-bit words, W = ceil(nx / 64): bit i % 64 of word i / 64 is voxel i; the padding bits of the last
 * word of a row are zero.  `words` below is nz * ny * W, the words of one map.
 */
#ifndef P2R_OCCUPANCY_H
#define P2R_OCCUPANCY_H

#include "p2r_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define P2R_OCC_MAX_DIM 1024          /* nx, ny, nz */
#define P2R_OCC_MAX_K 1024            /* node slots per sample (P2R_SCENE_MAX_K) */
#define P2R_OCC_MAX_H 64              /* hypotheses: votes fit a byte */
#define P2R_OCC_NODE_CHUNK 128        /* nodes of a sample held in LDS at a time by p2r_occ_boxes */

/* The voxels that the nodes of N samples cover.  Inputs as p2r_scene_nodes writes them: count (N) i32, node_obbs
 * (N,K,7) f64 centre, size, heading, node_rmat (N,K,3,3) f64, node_score (N,K) f32.
 * Slot s of sample n counts iff s < min(max(count[n], 0), K).  Node s covers a point p iff, with d = p - centre,
 *   fabs((d0 * R[a][0] + d1 * R[a][1]) + d2 * R[a][2]) - size[a] / 2.0 <= 0     for a = 0, 1, 2
 * (the expression of p2r_contact_frames; the boundary is inclusive).  A node with a non-finite value among its 7 box
 * parameters or its 9 matrix entries covers nothing.  A voxel is occupied iff a counted node covers its centre; its owner
 * is the covering node that precedes the others: higher f32 score first, a NaN score as -inf, ties to the lower slot.
 * Outputs: occ (N,nz,ny,W) i64 bit-packed; owner (N,nz,ny,nx) i16 the owner's slot, -1 for a free voxel -- NULL: skipped.
 *
 * One launch.  A wave owns 64 consecutive words of a sample's map: it forms each word with one ballot over the 64 voxels
 * of the word, keeps word l in lane l and stores the 64 words as 512 contiguous bytes.  The nodes sit in LDS in chunks of
 * P2R_OCC_NODE_CHUNK, each prepared once per workgroup (centre, half sizes, R, index bounds).  The bounds are those of
 * the eight corners in fp64, widened by one voxel and a relative slack, of a node whose R is orthonormal to 1e-9; any
 * other node has the whole grid as its bounds.  They never drop a node that the test above accepts.  A wave skips,
 * wave-uniformly, first the nodes whose bounds miss all its 64 words and then those that miss the word at hand. */
int p2r_occ_boxes(int N, int K, const int *count, const double *node_obbs, const double *node_rmat,
                  const float *node_score, double ox, double oy, double oz, double voxel, int nx, int ny, int nz,
                  long long *occ, short *owner, void *stream);

/* The voxels the joints of B recordings fall into.  joints (B,T,J,C) f32, C = 3 or 4 (x, y, z first).  A joint marks
 * voxel index_a = floor(((double)x_a - origin_a) / voxel) when all three indices are inside the grid; a joint with a
 * non-finite coordinate or an index outside marks nothing.  body (B,nz,ny,W) i64 bit-packed, cleared and filled by this
 * call: two launches (clear; one thread per joint, integer atomicOr). */
int p2r_occ_body(const float *joints, int B, int T, int J, int C, double ox, double oy, double oz, double voxel, int nx,
                 int ny, int nz, long long *body, void *stream);

/* Votes of H hypotheses.  occ (H * B,nz,ny,W) i64, hypothesis-major (n = h * B + b).  votes (B,nz,ny,nx) u8 = the number
 * of hypotheses whose bit is set -- NULL: skipped; fused (B,nz,ny,W) i64 has the bit iff votes >= min_votes.  Padding
 * bits of occ are ignored and written as zero.  One launch, one wave per word. */
int p2r_occ_votes(int H, int B, int nx, int ny, int nz, const long long *occ, int min_votes, unsigned char *votes,
                  long long *fused, void *stream);

/* Volumes and overlaps.  a (N,words) i64; gt (B,words) i64 or NULL; body (B,words) i64 or NULL; sample n reads row n % B.
 * counts (N,5) i64 = vol = popcount(a[n]), vol_gt = popcount(gt), inter_gt = popcount(a & gt), vol_body = popcount(body),
 * inter_body = popcount(a & body); the columns of a NULL map are 0.  One launch, one workgroup per sample, integer sums
 * reduced in a fixed order. */
int p2r_occ_counts(int N, int B, unsigned long long words, const long long *a, const long long *gt,
                   const long long *body, long long *counts, void *stream);

/* Limits -- P2R_EINVAL otherwise: 1 <= nx, ny, nz <= P2R_OCC_MAX_DIM; 0 <= K <= P2R_OCC_MAX_K; 1 <= H <= P2R_OCC_MAX_H;
 * 1 <= min_votes <= H; N, B >= 0; T, J >= 0 and C in {3, 4}; B >= 1 and N % B == 0 in p2r_occ_counts when N > 0, and
 * words <= 2^24 there (P2R_OCC_MAX_DIM^2 * 16); voxel finite and > 0; the origin finite; N * words (B * words; H * B * words)
 * at most 2^31 - 1 and B * T * J at most 2^31 - 1, so that every element count fits int64 and every grid its launch
 * dimension; a NULL pointer to a tensor that has elements, other than the optional ones named above.
 * N = 0 or B = 0 launches nothing; K = 0 writes an empty map. */

#ifdef __cplusplus
}
#endif
#endif /* P2R_OCCUPANCY_H */
