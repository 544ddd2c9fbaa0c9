// occupancy.hip -- occupancy maps of predicted scenes on the device (include/p2r_occupancy.h): the voxels the nodes of a
// scene cover (bit-packed, with the owning node), the voxels the body passed through, the votes of H hypotheses and the
// volumes and overlaps of maps.
//
//   occ_boxes_kernel   the cost: N * K boxes against nz * ny * nx voxel centres, three fp64 dot products per pair.  A wave
//                      owns 64 consecutive words of one sample's map.  Lane l is voxel 64 w + l of the word at hand; one
//                      ballot forms the word; lane q keeps word q, and the wave stores its 64 words as 512 contiguous
//                      bytes.  The sample's nodes sit in LDS in chunks of OC_CHUNK, prepared once per workgroup with index
//                      bounds.  Culling has two levels, both wave-uniform: per chunk a wave ballots the nodes whose bounds
//                      meet the range of its 64 words (two 64-bit masks), and per word it walks the set bits of those
//                      masks and tests the node's bounds against the word's row and x range.  After a per-hypothesis NMS
//                      a row meets a handful of boxes, so the fp64 test runs on few (word, node) pairs.
//   occ_clear_kernel / occ_body_kernel   one thread per word / per joint; the OR is an integer atomic.
//   occ_votes_kernel   one wave per word of the fused map: lane l counts bit l over the H hypotheses.
//   occ_counts_kernel  one workgroup per sample: popcounts, reduced by shuffles and one pass over the waves' partials.
#include "p2r_common.h"

#include "../../include/p2r_occupancy.h"

namespace {

constexpr int OC_CHUNK = P2R_OCC_NODE_CHUNK;      // nodes in LDS at a time
constexpr int OC_THREADS = 256;                   // four waves
constexpr int OC_WAVES = OC_THREADS / P2R_WAVE;
constexpr int OC_WORDS = P2R_WAVE;                // words per wave
constexpr int OC_WG_WORDS = OC_WAVES * OC_WORDS;  // words per workgroup
constexpr int OC_ND = 15;                         // doubles per node: centre 3, half sizes 3, R 9
constexpr double OC_ORTHO_TOL = 1e-9;             // |R R^T - I| elementwise for the corner bounds to be trusted
static_assert(OC_CHUNK % P2R_WAVE == 0 && OC_CHUNK <= OC_THREADS, "one thread prepares one node of a chunk");
constexpr int OC_MASKS = OC_CHUNK / P2R_WAVE;

__device__ __forceinline__ bool oc_finite(double v) { return fabs(v) <= 1.7976931348623157e308; }   // false for NaN
__device__ __forceinline__ float oc_neg_inf() { return -__int_as_float(0x7f800000); }

// floor / ceil of a double as an index clamped into [-1, n]: NaN and values outside int never reach the cast
__device__ __forceinline__ int oc_index_lo(double v, int n) {       // conservative below: NaN -> -1
  if (!(v >= 0.0)) return -1;
  if (v >= (double)n) return n;
  return (int)floor(v);
}
__device__ __forceinline__ int oc_index_hi(double v, int n) {       // conservative above: NaN -> n
  if (!(v < (double)n)) return n;
  if (v < 0.0) return -1;
  return (int)ceil(v);
}

struct OcGrid {
  double o[3];
  double voxel;
  int n[3];       // nx, ny, nz
  int W;
};

// Node `slot` of sample n into LDS slot `c` of the chunk: parameters and index bounds; lo > hi for a node that covers
// nothing (not counted, or a non-finite parameter).
__device__ __forceinline__ void oc_prepare(int c, bool counted, const double *__restrict__ obb,
                                           const double *__restrict__ rmat, float score, const OcGrid &g,
                                           double (*s_d)[OC_CHUNK], int (*s_b)[OC_CHUNK], float *s_sc) {
  int lo[3] = {1, 1, 1}, hi[3] = {0, 0, 0};
  double p[OC_ND];
#pragma unroll
  for (int a = 0; a < OC_ND; ++a) p[a] = 0.0;
  if (counted) {
    bool ok = oc_finite(obb[6]);
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      p[a] = obb[a];
      p[3 + a] = obb[3 + a] / 2.0;
      ok = ok && oc_finite(obb[a]) && oc_finite(obb[3 + a]);
    }
#pragma unroll
    for (int a = 0; a < 9; ++a) {
      p[6 + a] = rmat[a];
      ok = ok && oc_finite(rmat[a]);
    }
    if (ok) {
      const double *R = p + 6;
      bool ortho = true;
#pragma unroll
      for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = a; b < 3; ++b) {
          const double dot = (R[a * 3] * R[b * 3] + R[a * 3 + 1] * R[b * 3 + 1]) + R[a * 3 + 2] * R[b * 3 + 2];
          ortho = ortho && fabs(dot - (a == b ? 1.0 : 0.0)) <= OC_ORTHO_TOL;       // NaN (an overflow): false
        }
      const double h0 = fabs(p[3]), h1 = fabs(p[4]), h2 = fabs(p[5]);
      const double hmax = fmax(h0, fmax(h1, h2));
      const double cmax = fmax(fabs(p[0]), fmax(fabs(p[1]), fabs(p[2])));
      // one voxel, and what a matrix orthonormal only to OC_ORTHO_TOL and the rounding of the corners can move a face
      const double slack = (g.voxel + 1e-8 * hmax) + 1e-12 * cmax;
#pragma unroll
      for (int x = 0; x < 3; ++x) {
        if (ortho) {
          // the extreme of the eight corners along world axis x: centre -+ sum_a |h_a R[a][x]|
          const double ext = ((h0 * fabs(R[x]) + h1 * fabs(R[3 + x])) + h2 * fabs(R[6 + x])) + slack;
          lo[x] = oc_index_lo(((p[x] - ext) - g.o[x]) / g.voxel - 0.5, g.n[x]);
          hi[x] = oc_index_hi(((p[x] + ext) - g.o[x]) / g.voxel - 0.5, g.n[x]);
          lo[x] = lo[x] < 0 ? 0 : lo[x];
          hi[x] = hi[x] > g.n[x] - 1 ? g.n[x] - 1 : hi[x];
        } else {
          lo[x] = 0, hi[x] = g.n[x] - 1;
        }
      }
    }
  }
#pragma unroll
  for (int a = 0; a < OC_ND; ++a) s_d[a][c] = p[a];
#pragma unroll
  for (int x = 0; x < 3; ++x) s_b[x][c] = lo[x], s_b[3 + x][c] = hi[x];
  s_sc[c] = score != score ? oc_neg_inf() : score;
}

__global__ __launch_bounds__(OC_THREADS) void occ_boxes_kernel(int K, int wgs, const int *__restrict__ count,
                                                               const double *__restrict__ node_obbs,
                                                               const double *__restrict__ node_rmat,
                                                               const float *__restrict__ node_score, OcGrid g,
                                                               long long *__restrict__ occ, short *owner) {
  __shared__ double s_d[OC_ND][OC_CHUNK];
  __shared__ int s_b[6][OC_CHUNK];
  __shared__ float s_sc[OC_CHUNK];
  const int tid = threadIdx.x, lane = tid & (P2R_WAVE - 1), wave = tid / P2R_WAVE;
  const int n = blockIdx.x / wgs, wg = blockIdx.x - n * wgs;
  const int nx = g.n[0], ny = g.n[1], W = g.W;
  const int words = g.n[2] * ny * W;                           // <= 2^24
  const int q0 = wg * OC_WG_WORDS + wave * OC_WORDS;           // this wave's first word; may lie past the map
  const int nq = words - q0 < OC_WORDS ? words - q0 : OC_WORDS;   // <= 0: a wave without words (it still prepares nodes)
  int cnt = count[n];
  cnt = cnt < 0 ? 0 : (cnt > K ? K : cnt);

  // the range of the wave's words: rows r0 .. r1 of the map (row = k * ny + j)
  int j_lo = 0, j_hi = -1, k_lo = 0, k_hi = -1, i_lo = 0, i_hi = -1;
  if (nq > 0) {
    const int r0 = q0 / W, r1 = (q0 + nq - 1) / W;
    k_lo = r0 / ny, k_hi = r1 / ny;
    j_lo = k_lo == k_hi ? r0 - k_lo * ny : 0;
    j_hi = k_lo == k_hi ? r1 - k_hi * ny : ny - 1;
    i_lo = r0 == r1 ? (q0 - r0 * W) * 64 : 0;
    i_hi = r0 == r1 ? (q0 + nq - 1 - r0 * W) * 64 + 63 : nx - 1;
  }

  unsigned long long myword = 0ull;                            // word q0 + lane
  const long long node0 = (long long)n * K;
  for (int c0 = 0; c0 < cnt; c0 += OC_CHUNK) {                 // cnt is uniform over the workgroup
    const int nc = cnt - c0 < OC_CHUNK ? cnt - c0 : OC_CHUNK;
    if (c0 > 0) __syncthreads();                               // the previous chunk has been read by every wave
    if (tid < OC_CHUNK) {
      const int s = c0 + tid;
      const bool counted = tid < nc;
      const long long o = node0 + (counted ? s : 0);
      oc_prepare(tid, counted, node_obbs + o * 7, node_rmat + o * 9, counted ? node_score[o] : 0.0f, g, s_d, s_b, s_sc);
    }
    __syncthreads();
    if (nq <= 0) continue;

    // level 1: the nodes of the chunk whose bounds meet the wave's range
    unsigned long long mask[OC_MASKS];
#pragma unroll
    for (int m = 0; m < OC_MASKS; ++m) {
      const int c = m * P2R_WAVE + lane;
      const bool hit = s_b[0][c] <= i_hi && s_b[3][c] >= i_lo && s_b[1][c] <= j_hi && s_b[4][c] >= j_lo &&
                       s_b[2][c] <= k_hi && s_b[5][c] >= k_lo && s_b[0][c] <= s_b[3][c];
      mask[m] = __ballot(hit);
    }
    bool any = false;
#pragma unroll
    for (int m = 0; m < OC_MASKS; ++m) any = any || mask[m] != 0ull;
    if (!any && (owner == nullptr || c0 > 0)) continue;        // nothing to OR; the owner map holds a value already

    for (int qi = 0; qi < nq; ++qi) {
      const int q = q0 + qi;
      const int r = q / W, w = q - r * W;
      const int k = r / ny, j = r - k * ny;
      const int i = w * 64 + lane;
      const double px = g.o[0] + ((double)i + 0.5) * g.voxel;
      const double py = g.o[1] + ((double)j + 0.5) * g.voxel;
      const double pz = g.o[2] + ((double)k + 0.5) * g.voxel;
      bool covered = false;
      int best = -1;
      float best_sc = 0.0f;
#pragma unroll
      for (int m = 0; m < OC_MASKS; ++m) {
        unsigned long long rest = mask[m];
        while (rest) {                                         // ascending slots: at most 64 turns per mask
          const int c = m * P2R_WAVE + __builtin_ctzll(rest);
          rest &= rest - 1ull;
          // level 2: this word's row and x range
          if (s_b[1][c] > j || s_b[4][c] < j || s_b[2][c] > k || s_b[5][c] < k || s_b[0][c] > w * 64 + 63 ||
              s_b[3][c] < w * 64)
            continue;
          const double d0 = px - s_d[0][c], d1 = py - s_d[1][c], d2 = pz - s_d[2][c];
          bool in = i < nx;
#pragma unroll
          for (int a = 0; a < 3; ++a) {
            const double gap =
                fabs((d0 * s_d[6 + a * 3][c] + d1 * s_d[7 + a * 3][c]) + d2 * s_d[8 + a * 3][c]) - s_d[3 + a][c];
            in = in && gap <= 0.0;
          }
          if (in) {
            const float sc = s_sc[c];
            if (!covered || sc > best_sc) best = c0 + c, best_sc = sc;      // strictly higher: a tie stays with the lower slot
            covered = true;
          }
        }
      }
      const unsigned long long bits = __ballot(covered);
      if (lane == qi) myword |= bits;
      if (owner != nullptr && i < nx) {
        short *dst = owner + ((long long)n * g.n[2] * ny + r) * nx + i;
        if (c0 == 0) {
          *dst = (short)best;
        } else if (covered) {
          // a later chunk: this lane wrote *dst itself while it held the chunks before.  The earlier owner has the lower
          // slot, so it stays unless the newcomer's score is strictly higher.
          const int prev = *dst;
          bool take = prev < 0;
          if (!take) {
            const float ps = node_score[node0 + prev];
            take = best_sc > (ps != ps ? oc_neg_inf() : ps);
          }
          if (take) *dst = (short)best;
        }
      }
    }
  }

  if (cnt == 0 && owner != nullptr) {                          // no chunk ran: the owner map is all free
    for (int qi = 0; qi < nq; ++qi) {
      const int q = q0 + qi;
      const int r = q / W, w = q - r * W;
      const int i = w * 64 + lane;
      if (i < nx) owner[((long long)n * g.n[2] * ny + r) * nx + i] = (short)-1;
    }
  }
  if (lane < nq) occ[(long long)n * words + q0 + lane] = (long long)myword;
}

__global__ __launch_bounds__(OC_THREADS) void occ_clear_kernel(long long total, long long *__restrict__ dst) {
  const long long e = (long long)blockIdx.x * OC_THREADS + threadIdx.x;
  if (e < total) dst[e] = 0ll;
}

__global__ __launch_bounds__(OC_THREADS) void occ_body_kernel(const float *__restrict__ joints, int TJ, int C,
                                                              long long total, OcGrid g,
                                                              unsigned long long *__restrict__ body) {
  const long long e = (long long)blockIdx.x * OC_THREADS + threadIdx.x;       // (b, t, j)
  if (e >= total) return;
  const float *x = joints + e * C;
  int idx[3];
  bool ok = true;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const double v = floor(((double)x[a] - g.o[a]) / g.voxel);
    ok = ok && v >= 0.0 && v < (double)g.n[a];                 // false for NaN and +-inf; inside int before the cast
    idx[a] = ok ? (int)v : 0;
  }
  if (!ok) return;
  const long long b = e / TJ;
  const long long word = ((b * g.n[2] + idx[2]) * g.n[1] + idx[1]) * g.W + (idx[0] >> 6);
  atomicOr(body + word, 1ull << (idx[0] & 63));
}

// one wave per word of the fused map; `total` = B * words
__global__ __launch_bounds__(OC_THREADS) void occ_votes_kernel(int H, long long total, int nx, int W,
                                                               const unsigned long long *__restrict__ occ,
                                                               int min_votes, unsigned char *__restrict__ votes,
                                                               long long *__restrict__ fused) {
  const int lane = threadIdx.x & (P2R_WAVE - 1);
  const long long q = (long long)blockIdx.x * OC_WAVES + threadIdx.x / P2R_WAVE;   // b * words + word
  if (q >= total) return;                                                           // uniform over the wave
  const long long row = q / W;
  const int i = (int)(q - row * W) * 64 + lane;
  int v = 0;
  for (int h = 0; h < H; ++h) v += (int)((occ[(long long)h * total + q] >> lane) & 1ull);
  if (i >= nx) v = 0;                                          // padding bits of the input are ignored
  const unsigned long long bits = __ballot(v >= min_votes);
  if (lane == 0) fused[q] = (long long)bits;
  if (votes != nullptr && i < nx) votes[row * nx + i] = (unsigned char)v;
}

__global__ __launch_bounds__(OC_THREADS) void occ_counts_kernel(int B, long long words,
                                                                const unsigned long long *__restrict__ a,
                                                                const unsigned long long *__restrict__ gt,
                                                                const unsigned long long *__restrict__ body,
                                                                long long *__restrict__ counts) {
  __shared__ long long s_part[OC_WAVES][5];
  const int tid = threadIdx.x, lane = tid & (P2R_WAVE - 1), wave = tid / P2R_WAVE;
  const long long n = blockIdx.x, b = n % B;
  const unsigned long long *pa = a + n * words;
  const unsigned long long *pg = gt ? gt + b * words : nullptr, *pb = body ? body + b * words : nullptr;
  long long acc[5] = {0, 0, 0, 0, 0};
  for (long long q = tid; q < words; q += OC_THREADS) {
    const unsigned long long x = pa[q], y = pg ? pg[q] : 0ull, z = pb ? pb[q] : 0ull;
    acc[0] += __popcll(x);
    acc[1] += __popcll(y);
    acc[2] += __popcll(x & y);
    acc[3] += __popcll(z);
    acc[4] += __popcll(x & z);
  }
#pragma unroll
  for (int f = 0; f < 5; ++f) {
#pragma unroll
    for (int m = P2R_WAVE / 2; m >= 1; m >>= 1) acc[f] += __shfl_xor(acc[f], m);
    if (lane == 0) s_part[wave][f] = acc[f];
  }
  __syncthreads();
  if (tid < 5) {
    long long sum = 0;
    for (int w = 0; w < OC_WAVES; ++w) sum += s_part[w][tid];
    counts[n * 5 + tid] = sum;
  }
}

constexpr long long OC_MAX_ELEMS = 0x7fffffffLL;

bool grid_ok(double ox, double oy, double oz, double voxel, int nx, int ny, int nz) {
  const double lim = 1.7976931348623157e308;
  if (!(nx >= 1 && nx <= P2R_OCC_MAX_DIM && ny >= 1 && ny <= P2R_OCC_MAX_DIM && nz >= 1 && nz <= P2R_OCC_MAX_DIM))
    return false;
  if (!(voxel > 0.0 && voxel <= lim)) return false;
  return __builtin_fabs(ox) <= lim && __builtin_fabs(oy) <= lim && __builtin_fabs(oz) <= lim;
}

OcGrid make_grid(double ox, double oy, double oz, double voxel, int nx, int ny, int nz) {
  OcGrid g;
  g.o[0] = ox, g.o[1] = oy, g.o[2] = oz;
  g.voxel = voxel;
  g.n[0] = nx, g.n[1] = ny, g.n[2] = nz;
  g.W = (nx + 63) / 64;
  return g;
}

long long map_words(int nx, int ny, int nz) { return (long long)nz * ny * ((nx + 63) / 64); }

}  // namespace

extern "C" int p2r_occ_boxes(int N, int K, const int *count, const double *node_obbs, const double *node_rmat,
                             const float *node_score, double ox, double oy, double oz, double voxel, int nx, int ny,
                             int nz, long long *occ, short *owner, void *stream) {
  if (N < 0 || K < 0 || K > P2R_OCC_MAX_K || !grid_ok(ox, oy, oz, voxel, nx, ny, nz)) return P2R_EINVAL;
  const long long words = map_words(nx, ny, nz);
  if ((long long)N * words > OC_MAX_ELEMS || (long long)N * K > OC_MAX_ELEMS) return P2R_EINVAL;
  if (N == 0) return P2R_OK;
  if (!count || !occ) return P2R_EINVAL;
  if (K > 0 && (!node_obbs || !node_rmat || !node_score)) return P2R_EINVAL;
  const int wgs = (int)((words + OC_WG_WORDS - 1) / OC_WG_WORDS);
  hipLaunchKernelGGL(occ_boxes_kernel, dim3((unsigned)((long long)N * wgs)), dim3(OC_THREADS), 0, p2r_stream(stream), K,
                     wgs, count, node_obbs, node_rmat, node_score, make_grid(ox, oy, oz, voxel, nx, ny, nz), occ, owner);
  P2R_LAUNCH_CHECK();
  return P2R_OK;
}

extern "C" int p2r_occ_body(const float *joints, int B, int T, int J, int C, double ox, double oy, double oz,
                            double voxel, int nx, int ny, int nz, long long *body, void *stream) {
  if (B < 0 || T < 0 || J < 0 || (C != 3 && C != 4) || !grid_ok(ox, oy, oz, voxel, nx, ny, nz)) return P2R_EINVAL;
  const long long words = map_words(nx, ny, nz);
  const long long tj = (long long)T * J;                       // factors below 2^31: a product of two fits int64
  if ((long long)B * words > OC_MAX_ELEMS || tj > OC_MAX_ELEMS || (long long)B * tj > OC_MAX_ELEMS) return P2R_EINVAL;
  const long long total = (long long)B * tj;
  if (B == 0) return P2R_OK;
  if (!body || (total > 0 && !joints)) return P2R_EINVAL;
  const long long cells = (long long)B * words;
  hipLaunchKernelGGL(occ_clear_kernel, dim3((unsigned)((cells + OC_THREADS - 1) / OC_THREADS)), dim3(OC_THREADS), 0,
                     p2r_stream(stream), cells, body);
  P2R_LAUNCH_CHECK();
  if (total > 0) {
    hipLaunchKernelGGL(occ_body_kernel, dim3((unsigned)((total + OC_THREADS - 1) / OC_THREADS)), dim3(OC_THREADS), 0,
                       p2r_stream(stream), joints, T * J, C, total, make_grid(ox, oy, oz, voxel, nx, ny, nz),
                       reinterpret_cast<unsigned long long *>(body));
    P2R_LAUNCH_CHECK();
  }
  return P2R_OK;
}

extern "C" int p2r_occ_votes(int H, int B, int nx, int ny, int nz, const long long *occ, int min_votes,
                             unsigned char *votes, long long *fused, void *stream) {
  if (H < 1 || H > P2R_OCC_MAX_H || B < 0 || min_votes < 1 || min_votes > H) return P2R_EINVAL;
  if (!grid_ok(0.0, 0.0, 0.0, 1.0, nx, ny, nz)) return P2R_EINVAL;
  const long long words = map_words(nx, ny, nz);
  if ((long long)H * B * words > OC_MAX_ELEMS) return P2R_EINVAL;
  if (B == 0) return P2R_OK;
  if (!occ || !fused) return P2R_EINVAL;
  const long long total = (long long)B * words;
  hipLaunchKernelGGL(occ_votes_kernel, dim3((unsigned)((total + OC_WAVES - 1) / OC_WAVES)), dim3(OC_THREADS), 0,
                     p2r_stream(stream), H, total, nx, (nx + 63) / 64, reinterpret_cast<const unsigned long long *>(occ),
                     min_votes, votes, fused);
  P2R_LAUNCH_CHECK();
  return P2R_OK;
}

extern "C" int p2r_occ_counts(int N, int B, unsigned long long words, const long long *a, const long long *gt,
                              const long long *body, long long *counts, void *stream) {
  if (N < 0 || B < 0 || words > (1ull << 24)) return P2R_EINVAL;
  if (N > 0 && (B < 1 || N % B != 0)) return P2R_EINVAL;
  if ((long long)N * (long long)words > OC_MAX_ELEMS) return P2R_EINVAL;
  if (N == 0) return P2R_OK;
  if (!counts || (words > 0 && !a)) return P2R_EINVAL;
  hipLaunchKernelGGL(occ_counts_kernel, dim3((unsigned)N), dim3(OC_THREADS), 0, p2r_stream(stream), B, (long long)words,
                     reinterpret_cast<const unsigned long long *>(a), reinterpret_cast<const unsigned long long *>(gt),
                     reinterpret_cast<const unsigned long long *>(body), counts);
  P2R_LAUNCH_CHECK();
  return P2R_OK;
}
