// scene.hip -- the scene read-out of a batch on the device (include/p2r_scene.h): what the reference's demo.py does on
// the host per sample and per object (visualize_step, Vis_Demo's dist_node2bbox, np.unique over the frames).
//
//   p2r_scene_nodes     one workgroup per sample; the keep test of every proposal, a ballot per wave and a prefix over the
//                       four waves give each kept proposal its slot, in ascending proposal index.  A few hundred bytes
//                       of plain stores per proposal: bound by launch latency, not by anything on the card.
//   p2r_contact_frames  the only real work: N * K * T * J box-distance evaluations in fp64 (about 33 VALU operations
//                       each).  A node needs every joint of its sample, T * J * 3 floats (651 KB at T = 1024, J = 53),
//                       far more than LDS.  One workgroup owns CF_NODES = 4 consecutive slots of a sample, one per wave;
//                       the frames pass through LDS in chunks of CF_CH = 64, copied with coalesced loads, and lane l of
//                       every wave walks the joints of frame l of the chunk.  The LDS row stride is odd, so the 64
//                       lanes of a read hit 64 different banks.  The maximum over joints is then a serial maximum in one
//                       lane and the minimum over frames one running (value, frame) pair per lane: the only cross-lane
//                       step is one fixed-order reduction at the end.  Four nodes per workgroup because the kept
//                       proposals are compacted (slots 0 .. count-1): the joints of a sample are fetched count / 4
//                       times instead of count times, and a workgroup whose four slots are all empty returns at once.
//   p2r_unique_frames   one workgroup of 1024 threads per sample.  (1) a wave per frame reads the row coalesced and
//                       reduces a commutative 32-bit hash (-0 mapped to +0; a NaN marks the row as equal to none);
//                       (2) thread t scans the hashes of the frames before it -- all lanes read the same LDS word, a
//                       broadcast -- and confirms an equal hash by comparing the two rows in memory; (3) the first
//                       occurrences are compacted by ballots, chunk by chunk; (4) rank[t] = slot of first[t].
//                       LDS: three int tables of T entries, hence T <= 4096.
#include "p2r_common.h"

#include "../../include/p2r_scene.h"

namespace {

constexpr int SN_THREADS = 256;
constexpr int CF_THREADS = 256;
constexpr int CF_NODES = CF_THREADS / P2R_WAVE;      // slots per workgroup, one per wave
constexpr int CF_CH = P2R_WAVE;                      // frames per chunk, one per lane
constexpr int CF_LD = 16;                            // loads a thread has in flight while a chunk is copied
constexpr int UF_THREADS = 1024;

// Slot of this thread's element among the flagged elements of the workgroup, in thread order, behind the `running`
// elements flagged so far; `running` moves on by the workgroup's total.  lds_w: one int per wave.  Two barriers; every
// thread of the workgroup must call it.
template <int WAVES>
__device__ __forceinline__ int compact_slot(bool flag, int &running, int *lds_w) {
  const int lane = threadIdx.x & (P2R_WAVE - 1), wave = threadIdx.x / P2R_WAVE;
  const unsigned long long b = __ballot(flag);
  if (lane == 0) lds_w[wave] = __popcll(b);
  __syncthreads();
  int before = 0, total = 0;
#pragma unroll
  for (int w = 0; w < WAVES; ++w) {
    const int c = lds_w[w];
    before += w < wave ? c : 0;
    total += c;
  }
  const int slot = running + before + __popcll(b & ((1ull << lane) - 1ull));
  running += total;
  __syncthreads();
  return slot;
}

__global__ __launch_bounds__(SN_THREADS) void scene_nodes_kernel(
    int K, const double *__restrict__ obbs, const float *__restrict__ obj_prob,
    const unsigned char *__restrict__ pred_mask, const long long *__restrict__ pred_cls, double dump_threshold,
    int *__restrict__ count, int *__restrict__ inst_idx, double *__restrict__ node_obbs, double *__restrict__ node_rmat,
    long long *__restrict__ node_cls, float *__restrict__ node_score) {
  __shared__ int lds_w[SN_THREADS / P2R_WAVE];
  const int tid = threadIdx.x;
  const long long row = (long long)blockIdx.x * K;
  int running = 0;
  for (int k0 = 0; k0 < K; k0 += SN_THREADS) {
    const int k = k0 + tid;
    float prob = 0.0f;
    bool keep = false;
    if (k < K) {
      prob = obj_prob[row + k];
      keep = (double)prob > dump_threshold && pred_mask[row + k] == 1;
    }
    const int slot = compact_slot<SN_THREADS / P2R_WAVE>(keep, running, lds_w);
    if (keep) {
      const long long o = row + slot;
      double h = 0.0;
#pragma unroll
      for (int a = 0; a < 7; ++a) node_obbs[o * 7 + a] = h = obbs[(row + k) * 7 + a];
      const double c = cos(h), s = sin(h);
      double *R = node_rmat + o * 9;
      R[0] = c, R[1] = 0.0, R[2] = -s, R[3] = 0.0, R[4] = 1.0, R[5] = 0.0, R[6] = s, R[7] = 0.0, R[8] = c;
      inst_idx[o] = k;
      node_cls[o] = pred_cls[row + k];
      node_score[o] = prob;
    }
  }
  for (int s = running + tid; s < K; s += SN_THREADS) {
    const long long o = row + s;
#pragma unroll
    for (int a = 0; a < 7; ++a) node_obbs[o * 7 + a] = 0.0;
#pragma unroll
    for (int a = 0; a < 9; ++a) node_rmat[o * 9 + a] = 0.0;
    inst_idx[o] = -1;
    node_cls[o] = 0;
    node_score[o] = 0.0f;
  }
  if (tid == 0) count[blockIdx.x] = running;
}

// (d, t) of the other lane wins when it is smaller, or equal and earlier
__device__ __forceinline__ void take_min(double &d, int &t, double od, int ot) {
  if (od < d || (od == d && ot < t)) d = od, t = ot;
}

__global__ __launch_bounds__(CF_THREADS) void contact_frames_kernel(
    const float *__restrict__ joints, int B, int T, int J, int C, int N, int K, int stride,
    const double *__restrict__ node_obbs, const double *__restrict__ node_rmat, const int *__restrict__ count,
    int *__restrict__ frame, double *__restrict__ dist) {
  extern __shared__ float lds_x[];                     // CF_CH rows of `stride` floats: x, y, z of joint 0, of joint 1, ...
  const int tid = threadIdx.x, lane = tid & (P2R_WAVE - 1), wave = tid / P2R_WAVE;
  // group-major: the workgroups that have nodes (the first count / 4 of every sample) come first in the grid and spread
  // evenly over the XCDs, which take workgroups round-robin; sample-major, the nodes of a sample with 16 of them or fewer
  // all went to the same half of the XCDs
  const int n = blockIdx.x % N, s0 = (blockIdx.x / N) * CF_NODES;
  const int cnt = count[n];
  const int s = s0 + wave;                             // this wave's slot
  const bool live = s < K && s < cnt;
  if (s0 >= cnt) {                                     // uniform over the workgroup: no node here
    if (lane == 0 && s < K) frame[(long long)n * K + s] = -1, dist[(long long)n * K + s] = 0.0;
    return;
  }

  double ctr[3] = {0.0, 0.0, 0.0}, half[3] = {0.0, 0.0, 0.0}, R[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  if (live) {
    const long long o = (long long)n * K + s;
#pragma unroll
    for (int a = 0; a < 3; ++a) ctr[a] = node_obbs[o * 7 + a], half[a] = node_obbs[o * 7 + 3 + a] / 2.0;
#pragma unroll
    for (int a = 0; a < 9; ++a) R[a] = node_rmat[o * 9 + a];
  }

  const int JC = J * C;
  const float *src = joints + (long long)(n % B) * T * JC;
  double best_d = __longlong_as_double(0x7ff0000000000000LL);      // +inf
  int best_t = lane < T ? lane : 0x7fffffff;                       // a lane without a frame never wins a tie
  for (int t0 = 0; t0 < T; t0 += CF_CH) {
    const int nf = T - t0 < CF_CH ? T - t0 : CF_CH;
    const float *chunk = src + (long long)t0 * JC;
    // coalesced: the chunk is contiguous in memory.  CF_LD loads are in flight per thread before the first is stored: the
    // copy is bound by the latency of a load (one load at a time: 3.6 instead of 2.8 ms at 320 samples)
    const int total = nf * JC;
    for (int e0 = tid; e0 < total; e0 += CF_THREADS * CF_LD) {
      float v[CF_LD];
#pragma unroll
      for (int i = 0; i < CF_LD; ++i) {
        const int e = e0 + i * CF_THREADS;
        v[i] = e < total ? chunk[e] : 0.0f;
      }
#pragma unroll
      for (int i = 0; i < CF_LD; ++i) {
        const int e = e0 + i * CF_THREADS;
        if (e < total) {
          const int f = e / JC, r = e - f * JC;
          if (C == 3) {
            lds_x[f * stride + r] = v[i];
          } else if ((r & 3) != 3) {
            lds_x[f * stride + (r >> 2) * 3 + (r & 3)] = v[i];
          }
        }
      }
    }
    __syncthreads();
    if (live && lane < nf) {
      const float *x = lds_x + lane * stride;
      double d = -__longlong_as_double(0x7ff0000000000000LL);
      for (int j = 0; j < J; ++j) {
        const double v0 = (double)x[j * 3] - ctr[0], v1 = (double)x[j * 3 + 1] - ctr[1],
                     v2 = (double)x[j * 3 + 2] - ctr[2];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
          const double g = fabs((v0 * R[a * 3] + v1 * R[a * 3 + 1]) + v2 * R[a * 3 + 2]) - half[a];
          d = g > d ? g : d;
        }
      }
      if (d < best_d) best_d = d, best_t = t0 + lane;
    }
    __syncthreads();
  }
  if (!live) {
    if (lane == 0 && s < K) frame[(long long)n * K + s] = -1, dist[(long long)n * K + s] = 0.0;
    return;
  }
#pragma unroll
  for (int m = P2R_WAVE / 2; m >= 1; m >>= 1) {
    const double od = __shfl_xor(best_d, m);
    const int ot = __shfl_xor(best_t, m);
    take_min(best_d, best_t, od, ot);
  }
  if (lane == 0) {
    if (best_t >= T) best_t = 0;                       // every d(t) a NaN: unspecified, but a frame of the recording
    frame[(long long)n * K + s] = best_t;
    dist[(long long)n * K + s] = best_d;
  }
}

__device__ __forceinline__ unsigned mix32(unsigned bits, unsigned pos) {
  unsigned h = (bits ^ (pos * 0x9E3779B9u)) * 0x85EBCA6Bu;
  h ^= h >> 15;
  h *= 0xC2B2AE35u;
  h ^= h >> 13;
  return h;
}

__device__ __forceinline__ bool rows_equal(const float *__restrict__ a, const float *__restrict__ b, int JC) {
  bool eq = true;
  for (int i = 0; i < JC; ++i) eq = eq && a[i] == b[i];
  return eq;
}

__global__ __launch_bounds__(UF_THREADS) void unique_frames_kernel(const float *__restrict__ joints, int T, int JC,
                                                                   int *__restrict__ count, int *__restrict__ index,
                                                                   int *__restrict__ rank) {
  extern __shared__ int lds_i[];
  __shared__ int lds_w[UF_THREADS / P2R_WAVE];
  unsigned *hash = (unsigned *)lds_i;                  // T hashes
  int *first = lds_i + T;                              // T: the first frame with frame t's row; -1 while a NaN row waits
  int *slot = lds_i + 2 * T;                           // T: position in `index` of a first occurrence
  const int tid = threadIdx.x, lane = tid & (P2R_WAVE - 1), wave = tid / P2R_WAVE;
  const float *src = joints + (long long)blockIdx.x * T * JC;
  int *idx_out = index + (long long)blockIdx.x * T, *rank_out = rank + (long long)blockIdx.x * T;

  for (int t = wave; t < T; t += UF_THREADS / P2R_WAVE) {
    const float *row = src + (long long)t * JC;
    unsigned h = 0;
    bool nan = false;
    for (int i = lane; i < JC; i += P2R_WAVE) {
      const float x = row[i];
      nan = nan || x != x;
      h += mix32(x == 0.0f ? 0u : __float_as_uint(x), (unsigned)i);
    }
#pragma unroll
    for (int m = P2R_WAVE / 2; m >= 1; m >>= 1) h += __shfl_xor(h, m);
    const bool any_nan = __ballot(nan) != 0ull;
    if (lane == 0) hash[t] = h, first[t] = any_nan ? -1 : t;
  }
  __syncthreads();

  for (int t = tid; t < T; t += UF_THREADS) {
    if (first[t] < 0) continue;                        // a NaN row equals no row
    const unsigned h = hash[t];
    const float *row = src + (long long)t * JC;
    int f = t;
    for (int u = 0; u < t; ++u) {
      if (hash[u] == h && rows_equal(src + (long long)u * JC, row, JC)) {
        f = u;
        break;
      }
    }
    first[t] = f;          // only thread t writes or reads first[t] in this phase; a NaN row u fails rows_equal
  }
  __syncthreads();

  int running = 0;
  for (int t0 = 0; t0 < T; t0 += UF_THREADS) {
    const int t = t0 + tid;
    bool is_first = false;
    if (t < T) {
      if (first[t] < 0) first[t] = t;
      is_first = first[t] == t;
    }
    const int p = compact_slot<UF_THREADS / P2R_WAVE>(is_first, running, lds_w);
    if (is_first) slot[t] = p, idx_out[p] = t;
  }
  __syncthreads();
  for (int t = tid; t < T; t += UF_THREADS) {
    rank_out[t] = slot[first[t]];
    if (t >= running) idx_out[t] = -1;
  }
  if (tid == 0) count[blockIdx.x] = running;
}

bool fits_int(long long v) { return v >= 0 && v <= 0x7fffffffLL; }

}  // namespace

extern "C" int p2r_scene_nodes(int N, int K, const double *obbs, const float *obj_prob, const unsigned char *pred_mask,
                               const long long *pred_cls, double dump_threshold, int *count, int *inst_idx,
                               double *node_obbs, double *node_rmat, long long *node_cls, float *node_score,
                               void *stream) {
  if (N < 0 || K < 0 || K > P2R_SCENE_MAX_K || !fits_int((long long)N * K)) return P2R_EINVAL;
  if (N > 0 && !count) return P2R_EINVAL;
  if ((long long)N * K > 0 &&
      (!obbs || !obj_prob || !pred_mask || !pred_cls || !inst_idx || !node_obbs || !node_rmat || !node_cls || !node_score))
    return P2R_EINVAL;
  if (N == 0) return P2R_OK;
  hipLaunchKernelGGL(scene_nodes_kernel, dim3((unsigned)N), dim3(SN_THREADS), 0, p2r_stream(stream), K, obbs, obj_prob,
                     pred_mask, pred_cls, dump_threshold, count, inst_idx, node_obbs, node_rmat, node_cls, node_score);
  P2R_LAUNCH_CHECK();
  return P2R_OK;
}

extern "C" int p2r_contact_frames(const float *joints, int B, int T, int J, int C, int N, int K, const double *node_obbs,
                                  const double *node_rmat, const int *count, int *frame, double *dist, void *stream) {
  if (N < 0 || B < 1 || N % B != 0 || T < 1 || T > P2R_SCENE_MAX_T || J < 1 || J > P2R_SCENE_MAX_J || (C != 3 && C != 4) ||
      K < 0 || K > P2R_SCENE_MAX_K || !fits_int((long long)N * K))
    return P2R_EINVAL;
  if ((long long)N * K == 0) return P2R_OK;
  if (!joints || !node_obbs || !node_rmat || !count || !frame || !dist) return P2R_EINVAL;
  const int groups = p2r_cdiv(K, CF_NODES);
  if (!fits_int((long long)N * groups)) return P2R_EINVAL;
  const int stride = (3 * J) | 1;                      // odd: lane l reads bank (l * stride + const) % 64, all different
  hipLaunchKernelGGL(contact_frames_kernel, dim3((unsigned)(N * groups)), dim3(CF_THREADS),
                     (size_t)CF_CH * stride * sizeof(float), p2r_stream(stream), joints, B, T, J, C, N, K, stride,
                     node_obbs, node_rmat, count, frame, dist);
  P2R_LAUNCH_CHECK();
  return P2R_OK;
}

extern "C" int p2r_unique_frames(const float *joints, int B, int T, int J, int C, int *count, int *index, int *rank,
                                 void *stream) {
  if (B < 0 || T < 1 || T > P2R_UNIQUE_MAX_T || J < 1 || J > P2R_SCENE_MAX_J || (C != 3 && C != 4)) return P2R_EINVAL;
  if (B == 0) return P2R_OK;
  if (!joints || !count || !index || !rank) return P2R_EINVAL;
  hipLaunchKernelGGL(unique_frames_kernel, dim3((unsigned)B), dim3(UF_THREADS), (size_t)3 * T * sizeof(int),
                     p2r_stream(stream), joints, T, J * C, count, index, rank);
  P2R_LAUNCH_CHECK();
  return P2R_OK;
}
