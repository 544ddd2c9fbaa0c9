// interaction.hip -- the interaction timeline of a scene on the device (include/p2r_interaction.h): in which frames the
// body is in contact with which object node, with which joints, and the intervals those frames form.
//
//   p2r_contact_bits       the work: N * K * T * J enlarged-box tests in fp64, the loop of scene.hip's
//                          contact_frames_kernel.  One workgroup owns CB_NODES = 4 consecutive slots of a sample, one per
//                          wave; the frames pass through LDS in chunks of 64 with an odd row stride, copied with coalesced
//                          loads, and lane l of every wave walks the joints of frame l of the chunk.  A chunk of 64 frames
//                          is one word of `bits`: one ballot, stored by lane 0.  Every lane ORs the joints it saw inside
//                          into a 64-bit mask of its own; the only cross-lane step is the OR of those masks at the end.
//                          A workgroup whose four slots are all empty writes its zeros and returns.
//   p2r_contact_intervals  one wave (one workgroup of 64 threads) per node, lane = word, chunks of 64 words.  The node's
//                          words sit in LDS.  Merging needs, per word, the last set bit in the words before it and the
//                          first set bit in the words after it: a prefix maximum over the lanes with a carry from chunk
//                          to chunk going up, a suffix minimum with a carry going down; inside a word the zero runs are
//                          walked with ctz (at most 33 per word).  Dropping short runs is the same walk over the runs of
//                          ones with the scans taken over the complement.  The k-th run start and the k-th run end of a
//                          node belong to the same run, so starts and ends get their slots independently from popcounts
//                          and a prefix over the lanes.  No atomics.
//   p2r_frame_labels       one thread per (n, t); the loop over the slots reads one word per slot and wave (uniform) and
//                          one byte of njoint per slot whose bit is set.
#include "p2r_common.h"

#include "../../include/p2r_interaction.h"

namespace {

constexpr int CB_THREADS = 256;
constexpr int CB_NODES = CB_THREADS / P2R_WAVE;      // slots per workgroup, one per wave
constexpr int CB_CH = P2R_WAVE;                      // frames per chunk, one per lane: one word of `bits`
constexpr int CB_LD = 16;                            // loads a thread has in flight while a chunk is copied
constexpr int FL_THREADS = 256;
constexpr int NONE = 0x7fffffff;                     // "no bit after this word"

__device__ __forceinline__ unsigned long long or_lanes(unsigned long long v) {
#pragma unroll
  for (int m = P2R_WAVE / 2; m >= 1; m >>= 1) {
    const unsigned lo = __shfl_xor((unsigned)v, m), hi = __shfl_xor((unsigned)(v >> 32), m);
    v |= ((unsigned long long)hi << 32) | lo;
  }
  return v;
}

__global__ __launch_bounds__(CB_THREADS) void contact_bits_kernel(
    const float *__restrict__ joints, int B, int T, int J, int C, int N, int K, int W, int stride,
    const double *__restrict__ node_obbs, const double *__restrict__ node_rmat, const int *__restrict__ count,
    double contact_thresh, unsigned long long *__restrict__ bits, unsigned char *__restrict__ njoint,
    unsigned long long *__restrict__ joint_mask, int *__restrict__ n_raw) {
  extern __shared__ float lds_x[];                     // CB_CH rows of `stride` floats: x, y, z of joint 0, of joint 1, ...
  const int tid = threadIdx.x, lane = tid & (P2R_WAVE - 1), wave = tid / P2R_WAVE;
  // group-major, as contact_frames_kernel: the workgroups that have nodes come first and spread over the XCDs
  const int n = blockIdx.x % N, s0 = (blockIdx.x / N) * CB_NODES;
  const int cnt = count[n];
  const int s = s0 + wave;                             // this wave's slot
  const bool live = s < K && s < cnt;
  const long long o = (long long)n * K + s;            // used only where s < K
  if (s0 >= cnt) {                                     // uniform over the workgroup: no node here
    if (s < K) {
      for (int w = lane; w < W; w += P2R_WAVE) bits[o * W + w] = 0ull;
      if (njoint)
        for (int t = lane; t < T; t += P2R_WAVE) njoint[o * T + t] = 0;
      if (lane == 0) joint_mask[o] = 0ull, n_raw[o] = 0;
    }
    return;
  }

  double ctr[3] = {0.0, 0.0, 0.0}, half[3] = {0.0, 0.0, 0.0}, R[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  if (live) {
#pragma unroll
    for (int a = 0; a < 3; ++a) ctr[a] = node_obbs[o * 7 + a], half[a] = node_obbs[o * 7 + 3 + a] / 2.0 + contact_thresh;
#pragma unroll
    for (int a = 0; a < 9; ++a) R[a] = node_rmat[o * 9 + a];
  }

  const int JC = J * C;
  const float *src = joints + (long long)(n % B) * T * JC;
  unsigned long long jmask = 0ull;                     // the joints this lane saw inside
  int raw = 0;                                         // uniform over the wave
  for (int t0 = 0; t0 < T; t0 += CB_CH) {
    const int nf = T - t0 < CB_CH ? T - t0 : CB_CH;
    const float *chunk = src + (long long)t0 * JC;
    const int total = nf * JC;                         // the chunk is contiguous in memory: coalesced
    for (int e0 = tid; e0 < total; e0 += CB_THREADS * CB_LD) {
      float v[CB_LD];
#pragma unroll
      for (int i = 0; i < CB_LD; ++i) {
        const int e = e0 + i * CB_THREADS;
        v[i] = e < total ? chunk[e] : 0.0f;
      }
#pragma unroll
      for (int i = 0; i < CB_LD; ++i) {
        const int e = e0 + i * CB_THREADS;
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
    int in = 0;
    if (live && lane < nf) {
      const float *x = lds_x + lane * stride;
      for (int j = 0; j < J; ++j) {
        const double d0 = (double)x[j * 3] - ctr[0], d1 = (double)x[j * 3 + 1] - ctr[1],
                     d2 = (double)x[j * 3 + 2] - ctr[2];
        // all three axes are evaluated and combined with &, and the count and the mask take the flag as a number: with
        // && and an `if` the compiler branches on every axis of every joint and the joints no longer overlap
        unsigned inside = 1u;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
          const double local = ((0.0 + d0 * R[a * 3]) + d1 * R[a * 3 + 1]) + d2 * R[a * 3 + 2];
          inside &= fabs(local) <= half[a] ? 1u : 0u;  // 0 for a NaN
        }
        in += (int)inside;
        jmask |= (unsigned long long)inside << j;
      }
    }
    const unsigned long long word = __ballot(in > 0);  // lanes without a frame vote 0: the padding bits
    raw += __popcll(word);
    if (s < K) {
      if (lane == 0) bits[o * W + t0 / CB_CH] = word;
      if (njoint && lane < nf) njoint[o * T + t0 + lane] = (unsigned char)in;
    }
    __syncthreads();
  }
  if (s >= K) return;
  jmask = or_lanes(jmask);
  if (lane == 0) joint_mask[o] = jmask, n_raw[o] = raw;
}

// ---- intervals -------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned long long span_mask(int lo, int hi) {       // bits lo .. hi-1, 0 <= lo < hi <= 64
  return (hi >= 64 ? ~0ull : (1ull << hi) - 1ull) & ~((1ull << lo) - 1ull);
}

// before[w] = the position of the last set bit in the words below w (-1: none), for the W words x[] of this wave's node
__device__ __forceinline__ void scan_last_before(const unsigned long long *x, int W, int lane, int *before) {
  int carry = -1;
  for (int w0 = 0; w0 < W; w0 += P2R_WAVE) {
    const int w = w0 + lane;
    const unsigned long long v = w < W ? x[w] : 0ull;
    int incl = v ? 64 * w + 63 - __builtin_clzll(v) : -1;
#pragma unroll
    for (int d = 1; d < P2R_WAVE; d <<= 1) {
      const int o = __shfl_up(incl, d);
      if (lane >= d && o > incl) incl = o;
    }
    int excl = __shfl_up(incl, 1);
    if (lane == 0) excl = -1;
    if (w < W) before[w] = excl > carry ? excl : carry;
    const int top = __shfl(incl, P2R_WAVE - 1);
    carry = top > carry ? top : carry;
  }
}

// One step of the downward scan: -> the position of the first set bit in the words above w = w0 + lane (NONE: none);
// `carry` is that of the words above the chunk and moves on to the chunk below.
__device__ __forceinline__ int first_after(unsigned long long v, int w, int lane, int &carry) {
  int incl = v ? 64 * w + __builtin_ctzll(v) : NONE;
#pragma unroll
  for (int d = 1; d < P2R_WAVE; d <<= 1) {
    const int o = __shfl_down(incl, d);
    if (lane + d < P2R_WAVE && o < incl) incl = o;
  }
  int excl = __shfl_down(incl, 1);
  if (lane == P2R_WAVE - 1) excl = NONE;
  const int after = excl < carry ? excl : carry;
  const int bottom = __shfl(incl, 0);
  carry = bottom < carry ? bottom : carry;
  return after;
}

__global__ __launch_bounds__(P2R_WAVE) void contact_intervals_kernel(
    const unsigned long long *__restrict__ bits, const int *__restrict__ count, int K, int T, int W, int merge_gap,
    int min_len, int M, unsigned long long *__restrict__ clean, int *__restrict__ n_intervals, int *__restrict__ intervals,
    int *__restrict__ n_frames, int *__restrict__ first, int *__restrict__ last) {
  extern __shared__ unsigned long long lds_w[];        // W words, then W ints
  unsigned long long *x = lds_w;
  int *before = (int *)(lds_w + W);
  const int lane = threadIdx.x;
  const long long o = blockIdx.x;                      // n * K + s
  const int n = (int)(o / K), s = (int)(o - (long long)n * K);
  const bool live = s < count[n];
  const unsigned long long tail = (T & 63) ? (1ull << (T & 63)) - 1ull : ~0ull;
  const int chunks = (W + P2R_WAVE - 1) / P2R_WAVE;

  for (int w = lane; w < W; w += P2R_WAVE) x[w] = live ? bits[o * W + w] & (w == W - 1 ? tail : ~0ull) : 0ull;
  __syncthreads();

  // (2) merge: a run of zeros between the set bits a and b is filled when b - (a + 1) <= merge_gap
  scan_last_before(x, W, lane, before);
  __syncthreads();
  int carry = NONE;
  for (int c = chunks - 1; c >= 0; --c) {
    const int w = c * P2R_WAVE + lane;
    const unsigned long long v = w < W ? x[w] : 0ull;
    const int after = first_after(v, w, lane, carry);
    if (w < W) {
      const int prev = before[w];
      unsigned long long out = v, z = ~v;
      for (int it = 0; it < 33 && z; ++it) {
        const int lo = __builtin_ctzll(z);
        const int len = (z >> lo) == (~0ull >> lo) ? 64 - lo : __builtin_ctzll(~(z >> lo));     // up to bit 63: no ctz of 0
        const int hi = lo + len;
        const unsigned long long m = span_mask(lo, hi);
        const int a = lo > 0 ? 64 * w + lo - 1 : prev;
        const int b = hi < 64 ? 64 * w + hi : after;
        if (a >= 0 && b != NONE && b - (a + 1) <= merge_gap) out |= m;
        z &= ~m;
      }
      x[w] = out;                                      // only this lane reads or writes x[w] in this pass
    }
  }
  __syncthreads();

  // (3) drop the runs shorter than min_len: the same walk over the runs of ones, the scans over the complement.  The bits
  // at T and beyond are zeros of the complement's scan, so a run that reaches the last frame ends at T.
  for (int w = lane; w < W; w += P2R_WAVE) x[w] = ~x[w];
  __syncthreads();
  scan_last_before(x, W, lane, before);
  __syncthreads();
  carry = NONE;
  for (int c = chunks - 1; c >= 0; --c) {
    const int w = c * P2R_WAVE + lane;
    const unsigned long long zv = w < W ? x[w] : 0ull;
    const int after = first_after(zv, w, lane, carry);
    if (w < W) {
      const int prev = before[w];
      const unsigned long long v = ~zv;
      unsigned long long out = v, z = v;
      for (int it = 0; it < 33 && z; ++it) {
        const int lo = __builtin_ctzll(z);
        const int len = (z >> lo) == (~0ull >> lo) ? 64 - lo : __builtin_ctzll(~(z >> lo));
        const int hi = lo + len;
        const unsigned long long m = span_mask(lo, hi);
        const int start = lo > 0 ? 64 * w + lo : prev + 1;
        int end = hi < 64 ? 64 * w + hi : after;
        if (end > T) end = T;                          // NONE, or a padding position of the last word
        if (end - start < min_len) out &= ~m;
        z &= ~m;
      }
      x[w] = out & (w == W - 1 ? tail : ~0ull);
    }
  }
  __syncthreads();

  // the surviving runs: starts and ends get their slots independently, the k-th start and the k-th end are one run
  int *iv = intervals + o * M * 2;
  int run_s = 0, run_e = 0, frames = 0, lo_t = NONE, hi_t = -1;
  for (int w0 = 0; w0 < W; w0 += P2R_WAVE) {
    const int w = w0 + lane;
    unsigned long long v = 0ull, st = 0ull, en = 0ull;
    if (w < W) {
      v = x[w];
      const unsigned long long below = w > 0 ? x[w - 1] >> 63 : 0ull, above = w + 1 < W ? x[w + 1] << 63 : 0ull;
      st = v & ~((v << 1) | below);
      en = v & ~((v >> 1) | above);
      clean[o * W + w] = v;
    }
    int ps = __popcll(st), pe = __popcll(en), pf = __popcll(v);
    int is = ps, ie = pe;
#pragma unroll
    for (int d = 1; d < P2R_WAVE; d <<= 1) {
      const int a = __shfl_up(is, d), b = __shfl_up(ie, d);
      if (lane >= d) is += a, ie += b;
    }
    int slot_s = run_s + is - ps, slot_e = run_e + ie - pe;
    for (int it = 0; it < 32 && st; ++it, ++slot_s) {
      const int b = __builtin_ctzll(st);
      if (slot_s < M) iv[slot_s * 2] = 64 * w + b;
      st &= st - 1ull;
    }
    for (int it = 0; it < 32 && en; ++it, ++slot_e) {
      const int b = __builtin_ctzll(en);
      if (slot_e < M) iv[slot_e * 2 + 1] = 64 * w + b + 1;
      en &= en - 1ull;
    }
    run_s += __shfl(is, P2R_WAVE - 1);
    run_e += __shfl(ie, P2R_WAVE - 1);
    int f = v ? 64 * w + __builtin_ctzll(v) : NONE, l = v ? 64 * w + 63 - __builtin_clzll(v) : -1;
#pragma unroll
    for (int m = P2R_WAVE / 2; m >= 1; m >>= 1) {
      pf += __shfl_xor(pf, m);
      const int of = __shfl_xor(f, m), ol = __shfl_xor(l, m);
      f = of < f ? of : f;
      l = ol > l ? ol : l;
    }
    frames += pf;
    lo_t = f < lo_t ? f : lo_t;
    hi_t = l > hi_t ? l : hi_t;
  }
  if (lane < M && lane >= run_s) iv[lane * 2] = -1, iv[lane * 2 + 1] = -1;
  if (lane == 0) {
    n_intervals[o] = run_s;
    n_frames[o] = frames;
    first[o] = lo_t == NONE ? -1 : lo_t;
    last[o] = hi_t;
  }
}

// ---- labels ----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(FL_THREADS) void frame_labels_kernel(
    const unsigned long long *__restrict__ clean, const unsigned char *__restrict__ njoint, const int *__restrict__ count,
    int K, int T, int W, int *__restrict__ label, unsigned char *__restrict__ n_active, int *__restrict__ n_labelled) {
  const int tb = (T + FL_THREADS - 1) / FL_THREADS;
  const int n = blockIdx.x / tb, t = (blockIdx.x % tb) * FL_THREADS + threadIdx.x;        // a wave's 64 frames are one word
  const int lane = threadIdx.x & (P2R_WAVE - 1);
  int cnt = count[n];
  cnt = cnt < K ? cnt : K;
  int best = -1, best_s = -1, active = 0;
  if (t < T) {
    const long long row = (long long)n * K;
    for (int s = 0; s < cnt; ++s) {
      const unsigned long long word = clean[(row + s) * W + (t >> 6)];
      if ((word >> (t & 63)) & 1ull) {
        ++active;
        const int nj = njoint[(row + s) * T + t];
        if (nj > best) best = nj, best_s = s;          // ties stay with the lower slot
      }
    }
    label[(long long)n * T + t] = best_s;
    n_active[(long long)n * T + t] = (unsigned char)(active < 255 ? active : 255);
  }
  const unsigned long long any = __ballot(best_s >= 0);
  if (lane == 0 && any) atomicAdd(n_labelled + n, __popcll(any));
}

bool fits_int(long long v) { return v >= 0 && v <= 0x7fffffffLL; }

bool bad_shape(int N, int K, int T) {
  return N < 0 || K < 0 || K > P2R_INTERACTION_MAX_K || T < 1 || T > P2R_INTERACTION_MAX_T || !fits_int((long long)N * K) ||
         !fits_int((long long)N * K * T);
}

}  // namespace

extern "C" int p2r_contact_bits(const float *joints, int B, int T, int J, int C, int N, int K, const double *node_obbs,
                                const double *node_rmat, const int *count, double contact_thresh, long long *bits,
                                unsigned char *njoint, long long *joint_mask, int *n_raw, void *stream) {
  if (bad_shape(N, K, T) || B < 1 || N % B != 0 || J < 1 || J > P2R_INTERACTION_MAX_J || (C != 3 && C != 4))
    return P2R_EINVAL;
  if ((long long)N * K == 0) return P2R_OK;
  if (!joints || !node_obbs || !node_rmat || !count || !bits || !joint_mask || !n_raw) return P2R_EINVAL;
  const int groups = p2r_cdiv(K, CB_NODES);
  if (!fits_int((long long)N * groups)) return P2R_EINVAL;
  const int stride = (3 * J) | 1;                      // odd: lane l reads bank (l * stride + const) % 64, all different
  hipLaunchKernelGGL(contact_bits_kernel, dim3((unsigned)(N * groups)), dim3(CB_THREADS),
                     (size_t)CB_CH * stride * sizeof(float), p2r_stream(stream), joints, B, T, J, C, N, K, (T + 63) / 64,
                     stride, node_obbs, node_rmat, count, contact_thresh, (unsigned long long *)bits, njoint,
                     (unsigned long long *)joint_mask, n_raw);
  P2R_LAUNCH_CHECK();
  return P2R_OK;
}

extern "C" int p2r_contact_intervals(const long long *bits, const int *count, int N, int K, int T, int merge_gap,
                                     int min_len, int M, long long *clean, int *n_intervals, int *intervals,
                                     int *n_frames, int *first, int *last, void *stream) {
  if (bad_shape(N, K, T) || merge_gap < 0 || merge_gap > T || min_len < 1 || min_len > T || M < 1 ||
      M > P2R_INTERACTION_MAX_M || !fits_int((long long)N * K * M * 2))
    return P2R_EINVAL;
  if ((long long)N * K == 0) return P2R_OK;
  if (!bits || !count || !clean || !n_intervals || !intervals || !n_frames || !first || !last) return P2R_EINVAL;
  const int W = (T + 63) / 64;
  hipLaunchKernelGGL(contact_intervals_kernel, dim3((unsigned)(N * K)), dim3(P2R_WAVE),
                     (size_t)W * (sizeof(unsigned long long) + sizeof(int)), p2r_stream(stream),
                     (const unsigned long long *)bits, count, K, T, W, merge_gap, min_len, M, (unsigned long long *)clean,
                     n_intervals, intervals, n_frames, first, last);
  P2R_LAUNCH_CHECK();
  return P2R_OK;
}

extern "C" int p2r_frame_labels(const long long *clean, const unsigned char *njoint, const int *count, int N, int K, int T,
                                int *label, unsigned char *n_active, int *n_labelled, void *stream) {
  if (bad_shape(N, K, T) || !fits_int((long long)N * T)) return P2R_EINVAL;
  if (N == 0) return P2R_OK;
  if (!count || !label || !n_active || !n_labelled) return P2R_EINVAL;
  if (K > 0 && (!clean || !njoint)) return P2R_EINVAL;
  const hipError_t e = hipMemsetAsync(n_labelled, 0, sizeof(int) * (size_t)N, p2r_stream(stream));
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(frame_labels_kernel, dim3((unsigned)(N * p2r_cdiv(T, FL_THREADS))), dim3(FL_THREADS), 0,
                     p2r_stream(stream), (const unsigned long long *)clean, njoint, count, K, T, (T + 63) / 64, label,
                     n_active, n_labelled);
  P2R_LAUNCH_CHECK();
  return P2R_OK;
}
