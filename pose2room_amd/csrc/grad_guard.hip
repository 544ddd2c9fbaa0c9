// grad_guard.hip -- the gradients of one train step measured and clipped on the device (include/p2r_grad_guard.h): what
// torch.nn.utils.clip_grad_norm_ does with a norm per tensor, a stack, a second norm, a handful of scalar operations and
// a multiply over every gradient, plus the count of non-finite entries that it does not take.
//
//   gg_measure_kernel   one workgroup per chunk of P2R_GG_CHUNK elements.  The table of a group of gradients -- pointer,
//                       numel, first chunk, dtype -- is a kernel argument by value: the workgroup finds its gradient by a
//                       search over uniform loads and streams its chunk with one 16-byte load per lane and step.  The
//                       order of the sums is tied to the ELEMENT INDEX, never to the address (p2r_grad_guard.h): a
//                       gradient that does not start on a 16-byte boundary is read with dword-aligned 16-byte loads of the
//                       same groups, not with an address-dependent scalar head, which would move every element to another
//                       accumulator.  Squares are float64 (exact for f32 inputs), partial sums float64.
//   gg_finish_kernel    one workgroup.  Thread t adds the partials of gradients t, t + 256, ... in chunk order; thread 0
//                       adds the gradients in table order out of LDS and writes norm, scale, found and the counters.
//                       A launch of its own, not a "last workgroup finishes" handshake inside the first: the handshake
//                       needs an agent-scope release and acquire per workgroup to be right across XCDs and costs more
//                       than the launch boundary it saves.
//   gg_scale_kernel     g / scale in place, same table, same chunks; every workgroup returns when scale == 1.
//
// 8 MB of gradients in 131 tensors: the work is launches and kernel boundaries, not bandwidth.
#include "p2r_common.h"

#include "../../include/p2r_grad_guard.h"

namespace {

constexpr int GG_THREADS = 256;
constexpr int GG_WAVES = GG_THREADS / P2R_WAVE;
constexpr int GG_TILE = 2048;                        // gradients per LDS tile of the finishing workgroup

// The table of one launch.  3240 bytes: kernel arguments may take 4096.
struct gg_group {
  const void *data[P2R_GG_GROUP];
  long long numel[P2R_GG_GROUP];
  int first[P2R_GG_GROUP + 1];                       // first chunk of entry e inside the group; first[n] = chunks of the group
  unsigned f64[(P2R_GG_GROUP + 31) / 32];            // bit e: entry e is f64
  int n, entry0, chunk0;                             // entries; table index of entry 0; global index of chunk 0
};
static_assert(sizeof(gg_group) <= 3584, "the group must fit the kernel arguments with room for the pointers");

// 16 bytes of elements at dword (f32) or qword (f64) alignment
struct __attribute__((packed, aligned(4))) gg_f4u { float v[4]; };
struct __attribute__((packed, aligned(8))) gg_d2u { double v[2]; };

__device__ __forceinline__ bool gg_finite(float x) { return (__float_as_uint(x) & 0x7f800000u) != 0x7f800000u; }
__device__ __forceinline__ bool gg_finite(double x) {
  return ((unsigned)__double2hiint(x) & 0x7ff00000u) != 0x7ff00000u;
}

template <typename T>
__device__ __forceinline__ void gg_take(T x, double &acc, int &bad) {
  const bool fin = gg_finite(x);
  const double d = fin ? (double)x : 0.0;
  acc += d * d;
  bad += fin ? 0 : 1;
}

template <typename T> struct gg_vec;
template <> struct gg_vec<float> { static constexpr int N = 4; using aligned = float4; using dword = gg_f4u; };
template <> struct gg_vec<double> { static constexpr int N = 2; using aligned = double2; using dword = gg_d2u; };

template <typename T, bool ALIGNED>
__device__ __forceinline__ void gg_load(const T *p, T (&x)[gg_vec<T>::N]) {
  if constexpr (ALIGNED) {
    const typename gg_vec<T>::aligned v = *reinterpret_cast<const typename gg_vec<T>::aligned *>(p);
    if constexpr (gg_vec<T>::N == 4) { x[0] = v.x; x[1] = v.y; x[2] = v.z; x[3] = v.w; }
    else { x[0] = v.x; x[1] = v.y; }
  } else {
    const typename gg_vec<T>::dword v = *reinterpret_cast<const typename gg_vec<T>::dword *>(p);
#pragma unroll
    for (int e = 0; e < gg_vec<T>::N; ++e) x[e] = v.v[e];
  }
}

// The `len` (1 .. P2R_GG_CHUNK) elements at p: this thread's share of the sum of finite squares and of the non-finite
// count.  Group m = elements m * N .. m * N + N - 1 belongs to thread m % 256; element e of a group to accumulator e.
template <typename T, bool ALIGNED>
__device__ __forceinline__ void gg_chunk(const T *__restrict__ p, int len, double &sum, int &bad) {
  constexpr int N = gg_vec<T>::N;
  double acc[N];
#pragma unroll
  for (int e = 0; e < N; ++e) acc[e] = 0.0;
  const int whole = len / N;
#pragma unroll 4
  for (int m = threadIdx.x; m < whole; m += GG_THREADS) {
    T x[N];
    gg_load<T, ALIGNED>(p + (size_t)m * N, x);
#pragma unroll
    for (int e = 0; e < N; ++e) gg_take(x[e], acc[e], bad);
  }
  // behind the last whole group of a gradient: single elements, in the thread and the accumulators that their group has
  if (whole * N < len && (int)threadIdx.x == whole % GG_THREADS) {
#pragma unroll
    for (int e = 0; e < N - 1; ++e)
      if (whole * N + e < len) gg_take(p[whole * N + e], acc[e], bad);
  }
  sum = acc[0];
#pragma unroll
  for (int e = 1; e < N; ++e) sum += acc[e];
}

template <typename T>
__device__ __forceinline__ void gg_chunk_any(const void *data, long long start, int len, double &sum, int &bad) {
  const T *p = static_cast<const T *>(data) + start;
  if ((reinterpret_cast<uintptr_t>(p) & 15) == 0) gg_chunk<T, true>(p, len, sum, bad);
  else gg_chunk<T, false>(p, len, sum, bad);
}

// entry of chunk b of the group: the last e with first[e] <= b (every entry owns at least one chunk)
__device__ __forceinline__ int gg_entry(const gg_group &g, int b) {
  int lo = 0, hi = g.n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (g.first[mid] <= b) lo = mid; else hi = mid - 1;
  }
  return lo;
}

__global__ __launch_bounds__(GG_THREADS) void gg_measure_kernel(const gg_group g, double *__restrict__ part_sumsq,
                                                                int *__restrict__ part_count,
                                                                int *__restrict__ first_chunk) {
  __shared__ double s_sum[GG_WAVES];
  __shared__ int s_bad[GG_WAVES];
  const int b = blockIdx.x;
  const int e = gg_entry(g, b);
  const int c = b - g.first[e];
  const long long numel = g.numel[e];
  const long long start = (long long)c * P2R_GG_CHUNK;
  const long long left = numel - start;
  const int len = left < P2R_GG_CHUNK ? (int)left : P2R_GG_CHUNK;      // 0 for an entry without elements
  double sum = 0.0;
  int bad = 0;
  if (len > 0) {
    if ((g.f64[e >> 5] >> (e & 31)) & 1u) gg_chunk_any<double>(g.data[e], start, len, sum, bad);
    else gg_chunk_any<float>(g.data[e], start, len, sum, bad);
  }
  // lanes: xor butterfly (both partners form the same sum); waves: ascending
#pragma unroll
  for (int off = P2R_WAVE / 2; off >= 1; off >>= 1) {
    sum += __shfl_xor(sum, off, P2R_WAVE);
    bad += __shfl_xor(bad, off, P2R_WAVE);
  }
  const int lane = threadIdx.x & (P2R_WAVE - 1), wave = threadIdx.x / P2R_WAVE;
  if (lane == 0) { s_sum[wave] = sum; s_bad[wave] = bad; }
  __syncthreads();
  if (threadIdx.x == 0) {
    double s = s_sum[0];
    int k = s_bad[0];
#pragma unroll
    for (int w = 1; w < GG_WAVES; ++w) { s += s_sum[w]; k += s_bad[w]; }
    part_sumsq[g.chunk0 + b] = s;
    part_count[g.chunk0 + b] = k;
    if (c == 0) first_chunk[g.entry0 + e] = g.chunk0 + b;
  }
}

__global__ __launch_bounds__(GG_THREADS) void gg_finish_kernel(
    int n, int n_chunks, double max_norm, int count_skips, const double *__restrict__ part_sumsq,
    const int *__restrict__ part_count, const int *__restrict__ first_chunk, double *__restrict__ sumsq,
    int *__restrict__ nonfinite, double *__restrict__ norm, float *__restrict__ scale, float *__restrict__ found,
    long long *__restrict__ steps, long long *__restrict__ skipped) {
  __shared__ double s_sum[GG_TILE];
  __shared__ int s_bad[GG_TILE];
  double total = 0.0;                                  // thread 0 only
  long long bad_total = 0;
  for (int base = 0; base < n; base += GG_TILE) {
    const int m = n - base < GG_TILE ? n - base : GG_TILE;
    for (int t = threadIdx.x; t < m; t += GG_THREADS) {
      const int i = base + t;
      const int c0 = first_chunk[i], c1 = i + 1 < n ? first_chunk[i + 1] : n_chunks;
      double s = 0.0;
      int k = 0;
#pragma unroll 4
      for (int c = c0; c < c1; ++c) { s += part_sumsq[c]; k += part_count[c]; }
      sumsq[i] = s;
      nonfinite[i] = k;
      s_sum[t] = s;
      s_bad[t] = k;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll 8
      for (int t = 0; t < m; ++t) { total += s_sum[t]; bad_total += s_bad[t]; }
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const double nrm = sqrt(total);
    float sc = 1.0f;
    if (max_norm > 0.0) {
      const double d = (nrm + 1e-6) / max_norm;
      sc = (float)(d > 1.0 ? d : 1.0);
    }
    norm[0] = nrm;
    scale[0] = sc;
    found[0] = bad_total > 0 ? 1.0f : 0.0f;
    steps[0] = steps[0] + 1;
    skipped[0] = skipped[0] + ((bad_total > 0 && count_skips != 0) ? 1 : 0);
  }
}

template <typename T>
__device__ __forceinline__ void gg_divide(void *data, long long start, int len, float scale) {
  constexpr int N = gg_vec<T>::N;
  T *p = static_cast<T *>(data) + start;
  const T s = (T)scale;
  // whole 16-byte groups from the first aligned element on; the elements in front of it and behind them one by one
  int head = (int)(((16 - (reinterpret_cast<uintptr_t>(p) & 15)) & 15) / sizeof(T));
  if (head > len) head = len;
  const int whole = (len - head) / N;
  using V = typename gg_vec<T>::aligned;
  V *pv = reinterpret_cast<V *>(p + head);
#pragma unroll 4
  for (int m = threadIdx.x; m < whole; m += GG_THREADS) {
    V v = pv[m];
    v.x = v.x / s;
    v.y = v.y / s;
    if constexpr (N == 4) { v.z = v.z / s; v.w = v.w / s; }
    pv[m] = v;
  }
  const int rest = len - whole * N;                    // head + tail: at most 2 * (N - 1) elements
  if ((int)threadIdx.x < rest) {
    const int j = (int)threadIdx.x < head ? (int)threadIdx.x : whole * N + (int)threadIdx.x;
    p[j] = p[j] / s;
  }
}

__global__ __launch_bounds__(GG_THREADS) void gg_scale_kernel(const gg_group g, const float *__restrict__ scale) {
  const float s = scale[0];
  if (s == 1.0f) return;
  const int b = blockIdx.x;
  const int e = gg_entry(g, b);
  const long long start = (long long)(b - g.first[e]) * P2R_GG_CHUNK;
  const long long left = g.numel[e] - start;
  const int len = left < P2R_GG_CHUNK ? (int)left : P2R_GG_CHUNK;
  if (len <= 0) return;
  if ((g.f64[e >> 5] >> (e & 31)) & 1u) gg_divide<double>(const_cast<void *>(g.data[e]), start, len, s);
  else gg_divide<float>(const_cast<void *>(g.data[e]), start, len, s);
}

long long gg_chunks_of(long long numel) {
  return numel <= 0 ? 1 : (numel + P2R_GG_CHUNK - 1) / P2R_GG_CHUNK;
}

// -> the sum of the chunks of the table, or -1 for a table outside the limits
long long gg_validate(const p2r_grad_entry *table, int n) {
  if (n < 0 || (n > 0 && !table)) return -1;
  long long total = 0;
  for (int i = 0; i < n; ++i) {
    const p2r_grad_entry &t = table[i];
    if (t.numel < 0 || (t.dtype != P2R_GG_F32 && t.dtype != P2R_GG_F64)) return -1;
    if (t.numel > 0 && !t.data) return -1;
    if (reinterpret_cast<uintptr_t>(t.data) % (t.dtype == P2R_GG_F64 ? 8 : 4) != 0) return -1;
    total += gg_chunks_of(t.numel);
    if (total > 0x7fffffffLL) return -1;
  }
  return total;
}

// Calls launch(group) for every group of up to P2R_GG_GROUP consecutive entries; stops at the first error.
template <typename F>
int gg_for_groups(const p2r_grad_entry *table, int n, F launch) {
  int chunk0 = 0;
  for (int entry0 = 0; entry0 < n; entry0 += P2R_GG_GROUP) {
    gg_group g = {};
    g.n = n - entry0 < P2R_GG_GROUP ? n - entry0 : P2R_GG_GROUP;
    g.entry0 = entry0;
    g.chunk0 = chunk0;
    int chunks = 0;
    for (int e = 0; e < g.n; ++e) {
      const p2r_grad_entry &t = table[entry0 + e];
      g.data[e] = t.data;
      g.numel[e] = t.numel;
      g.first[e] = chunks;
      if (t.dtype == P2R_GG_F64) g.f64[e >> 5] |= 1u << (e & 31);
      chunks += (int)gg_chunks_of(t.numel);
    }
    g.first[g.n] = chunks;
    const int status = launch(g, chunks);
    if (status != P2R_OK) return status;
    chunk0 += chunks;
  }
  return P2R_OK;
}

}  // namespace

extern "C" int p2r_grad_measure(const p2r_grad_entry *table, int n, double max_norm, int count_skips, int n_chunks,
                                double *part_sumsq, int *part_count, int *first_chunk, double *sumsq, int *nonfinite,
                                double *norm, float *scale, float *found, long long *steps, long long *skipped,
                                void *stream) {
  const long long total = gg_validate(table, n);
  if (total < 0 || total != (long long)n_chunks || max_norm != max_norm) return P2R_EINVAL;
  if (!norm || !scale || !found || !steps || !skipped) return P2R_EINVAL;
  if (n > 0 && (!part_sumsq || !part_count || !first_chunk || !sumsq || !nonfinite)) return P2R_EINVAL;
  const int status = gg_for_groups(table, n, [&](const gg_group &g, int chunks) {
    hipLaunchKernelGGL(gg_measure_kernel, dim3((unsigned)chunks), dim3(GG_THREADS), 0, p2r_stream(stream), g, part_sumsq,
                       part_count, first_chunk);
    P2R_LAUNCH_CHECK();
    return (int)P2R_OK;
  });
  if (status != P2R_OK) return status;
  hipLaunchKernelGGL(gg_finish_kernel, dim3(1), dim3(GG_THREADS), 0, p2r_stream(stream), n, n_chunks, max_norm,
                     count_skips, part_sumsq, part_count, first_chunk, sumsq, nonfinite, norm, scale, found, steps, skipped);
  P2R_LAUNCH_CHECK();
  return P2R_OK;
}

extern "C" int p2r_grad_scale(const p2r_grad_entry *table, int n, const float *scale, void *stream) {
  const long long total = gg_validate(table, n);
  if (total < 0) return P2R_EINVAL;
  long long elements = 0;
  for (int i = 0; i < n; ++i) elements += table[i].numel > 0 ? 1 : 0;
  if (elements == 0) return P2R_OK;
  if (!scale) return P2R_EINVAL;
  return gg_for_groups(table, n, [&](const gg_group &g, int chunks) {
    hipLaunchKernelGGL(gg_scale_kernel, dim3((unsigned)chunks), dim3(GG_THREADS), 0, p2r_stream(stream), g, scale);
    P2R_LAUNCH_CHECK();
    return (int)P2R_OK;
  });
}
