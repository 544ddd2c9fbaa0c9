// mdn_sample.hip -- Bernoulli-gated mixture sampling for multi-hypothesis generation (include/p2r_hip.h:
// p2r_mdn_sample, p2r_mdn_sample_ex).  The reference's multi-mode read-out (mdn.py:49-69, generate_point_predictions(pi,
// n, sample_pi=True) with central_tendency 'mean' or 'median') draws a (B*L, G, n, D) normal tensor and a (B*L, G, n)
// Bernoulli gate per head and hypothesis; here every draw comes from a counter-based generator inside the kernel and
// nothing is materialised unless the caller asks for the draws (second half of this file).
//
// Random stream (the contract that the host mirror, pose2room_amd/p2rnet/mdn_sample_op.py, reproduces)
// ----------------------------------------------------------------------------------------------------
//   generator   Philox4x32-10 (Salmon, Moraes, Dror, Shaw, SC'11): multipliers 0xD2511F53 / 0xCD9E8D57, Weyl
//               increments 0x9E3779B9 / 0xBB67AE85, ten rounds, the key bumped between rounds.
//   key         (k0, k1) = (seed & 0xffffffff, seed >> 32)
//   counter     c0 = row = b * L + l
//               c1 = g | s << 8 | head_id << 16            (g < 256 component, s < 256 sample, head_id < 256)
//               c2 = hypothesis stream index (h_offset + i)
//               c3 = j, the block of the draw (below)
//   uniforms    u24(x) = (x >> 8) * 2^-24                                          in [0, 1)
//               u53(a, b) = ((a >> 5) * 2^26 + (b >> 6)) * 2^-53                   in [0, 1), double
//   normals     Box-Muller: r = sqrt(-2 log(1 - u1)) (log argument in (0, 1]), n_a = r cos(2 pi u2), n_b = r sin(2 pi u2)
//   block j = 0 (x0..x3): the gate, [u24(x0) < pi[b, g, l]] compared in f32.  Only a gated draw reads the blocks below
//               (the others are skipped; their counters stay reserved, so the stream does not depend on the gates).
//   f32 head    eps_0, eps_1 = BM(u24(x1), u24(x2)) of block 0 (x3 unused);  D > 2: eps_2, eps_3 = BM(u24(y0), u24(y1))
//               of block 1.  Box-Muller in f32 (logf, sqrtf, sincospif(2 u2)).
//   f64 head    eps_0, eps_1 = BM(u53(y0, y1), u53(y2, y3)) of block 1;  D > 2: the same from block 2.  Box-Muller in
//               double (log, sqrt, sincospi(2 u2)).
//   sigma       f32 head: expf(log_sigma); f64 head: exp((double)log_sigma).  One component's value is mu + sigma * eps
//               in the head's type (no contraction), accumulated in double.
// The stream is indexed by (head_id, hypothesis, row, g, s) alone: launch geometry, the split of the hypotheses over
// calls (h_offset) and the block size do not change a draw.
//
// Layout: a workgroup owns 16 rows of one (head, hypothesis); thread (r = tid & 15, q = tid >> 4) takes samples
// s = q, q + 16, ... of row r, components in order inside.  pi for the 16 rows and mu / sigma of the head sit in LDS.
// The 16 sample slices of a row meet in LDS and are added in slice order: a fixed-order reduction, so outputs are
// bit-identical from run to run.  The work is Philox's 32-bit multiplies and Box-Muller's transcendentals; memory
// traffic is pi once per (head, hypothesis) and the output.
#include "p2r_common.h"

namespace {

constexpr int SMP_ROWS = 16, SMP_SLICES = 16, SMP_THREADS = SMP_ROWS * SMP_SLICES;
constexpr int SMP_GMAX = 256, SMP_DMAX = 4, SMP_NMAX = 256;
constexpr int SMP_HCHUNK = 64;      // hypotheses per launch (their sample counts travel in the kernel arguments)

constexpr uint32_t PH_M0 = 0xD2511F53u, PH_M1 = 0xCD9E8D57u, PH_W0 = 0x9E3779B9u, PH_W1 = 0xBB67AE85u;

struct SampleArgs {
  p2r_mdn_sample_head h[P2R_MDN_SAMPLE_MAX_HEADS];
  int n[SMP_HCHUNK];
};

struct U4 { uint32_t x0, x1, x2, x3; };

__device__ __forceinline__ U4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0,
                                            uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    if (r) { k0 += PH_W0; k1 += PH_W1; }
    const uint32_t hi0 = __umulhi(PH_M0, c0), lo0 = PH_M0 * c0;
    const uint32_t hi1 = __umulhi(PH_M1, c2), lo1 = PH_M1 * c2;
    const uint32_t n0 = hi1 ^ c1 ^ k0, n2 = hi0 ^ c3 ^ k1;
    c0 = n0; c1 = lo1; c2 = n2; c3 = lo0;
  }
  return U4{c0, c1, c2, c3};
}

__device__ __forceinline__ float u24(uint32_t x) { return (float)(x >> 8) * 0x1p-24f; }
__device__ __forceinline__ double u53(uint32_t a, uint32_t b) {
  return ((double)(a >> 5) * 67108864.0 + (double)(b >> 6)) * 0x1p-53;
}

__device__ __forceinline__ void box_muller(float u1, float u2, float &na, float &nb) {
  const float r = sqrtf(-2.f * logf(1.f - u1));
  float sn, cs;
  sincospif(2.f * u2, &sn, &cs);
  na = r * cs;
  nb = r * sn;
}
__device__ __forceinline__ void box_muller(double u1, double u2, double &na, double &nb) {
  const double r = sqrt(-2.0 * log(1.0 - u1));
  double sn, cs;
  sincospi(2.0 * u2, &sn, &cs);
  na = r * cs;
  nb = r * sn;
}

// the normals of one gated draw, in the head's type
template <typename T> struct Normals;
template <> struct Normals<float> {
  __device__ static __forceinline__ void get(const U4 &x, int D, uint32_t row, uint32_t c1, uint32_t h, uint32_t k0,
                                             uint32_t k1, float (&e)[SMP_DMAX]) {
    box_muller(u24(x.x1), u24(x.x2), e[0], e[1]);
    if (D > 2) {
      const U4 y = philox4x32_10(row, c1, h, 1u, k0, k1);
      box_muller(u24(y.x0), u24(y.x1), e[2], e[3]);
    }
  }
};
template <> struct Normals<double> {
  __device__ static __forceinline__ void get(const U4 &, int D, uint32_t row, uint32_t c1, uint32_t h, uint32_t k0,
                                             uint32_t k1, double (&e)[SMP_DMAX]) {
    const U4 y = philox4x32_10(row, c1, h, 1u, k0, k1);
    box_muller(u53(y.x0, y.x1), u53(y.x2, y.x3), e[0], e[1]);
    if (D > 2) {
      const U4 z = philox4x32_10(row, c1, h, 2u, k0, k1);
      box_muller(u53(z.x0, z.x1), u53(z.x2, z.x3), e[2], e[3]);
    }
  }
};

template <typename T>
__device__ __forceinline__ void sample_body(const p2r_mdn_sample_head &H, int rows, int G, int L, int ctot, int hloc,
                                            uint32_t hstream, int n, uint32_t k0, uint32_t k1, float (*pi_s)[SMP_ROWS],
                                            T *mu_s, T *sg_s, double (*red)[SMP_SLICES][SMP_ROWS]) {
  const int tid = threadIdx.x, r = tid & (SMP_ROWS - 1), q = tid / SMP_ROWS;
  const int row0 = blockIdx.x * SMP_ROWS;
  const int D = H.D;
  for (int i = tid; i < G * SMP_ROWS; i += SMP_THREADS) {
    const int g = i / SMP_ROWS, rr = i - g * SMP_ROWS, row = row0 + rr;
    float p = 0.f;
    if (row < rows) {
      const int b = row / L, l = row - b * L;
      p = H.pi[((size_t)b * ctot + g) * L + l];
    }
    pi_s[g][rr] = p;
  }
  for (int i = tid; i < G * D; i += SMP_THREADS) {
    mu_s[i] = ((const T *)H.mu)[i];
    if (sizeof(T) == 8) sg_s[i] = (T)exp((double)H.log_sigma[i]);
    else sg_s[i] = (T)expf(H.log_sigma[i]);
  }
  __syncthreads();

  const int row = row0 + r;
  double acc[SMP_DMAX] = {0.0, 0.0, 0.0, 0.0};
  if (row < rows) {
    for (int s = q; s < n; s += SMP_SLICES) {
      for (int g = 0; g < G; ++g) {
        const uint32_t c1 = (uint32_t)g | ((uint32_t)s << 8) | ((uint32_t)H.head_id << 16);
        const U4 x = philox4x32_10((uint32_t)row, c1, hstream, 0u, k0, k1);
        if (u24(x.x0) < pi_s[g][r]) {
          T e[SMP_DMAX];
          Normals<T>::get(x, D, (uint32_t)row, c1, hstream, k0, k1, e);
#pragma unroll
          for (int d = 0; d < SMP_DMAX; ++d) {
            if (d < D) {
              const T comp = mu_s[g * D + d] + sg_s[g * D + d] * e[d];
              acc[d] += (double)comp;
            }
          }
        }
      }
    }
  }
#pragma unroll
  for (int d = 0; d < SMP_DMAX; ++d) red[d][q][r] = acc[d];
  __syncthreads();
  if (tid < SMP_ROWS * D) {                 // thread (d, r): slices added in order
    const int d = tid / SMP_ROWS, rr = tid & (SMP_ROWS - 1), orow = row0 + rr;
    double tot = 0.0;
    for (int i = 0; i < SMP_SLICES; ++i) tot += red[d][i][rr];
    if (orow < rows) ((T *)H.out)[((size_t)hloc * rows + orow) * D + d] = (T)(tot / (double)n);
  }
}

__global__ __launch_bounds__(SMP_THREADS) void mdn_sample_kernel(SampleArgs a, int rows, int G, int L, int ctot,
                                                                 int h0, int h_stream0, uint32_t k0, uint32_t k1) {
  __shared__ float pi_s[SMP_GMAX][SMP_ROWS];
  __shared__ double mu_s[SMP_GMAX * SMP_DMAX], sg_s[SMP_GMAX * SMP_DMAX];
  __shared__ double red[SMP_DMAX][SMP_SLICES][SMP_ROWS];
  const p2r_mdn_sample_head &H = a.h[blockIdx.z];
  const int hl = blockIdx.y;
  const int n = a.n[hl];
  const uint32_t hs = (uint32_t)(h_stream0 + hl);
  if (H.f64)
    sample_body<double>(H, rows, G, L, ctot, h0 + hl, hs, n, k0, k1, pi_s, mu_s, sg_s, red);
  else
    sample_body<float>(H, rows, G, L, ctot, h0 + hl, hs, n, k0, k1, pi_s, (float *)mu_s, (float *)sg_s, red);
}

// ---------------------------------------------------------------------------------------------------------------------
// Read-outs over the individual draws (p2r_mdn_sample_ex: median, draws).  The value of draw s,
//   v[s][d] = T(sum_g gate(g, s) * (mu[g, d] + sigma[g, d] * eps(g, s, d))),   components in T, the sum in double with
// g ascending, rounded once to the head's type T, depends on (seed, head_id, hypothesis, row, s, d) alone.  Thread (r, q)
// still owns samples q, q + 16, ... of row r, but leaves each v in LDS, val[d][s][r] (row innermost, as pi_s and red: the
// 16 rows of a wave's four slices land on 16 consecutive banks, and the selection below reads one address per row).
//   mean    the running sum of sample_body beside the per-draw sum: the same additions in the same order, so the same
//           bytes as mdn_sample_kernel.
//   median  rank counting: rank(s) = #{j : v_j < v_s or (v_j == v_s and j < s)} is a permutation of 0..n-1, the draw
//           of rank (n - 1) / 2 is the lower median.  Thread (r, q) ranks its own draws four at a time against all n
//           of the row (one LDS read per j, shared by the four slices of the wave); n^2 / 16 compares per thread and
//           dimension, nothing indexed dynamically in registers.  NaN orders after every number, as torch.sort has it.
//   draws   val[.][s][r] copied out (B, L, n_max, D)-contiguous, zeros for n <= s < n_max.
// LDS is carved from one dynamic array sized by the launch: red 8 KiB | pi_s [G][16] f32 | mu_s, sg_s [G][D] T |
// val [dpass][n][16] T, val at most 64 KiB: a head whose D * n * 16 values in T exceed that (f64, D > 2, n > 128)
// takes its dimensions in passes of dpass, drawing again for each.
constexpr int SMP_VAL_BYTES = 64 * 1024;
constexpr int SMP_RANK_BLOCK = 4;

struct SampleArgsEx {
  p2r_mdn_sample_head_ex h[P2R_MDN_SAMPLE_MAX_HEADS];
  int dpass[P2R_MDN_SAMPLE_MAX_HEADS];
  int n[SMP_HCHUNK];
};

template <typename T> __device__ __forceinline__ bool draw_before(T a, T b) { return a < b || (a == a && b != b); }

template <typename T>
__device__ __forceinline__ void readout_body(const p2r_mdn_sample_head_ex &H, int dpass, int rows, int G, int L,
                                             int ctot, int hloc, uint32_t hstream, int n, int n_max, int readout,
                                             uint32_t k0, uint32_t k1, unsigned char *lds) {
  const int tid = threadIdx.x, r = tid & (SMP_ROWS - 1), q = tid / SMP_ROWS;
  const int row0 = blockIdx.x * SMP_ROWS;
  const int D = H.D;
  double (*red)[SMP_SLICES][SMP_ROWS] = (double (*)[SMP_SLICES][SMP_ROWS])lds;
  float (*pi_s)[SMP_ROWS] = (float (*)[SMP_ROWS])(lds + sizeof(double) * SMP_DMAX * SMP_SLICES * SMP_ROWS);
  T *mu_s = (T *)(pi_s + G), *sg_s = mu_s + G * D, *val = sg_s + G * D;           // val[(dd * n + s) * 16 + r]
  for (int i = tid; i < G * SMP_ROWS; i += SMP_THREADS) {
    const int g = i / SMP_ROWS, rr = i - g * SMP_ROWS, row = row0 + rr;
    float p = 0.f;
    if (row < rows) {
      const int b = row / L, l = row - b * L;
      p = H.pi[((size_t)b * ctot + g) * L + l];
    }
    pi_s[g][rr] = p;
  }
  for (int i = tid; i < G * D; i += SMP_THREADS) {
    mu_s[i] = ((const T *)H.mu)[i];
    if (sizeof(T) == 8) sg_s[i] = (T)exp((double)H.log_sigma[i]);
    else sg_s[i] = (T)expf(H.log_sigma[i]);
  }
  __syncthreads();

  const int row = row0 + r;
  const size_t orow0 = (size_t)hloc * rows + row0;
  for (int d0 = 0; d0 < D; d0 += dpass) {
    const int d1 = d0 + dpass < D ? d0 + dpass : D;
    double acc[SMP_DMAX] = {0.0, 0.0, 0.0, 0.0};
    if (row < rows) {
      for (int s = q; s < n; s += SMP_SLICES) {
        double v[SMP_DMAX] = {0.0, 0.0, 0.0, 0.0};
        for (int g = 0; g < G; ++g) {
          const uint32_t c1 = (uint32_t)g | ((uint32_t)s << 8) | ((uint32_t)H.head_id << 16);
          const U4 x = philox4x32_10((uint32_t)row, c1, hstream, 0u, k0, k1);
          if (u24(x.x0) < pi_s[g][r]) {
            T e[SMP_DMAX];
            Normals<T>::get(x, D, (uint32_t)row, c1, hstream, k0, k1, e);
#pragma unroll
            for (int d = 0; d < SMP_DMAX; ++d) {
              if (d < D) {
                const T comp = mu_s[g * D + d] + sg_s[g * D + d] * e[d];
                acc[d] += (double)comp;
                v[d] += (double)comp;
              }
            }
          }
        }
#pragma unroll
        for (int d = 0; d < SMP_DMAX; ++d)
          if (d >= d0 && d < d1) val[((d - d0) * n + s) * SMP_ROWS + r] = (T)v[d];
      }
    }
    if (readout == P2R_MDN_READOUT_MEAN && d0 == 0) {
#pragma unroll
      for (int d = 0; d < SMP_DMAX; ++d) red[d][q][r] = acc[d];
    }
    __syncthreads();
    if (readout == P2R_MDN_READOUT_MEAN) {
      if (d0 == 0 && tid < SMP_ROWS * D) {    // thread (d, r): slices added in order
        const int d = tid / SMP_ROWS, rr = tid & (SMP_ROWS - 1);
        double tot = 0.0;
        for (int i = 0; i < SMP_SLICES; ++i) tot += red[d][i][rr];
        if (row0 + rr < rows) ((T *)H.out)[(orow0 + rr) * D + d] = (T)(tot / (double)n);
      }
    } else if (row < rows) {
      const int want = (n - 1) / 2;
      for (int dd = 0; dd < d1 - d0; ++dd) {
        const T *col = val + (size_t)dd * n * SMP_ROWS + r;
        for (int sb = q; sb < n; sb += SMP_SLICES * SMP_RANK_BLOCK) {
          T mine[SMP_RANK_BLOCK];
          int below[SMP_RANK_BLOCK];
#pragma unroll
          for (int i = 0; i < SMP_RANK_BLOCK; ++i) {
            const int s = sb + i * SMP_SLICES;
            mine[i] = col[(s < n ? s : sb) * SMP_ROWS];
            below[i] = 0;
          }
          for (int j = 0; j < n; ++j) {
            const T vj = col[j * SMP_ROWS];
#pragma unroll
            for (int i = 0; i < SMP_RANK_BLOCK; ++i)
              below[i] += (draw_before(vj, mine[i]) || (!draw_before(mine[i], vj) && j < sb + i * SMP_SLICES)) ? 1 : 0;
          }
#pragma unroll
          for (int i = 0; i < SMP_RANK_BLOCK; ++i)
            if (sb + i * SMP_SLICES < n && below[i] == want) ((T *)H.out)[(orow0 + r) * D + d0 + dd] = mine[i];
        }
      }
    }
    if (H.draws) {                              // (row, s, d) with d fastest: contiguous stores
      const int dn = d1 - d0, per_row = n_max * dn;
      for (int i = tid; i < SMP_ROWS * per_row; i += SMP_THREADS) {
        const int rr = i / per_row, rem = i - rr * per_row, s = rem / dn, dd = rem - s * dn;
        if (row0 + rr < rows)
          ((T *)H.draws)[((orow0 + rr) * n_max + s) * D + d0 + dd] = s < n ? val[(dd * n + s) * SMP_ROWS + rr] : (T)0;
      }
    }
    if (d1 < D) __syncthreads();                // val is drawn again for the next dimensions
  }
}

__global__ __launch_bounds__(SMP_THREADS) void mdn_readout_kernel(SampleArgsEx a, int rows, int G, int L, int ctot,
                                                                  int h0, int h_stream0, int n_max, int readout,
                                                                  uint32_t k0, uint32_t k1) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smp_lds[];
  const p2r_mdn_sample_head_ex &H = a.h[blockIdx.z];
  const int hl = blockIdx.y;
  const int n = a.n[hl];
  const uint32_t hs = (uint32_t)(h_stream0 + hl);
  if (H.f64)
    readout_body<double>(H, a.dpass[blockIdx.z], rows, G, L, ctot, h0 + hl, hs, n, n_max, readout, k0, k1, smp_lds);
  else
    readout_body<float>(H, a.dpass[blockIdx.z], rows, G, L, ctot, h0 + hl, hs, n, n_max, readout, k0, k1, smp_lds);
}

}  // namespace

extern "C" int p2r_mdn_sample_ex(int nheads, const p2r_mdn_sample_head_ex *heads, int B, int G, int L, int pi_ctot,
                                 int H, const int *n_samples, unsigned long long seed, int h_offset, int readout,
                                 int n_max, void *stream) {
  if (nheads < 1 || nheads > P2R_MDN_SAMPLE_MAX_HEADS || !heads || !n_samples || B < 0 || G < 1 || G > SMP_GMAX ||
      L < 1 || pi_ctot < G || H < 1 || h_offset < 0 || (long long)h_offset + H > 0x7fffffffLL ||
      (long long)B * L > 0x7fffffffLL || (readout != P2R_MDN_READOUT_MEAN && readout != P2R_MDN_READOUT_MEDIAN) ||
      n_max > SMP_NMAX)
    return P2R_EINVAL;
  bool any_draws = false;
  for (int i = 0; i < nheads; ++i) {
    const p2r_mdn_sample_head_ex &h = heads[i];
    if (!h.pi || !h.log_sigma || !h.mu || !h.out || h.D < 1 || h.D > SMP_DMAX || (h.f64 != 0 && h.f64 != 1) ||
        h.head_id < 0 || h.head_id > 255)
      return P2R_EINVAL;
    any_draws = any_draws || h.draws;
  }
  for (int i = 0; i < H; ++i)
    if (n_samples[i] < 1 || n_samples[i] > SMP_NMAX || (any_draws && n_samples[i] > n_max)) return P2R_EINVAL;
  if (readout == P2R_MDN_READOUT_MEAN && !any_draws) {      // nothing per draw wanted: the sampler as it was
    p2r_mdn_sample_head plain[P2R_MDN_SAMPLE_MAX_HEADS];
    for (int i = 0; i < nheads; ++i)
      plain[i] = p2r_mdn_sample_head{heads[i].pi, heads[i].log_sigma, heads[i].mu, heads[i].out, heads[i].D,
                                     heads[i].f64, heads[i].head_id};
    return p2r_mdn_sample(nheads, plain, B, G, L, pi_ctot, H, n_samples, seed, h_offset, stream);
  }
  if (B == 0) return P2R_OK;
  static unsigned char lds_ok[P2R_MAX_DEVICES];
  const hipError_t e = p2r_allow_big_lds(mdn_readout_kernel, lds_ok);
  if (e != hipSuccess) return (int)e;
  SampleArgsEx a;
  const int rows = B * L;
  const uint32_t k0 = (uint32_t)(seed & 0xffffffffull), k1 = (uint32_t)(seed >> 32);
  for (int h0 = 0; h0 < H; h0 += SMP_HCHUNK) {
    const int hc = H - h0 < SMP_HCHUNK ? H - h0 : SMP_HCHUNK;
    int nc = 1;
    for (int i = 0; i < hc; ++i) {
      a.n[i] = n_samples[h0 + i];
      nc = a.n[i] > nc ? a.n[i] : nc;
    }
    size_t lds = 0;
    for (int i = 0; i < nheads; ++i) {
      const size_t sz = heads[i].f64 ? sizeof(double) : sizeof(float);
      const int fit = (int)(SMP_VAL_BYTES / (sz * SMP_ROWS * nc));      // >= 2: 64 KiB / (8 * 16 * 256)
      a.h[i] = heads[i];
      a.dpass[i] = heads[i].D < fit ? heads[i].D : fit;
      const size_t need = sizeof(double) * SMP_DMAX * SMP_SLICES * SMP_ROWS + sizeof(float) * SMP_ROWS * G +
                          sz * (2 * (size_t)G * heads[i].D + (size_t)a.dpass[i] * nc * SMP_ROWS);
      lds = need > lds ? need : lds;
    }
    hipLaunchKernelGGL(mdn_readout_kernel, dim3((unsigned)p2r_cdiv(rows, SMP_ROWS), (unsigned)hc, (unsigned)nheads),
                       dim3(SMP_THREADS), lds, p2r_stream(stream), a, rows, G, L, pi_ctot, h0, h_offset + h0,
                       any_draws ? n_max : 0, readout, k0, k1);
    P2R_LAUNCH_CHECK();
  }
  return P2R_OK;
}

extern "C" int p2r_mdn_sample(int nheads, const p2r_mdn_sample_head *heads, int B, int G, int L, int pi_ctot, int H,
                              const int *n_samples, unsigned long long seed, int h_offset, void *stream) {
  if (nheads < 1 || nheads > P2R_MDN_SAMPLE_MAX_HEADS || !heads || !n_samples || B < 0 || G < 1 || G > SMP_GMAX ||
      L < 1 || pi_ctot < G || H < 1 || h_offset < 0 || (long long)h_offset + H > 0x7fffffffLL ||
      (long long)B * L > 0x7fffffffLL)
    return P2R_EINVAL;
  SampleArgs a;
  for (int i = 0; i < nheads; ++i) {
    const p2r_mdn_sample_head &h = heads[i];
    if (!h.pi || !h.log_sigma || !h.mu || !h.out || h.D < 1 || h.D > SMP_DMAX || (h.f64 != 0 && h.f64 != 1) ||
        h.head_id < 0 || h.head_id > 255)
      return P2R_EINVAL;
    a.h[i] = h;
  }
  for (int i = 0; i < H; ++i)
    if (n_samples[i] < 1 || n_samples[i] > SMP_NMAX) return P2R_EINVAL;
  if (B == 0) return P2R_OK;
  const int rows = B * L;
  const uint32_t k0 = (uint32_t)(seed & 0xffffffffull), k1 = (uint32_t)(seed >> 32);
  for (int h0 = 0; h0 < H; h0 += SMP_HCHUNK) {
    const int hc = H - h0 < SMP_HCHUNK ? H - h0 : SMP_HCHUNK;
    for (int i = 0; i < hc; ++i) a.n[i] = n_samples[h0 + i];
    hipLaunchKernelGGL(mdn_sample_kernel, dim3((unsigned)p2r_cdiv(rows, SMP_ROWS), (unsigned)hc, (unsigned)nheads),
                       dim3(SMP_THREADS), 0, p2r_stream(stream), a, rows, G, L, pi_ctot, h0, h_offset + h0, k0, k1);
    P2R_LAUNCH_CHECK();
  }
  return P2R_OK;
}
