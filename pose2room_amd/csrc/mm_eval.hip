// mm_eval.hip -- multi-modal evaluation on the device for gfx950: the dump records' box parameters and the TMD
// diversity value of every (sample, proposal) over the hypotheses, fp64 like the host code.
//
// Replaces, for the device-resident evaluator (net_utils/mm_device.py), the per-sample NumPy pass of
// multi_modal_eval.corners_to_params and the Python dict walk of multi_modal_eval.tmd over every
// (sample, proposal, run).  Both kernels are a handful of microseconds of work: they are bound by launch and memory
// latency, not by arithmetic or bandwidth.
//
// All arithmetic is IEEE fp64 in the operation order of net_utils/multi_modal_eval.py with contraction off.  Every
// loop is bounded at compile time, so NaN and degenerate boxes are ordinary data.  No atomics: each output element has
// one writer, partial sums meet in a fixed xor-butterfly, so two runs give identical bits.
#include "p2r_common.h"

#include "../../include/p2r_mm_eval.h"

namespace {

// ---- p2r_box_params ------------------------------------------------------------------------------------------------------
constexpr int BP_THREADS = 256;

// np.max / np.min keep NaN; fmax / fmin would drop it
__device__ __forceinline__ double bp_min(double a, double b) { return (a < b || a != a) ? a : b; }
__device__ __forceinline__ double bp_max(double a, double b) { return (a > b || a != a) ? a : b; }

__global__ __launch_bounds__(BP_THREADS) void box_params_kernel(int N, const double *__restrict__ corners,
                                                                double *__restrict__ obbs) {
  const long long i = (long long)blockIdx.x * BP_THREADS + threadIdx.x;
  if (i >= N) return;
  const double *c = corners + i * 24;
  double *o = obbs + i * 7;
  double v[3][3];
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    double lo = c[d], hi = c[d];
#pragma unroll
    for (int q = 1; q < 8; ++q) {
      lo = bp_min(lo, c[q * 3 + d]);
      hi = bp_max(hi, c[q * 3 + d]);
    }
    o[d] = (hi + lo) / 2.;
    v[0][d] = (c[1 * 3 + d] - c[0 * 3 + d]) / 2.;
    v[1][d] = (c[2 * 3 + d] - c[1 * 3 + d]) / 2.;
    v[2][d] = (c[4 * 3 + d] - c[0 * 3 + d]) / 2.;
  }
  double R[3][3];
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    const double size = sqrt(v[r][0] * v[r][0] + v[r][1] * v[r][1] + v[r][2] * v[r][2]) * 2;
    o[3 + r] = size;
    const double inv = 1 / (size / 2);
#pragma unroll
    for (int d = 0; d < 3; ++d) R[r][d] = inv * v[r][d];
  }
  if (R[1][1] < 0) {
#pragma unroll
    for (int d = 0; d < 3; ++d) R[1][d] *= -1;
  }
  // np.cross(R0, R1) . R2; only its sign is used, and only row 2 depends on it -- the heading reads row 0
  const double x0 = R[0][1] * R[1][2] - R[0][2] * R[1][1];
  const double x1 = R[0][2] * R[1][0] - R[0][0] * R[1][2];
  const double x2 = R[0][0] * R[1][1] - R[0][1] * R[1][0];
  if (x0 * R[2][0] + x1 * R[2][1] + x2 * R[2][2] < 0) {
#pragma unroll
    for (int d = 0; d < 3; ++d) R[2][d] *= -1;
  }
  o[6] = atan2(-R[0][2], R[0][0]);
}

// ---- p2r_tmd ----------------------------------------------------------------------------------------------------------------
constexpr int TMD_MAXH = 64;    // one lane per hypothesis
constexpr int TMD_MAXK = 1024;
constexpr int TMD_ROW = 25;     // 24 corner coordinates + 1: an odd stride in 8-byte words spreads rows over the banks

// every lane gets the total; lane l adds its partner's value to its own at every level, so all lanes hold the same bits
__device__ __forceinline__ double tmd_wave_sum(double v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, P2R_WAVE);
  return v;
}

// One wave (one workgroup) per (sample, proposal).
__global__ __launch_bounds__(P2R_WAVE) void tmd_kernel(int H, int BK, const double *__restrict__ obbs,
                                                       const unsigned char *__restrict__ keep,
                                                       const long long *__restrict__ cls, double *__restrict__ value,
                                                       int *__restrict__ count) {
  __shared__ double s_c[TMD_MAXH][TMD_ROW];   // corners of the kept boxes, compacted in ascending h
  __shared__ long long s_cls[TMD_MAXH];
  const int lane = threadIdx.x;
  const int cell = blockIdx.x;   // b * K + k
  bool kept = false;
  size_t src = 0;
  if (lane < H) {
    src = (size_t)lane * BK + cell;
    kept = keep[src] != 0;
  }
  const unsigned long long mask = __ballot(kept);
  const int n = __popcll(mask);
  if (n == 0) {   // wave-uniform
    if (lane == 0) {
      value[cell] = 0.0;
      count[cell] = 0;
    }
    return;
  }
  if (kept) {
    const int r = __popcll(mask & ((1ull << lane) - 1ull));
    const double *p = obbs + src * 7;
    // multi_modal_eval.params_to_corners: vectors = (size / 2) * R, R rows (cos, 0, -sin), (0, 1, 0), (sin, 0, cos)
    const double ch = cos(p[6]), sh = sin(p[6]);
    const double h0 = p[3] / 2., h1 = p[4] / 2., h2 = p[5] / 2.;
    const double vec[3][3] = {{h0 * ch, h0 * 0.0, h0 * -sh}, {h1 * 0.0, h1 * 1.0, h1 * 0.0}, {h2 * sh, h2 * 0.0, h2 * ch}};
    constexpr double SG[8][3] = {{-1, -1, -1}, {1, -1, -1}, {1, 1, -1}, {-1, 1, -1},
                                 {-1, -1, 1},  {1, -1, 1},  {1, 1, 1},  {-1, 1, 1}};   // get_box_corners
#pragma unroll
    for (int q = 0; q < 8; ++q) {
#pragma unroll
      for (int d = 0; d < 3; ++d)
        s_c[r][q * 3 + d] = ((p[d] + SG[q][0] * vec[0][d]) + SG[q][1] * vec[1][d]) + SG[q][2] * vec[2][d];
    }
    s_cls[r] = cls[src];
  }
  __syncthreads();

  // shape: the n * n ordered pairs strided over the lanes, each lane's partial sum in ascending pair index
  const int nn = n * n;
  double acc = 0.0;
  for (int it = 0; it < TMD_MAXH; ++it) {
    if (it * P2R_WAVE >= nn) break;   // wave-uniform
    const int pr = it * P2R_WAVE + lane;
    if (pr < nn) {
      const int i = pr / n, j = pr - i * n;
      double dist[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        const double dx = s_c[i][q * 3 + 0] - s_c[j][q * 3 + 0];
        const double dy = s_c[i][q * 3 + 1] - s_c[j][q * 3 + 1];
        const double dz = s_c[i][q * 3 + 2] - s_c[j][q * 3 + 2];
        dist[q] = sqrt(dx * dx + dy * dy + dz * dz);
      }
      // np.mean over 8 contiguous elements: NumPy's pairwise tree
      acc += (((dist[0] + dist[1]) + (dist[2] + dist[3])) + ((dist[4] + dist[5]) + (dist[6] + dist[7]))) / 8.0;
    }
  }
  const double shape = tmd_wave_sum(acc) / (double)n;

  // entropy: the first kept entry of every distinct label contributes p ln p
  double term = 0.0;
  if (lane < n) {
    const long long mine = s_cls[lane];
    int same = 0;
    bool first = true;
    for (int j = 0; j < TMD_MAXH; ++j) {
      if (j < n) {
        const bool eq = s_cls[j] == mine;
        same += eq ? 1 : 0;
        first = first && !(eq && j < lane);
      }
    }
    if (first) {
      const double pc = (double)same / (double)n;
      term = pc * log(pc);
    }
  }
  const double entropy = -tmd_wave_sum(term) / log(2.0);
  if (lane == 0) {
    value[cell] = (entropy + 1.0) * (shape + 1.0);
    count[cell] = n;
  }
}

}  // namespace

extern "C" int p2r_box_params(int N, const double *corners, double *obbs, void *stream) {
  if (N < 0) return P2R_EINVAL;
  if (N == 0) return P2R_OK;
  hipLaunchKernelGGL(box_params_kernel, dim3(p2r_cdiv(N, BP_THREADS)), dim3(BP_THREADS), 0, p2r_stream(stream), N,
                     corners, obbs);
  P2R_LAUNCH_CHECK();
  return P2R_OK;
}

extern "C" int p2r_tmd(int H, int B, int K, const double *obbs, const unsigned char *keep, const long long *cls,
                       double *value, int *count, void *stream) {
  if (H < 1 || H > TMD_MAXH || B < 0 || K < 0 || K > TMD_MAXK) return P2R_EINVAL;
  const long long BK = (long long)B * K;
  if (BK > 0x7fffffffLL) return P2R_EINVAL;
  if (BK == 0) return P2R_OK;
  hipLaunchKernelGGL(tmd_kernel, dim3((unsigned)BK), dim3(P2R_WAVE), 0, p2r_stream(stream), H, (int)BK, obbs, keep,
                     cls, value, count);
  P2R_LAUNCH_CHECK();
  return P2R_OK;
}
