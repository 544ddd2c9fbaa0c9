// ap_eval.hip -- detection AP on the device for gfx950: oriented-box IoU of every (detection, ground truth) pair
// and the greedy matching of the VOC metric, fp64 like the reference.
//
// Replaces, for the device-resident calculator (net_utils/ap_device.py), the per-class pair lists of
// net_utils/eval_det.py (`_pair_ious`: one ~40-op tensor pass per class, threshold and hypothesis) and the Python
// sweep over the sorted detections (`eval_det_cls_wo_mesh`, reference eval_det.py:259-343).  The IoU of proposal k
// with ground truth g depends neither on the class nor on the threshold: it is computed once per batch
// (p2r_obb_iou), and one launch of p2r_ap_match turns it into true-positive flags for all classes and thresholds.
//
// All arithmetic is IEEE fp64 in the operation order of net_utils/box_util.py with contraction off (the strict
// `inside` predicate must not see fused products).  Every loop is bounded at compile time or by a checked size, so
// NaN and degenerate boxes cannot make a lane loop or write outside its own slots.
#include "p2r_common.h"
#include "obb_iou_body.h"

#include "../../include/p2r_ap_eval.h"

namespace {

// ---- p2r_obb_iou ---------------------------------------------------------------------------------------------------------
// The per-pair body (clip, shoelace, height overlap, volumes) lives in obb_iou_body.h, shared with consensus.hip.
constexpr int IOU_LANES = 64;   // one wave per workgroup
constexpr int IOU_MAXK = 1024;
constexpr int IOU_MAXG = 256;

__global__ __launch_bounds__(IOU_LANES) void obb_iou_kernel(int P, int K, int G, const double *__restrict__ det,
                                                            const double *__restrict__ gt,
                                                            double *__restrict__ iou3d, double *__restrict__ iou2d) {
  __shared__ double s_v[2][IOU_CAP][2][IOU_LANES];   // 32 KiB: the two vertex buffers of the clip, one column per lane
  const int lane = threadIdx.x;
  const long long p = (long long)blockIdx.x * IOU_LANES + lane;
  if (p >= P) return;   // no barrier below: lanes are independent
  const int g = (int)(p % G);
  const long long bk = p / G;   // b * K + k
  const long long b = bk / K;
  ObbFoot f1, f2;   // subject = detection footprint, clip = ground-truth footprint
  obb_foot_load(det + bk * 24, f1);
  obb_foot_load(gt + (b * G + g) * 24, f2);
  double i2;
  iou3d[p] = obb_pair_iou<IOU_LANES>(f1, f2, s_v, lane, i2);
  if (iou2d) iou2d[p] = i2;
}

// ---- p2r_ap_match -------------------------------------------------------------------------------------------------------
constexpr int APM_MAXK = 1024;
constexpr int APM_MAXG = 256;
constexpr int APM_MAXC = 64;
constexpr int APM_MAXT = 8;

// One workgroup per (scan, class), one thread per proposal.
__global__ __launch_bounds__(APM_MAXK) void ap_match_kernel(
    int K, int G, int C, int T, const double *__restrict__ iou, const float *__restrict__ score,
    const unsigned char *__restrict__ valid, const long long *__restrict__ gt_cls,
    const unsigned char *__restrict__ gt_mask, const double *__restrict__ thr, unsigned char *__restrict__ tp,
    int *__restrict__ npos) {
  __shared__ double s_biou[APM_MAXK];          // IoU with the best ground truth
  __shared__ float s_score[APM_MAXK];
  __shared__ int s_best[APM_MAXK];             // best ground truth; -1: none; -2: not a detection
  __shared__ unsigned char s_gsel[APM_MAXG];   // ground truth g is unmasked and of this class
  __shared__ double s_thr[APM_MAXT];
  const int n = blockIdx.x, c = blockIdx.y, N = gridDim.x;
  const int t = threadIdx.x;

  for (int g = t; g < G; g += blockDim.x) {
    const size_t o = (size_t)n * G + g;
    s_gsel[g] = (gt_mask[o] != 0 && gt_cls[o] == (long long)c) ? 1 : 0;
  }
  if (t < APM_MAXT) s_thr[t] = t < T ? thr[t] : 0.0;
  __syncthreads();
  if (t == 0) {
    int cnt = 0;
    for (int g = 0; g < G; ++g) cnt += s_gsel[g];
    npos[(size_t)n * C + c] = cnt;
  }

  bool det = false;
  float sc = 0.f;
  double bi = -__builtin_inf();
  int jb = -1;
  if (t < K) {
    const size_t o = ((size_t)n * K + t) * C + c;
    det = valid[o] != 0;
    if (det) {
      sc = score[o];
      const double *row = iou + ((size_t)n * K + t) * G;
      for (int g = 0; g < G; ++g) {
        if (s_gsel[g]) {
          const double ov = row[g];
          if (ov > bi) {   // strict: the first index wins on equal IoU, NaN never wins
            bi = ov;
            jb = g;
          }
        }
      }
    }
    s_score[t] = sc;
    s_biou[t] = bi;
    s_best[t] = det ? jb : -2;
  }
  __syncthreads();

  // bit q: an earlier-ranked detection with the same best ground truth exceeds thr[q], i.e. has taken it
  unsigned claimed = 0;
  if (det && jb >= 0) {
    for (int u = 0; u < K; ++u) {
      if (s_best[u] != jb) continue;
      const float su = s_score[u];
      if (su > sc || (su == sc && u < t)) {
        const double bu = s_biou[u];
#pragma unroll
        for (int q = 0; q < APM_MAXT; ++q) claimed |= (bu > s_thr[q]) ? (1u << q) : 0u;
      }
    }
  }
  if (t < K) {
#pragma unroll
    for (int q = 0; q < APM_MAXT; ++q) {
      if (q < T) {
        const bool hit = jb >= 0 && bi > s_thr[q] && !((claimed >> q) & 1u);
        tp[(((size_t)q * N + n) * K + t) * C + c] = det ? (hit ? 1 : 0) : 255;
      }
    }
  }
}

}  // namespace

extern "C" int p2r_obb_iou(int B, int K, int G, const double *det, const double *gt, double *iou3d, double *iou2d,
                           void *stream) {
  if (B < 0 || K < 0 || G < 0 || K > IOU_MAXK || G > IOU_MAXG) return P2R_EINVAL;
  const long long P = (long long)B * K * G;
  if (P > 0x7fffffffLL) return P2R_EINVAL;
  if (P == 0) return P2R_OK;
  hipLaunchKernelGGL(obb_iou_kernel, dim3(p2r_cdiv(P, IOU_LANES)), dim3(IOU_LANES), 0, p2r_stream(stream), (int)P, K,
                     G, det, gt, iou3d, iou2d);
  P2R_LAUNCH_CHECK();
  return P2R_OK;
}

extern "C" int p2r_ap_match(int N, int K, int G, int C, int T, const double *iou3d, const float *score,
                            const unsigned char *valid, const long long *gt_cls, const unsigned char *gt_mask,
                            const double *thr, unsigned char *tp, int *npos, void *stream) {
  if (N < 0 || K < 0 || G < 0 || C < 0 || T < 0 || K > APM_MAXK || G > APM_MAXG || C > APM_MAXC || T > APM_MAXT)
    return P2R_EINVAL;
  if (N == 0 || C == 0) return P2R_OK;
  // K = 0 and T = 0 still launch: npos is an output of every (scan, class)
  const int threads = K > 0 ? ((K + 63) / 64) * 64 : 64;
  hipLaunchKernelGGL(ap_match_kernel, dim3(N, C), dim3(threads), 0, p2r_stream(stream), K, G, C, T, iou3d, score,
                     valid, gt_cls, gt_mask, thr, tp, npos);
  P2R_LAUNCH_CHECK();
  return P2R_OK;
}
