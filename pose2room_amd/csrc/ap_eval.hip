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

#include "../../include/p2r_ap_eval.h"

namespace {

// ---- p2r_obb_iou ---------------------------------------------------------------------------------------------------------
constexpr int IOU_LANES = 64;   // one wave per workgroup
constexpr int IOU_CAP = 16;     // vertex slots per polygon (_CAP of box_util.py; a convex quad clipped by four
                                // half-planes has <= 8 vertices, the slack absorbs rounding artefacts)
constexpr int IOU_MAXK = 1024;
constexpr int IOU_MAXG = 256;

// box_util.py:37-38: p strictly left of the directed clip edge cp1 -> cp2
__device__ __forceinline__ bool iou_inside(double c1x, double c1y, double c2x, double c2y, double px, double py) {
  return (c2x - c1x) * (py - c1y) > (c2y - c1y) * (px - c1x);
}

// torch.minimum / torch.maximum / clamp(min=0) keep NaN; fmin / fmax would drop it
__device__ __forceinline__ double iou_min(double a, double b) { return (a < b || a != a) ? a : b; }
__device__ __forceinline__ double iou_max(double a, double b) { return (a > b || a != a) ? a : b; }

// box_util.py:83-88 on corners 7,6,2,4: |c7-c6| |c6-c2| |c7-c4|
__device__ __forceinline__ double iou_edge(const double *a, const double *b) {
  const double dx = a[0] - b[0], dy = a[1] - b[1], dz = a[2] - b[2];
  return sqrt(dx * dx + dy * dy + dz * dz);
}

// shoelace on a quad (box_util.py:17-20): 0.5 |sum x_i y_{i-1} - sum y_i x_{i-1}|
__device__ __forceinline__ double iou_quad_area(const double (&x)[4], const double (&y)[4]) {
  const double a = x[0] * y[3] + x[1] * y[0] + x[2] * y[1] + x[3] * y[2];
  const double b = y[0] * x[3] + y[1] * x[0] + y[2] * x[1] + y[3] * x[2];
  return 0.5 * fabs(a - b);
}

__global__ __launch_bounds__(IOU_LANES) void obb_iou_kernel(int P, int K, int G, const double *__restrict__ det,
                                                            const double *__restrict__ gt,
                                                            double *__restrict__ iou3d, double *__restrict__ iou2d) {
  // the two vertex buffers of the clip, one column per lane: lane l touches only [..][..][..][l], consecutive lanes
  // are consecutive 8-byte words (no bank conflict), and a slot index is checked against IOU_CAP before every store.
  // A private array indexed by the running vertex count would live in scratch.
  __shared__ double s_v[2][IOU_CAP][2][IOU_LANES];   // 32 KiB
  const int lane = threadIdx.x;
  const long long p = (long long)blockIdx.x * IOU_LANES + lane;
  if (p >= P) return;   // no barrier below: lanes are independent
  const int g = (int)(p % G);
  const long long bk = p / G;   // b * K + k
  const long long b = bk / K;
  const double *c1 = det + bk * 24;
  const double *c2 = gt + (b * G + g) * 24;

  constexpr int FOOT[4] = {3, 2, 6, 7};   // counter-clockwise on (x, z) for any heading
  double q1x[4], q1y[4], q2x[4], q2y[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    q1x[i] = c1[FOOT[i] * 3 + 0];
    q1y[i] = c1[FOOT[i] * 3 + 2];
    q2x[i] = c2[FOOT[i] * 3 + 0];
    q2y[i] = c2[FOOT[i] * 3 + 2];
    s_v[0][i][0][lane] = q1x[i];
    s_v[0][i][1][lane] = q1y[i];
  }

  // Sutherland-Hodgman (box_util.py:22-69): subject = detection footprint, clip = ground-truth footprint
  int cnt = 4;
  double cp1x = q2x[3], cp1y = q2y[3];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int cur = j & 1, nxt = cur ^ 1;
    const double cp2x = q2x[j], cp2y = q2y[j];
    const int last = cnt > 0 ? cnt - 1 : 0;
    double sx = s_v[cur][last][0][lane], sy = s_v[cur][last][1][lane];
    int n = 0;   // vertices emitted; only the first IOU_CAP are stored
    for (int i = 0; i < IOU_CAP; ++i) {
      if (i < cnt) {
        const double ex = s_v[cur][i][0][lane], ey = s_v[cur][i][1][lane];
        const bool in_e = iou_inside(cp1x, cp1y, cp2x, cp2y, ex, ey);
        const bool in_s = iou_inside(cp1x, cp1y, cp2x, cp2y, sx, sy);
        if (in_e != in_s) {   // the edge s -> e crosses the clip line (box_util.py:40-46)
          const double dcx = cp1x - cp2x, dcy = cp1y - cp2y;
          const double dpx = sx - ex, dpy = sy - ey;
          const double n1 = cp1x * cp2y - cp1y * cp2x;
          const double n2 = sx * ey - sy * ex;
          const double n3 = 1.0 / (dcx * dpy - dcy * dpx);
          if (n < IOU_CAP) {
            s_v[nxt][n][0][lane] = (n1 * dpx - n2 * dcx) * n3;
            s_v[nxt][n][1][lane] = (n1 * dpy - n2 * dcy) * n3;
          }
          ++n;
        }
        if (in_e) {
          if (n < IOU_CAP) {
            s_v[nxt][n][0][lane] = ex;
            s_v[nxt][n][1][lane] = ey;
          }
          ++n;
        }
        sx = ex;
        sy = ey;
      }
    }
    cnt = n < IOU_CAP ? n : IOU_CAP;
    cp1x = cp2x;
    cp1y = cp2y;
  }

  // shoelace over the cnt vertices left in buffer 0 (four passes: 0 -> 1 -> 0 -> 1 -> 0)
  double inter = 0.0;
  if (cnt >= 3) {
    const double x0 = s_v[0][0][0][lane], y0 = s_v[0][0][1][lane];
    double xi = x0, yi = y0, acc = 0.0;
    for (int i = 0; i < IOU_CAP; ++i) {
      if (i < cnt) {
        const bool wrap = i + 1 >= cnt;
        const int i1 = wrap ? 0 : i + 1;
        const double xn = s_v[0][i1][0][lane], yn = s_v[0][i1][1][lane];
        acc += xi * yn - yi * xn;
        xi = xn;
        yi = yn;
      }
    }
    inter = 0.5 * fabs(acc);
  }

  const double a1 = iou_quad_area(q1x, q1y), a2 = iou_quad_area(q2x, q2y);
  if (iou2d) iou2d[p] = inter / (a1 + a2 - inter);
  const double ymax = iou_min(c1[7 * 3 + 1], c2[7 * 3 + 1]);
  const double ymin = iou_max(c1[4 * 3 + 1], c2[4 * 3 + 1]);
  const double h = iou_max(ymax - ymin, 0.0);
  const double inter_vol = inter * h;
  const double v1 = iou_edge(c1 + 21, c1 + 18) * iou_edge(c1 + 18, c1 + 6) * iou_edge(c1 + 21, c1 + 12);
  const double v2 = iou_edge(c2 + 21, c2 + 18) * iou_edge(c2 + 18, c2 + 6) * iou_edge(c2 + 21, c2 + 12);
  iou3d[p] = inter_vol / (v1 + v2 - inter_vol);
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
