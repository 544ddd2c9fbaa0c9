// obb_iou_body.h -- the oriented-box IoU of one pair of boxes, one pair per lane: the body of obb_iou_kernel
// (ap_eval.hip), shared with the consensus clustering (consensus.hip) so that both evaluate the same arithmetic.
//
// All arithmetic is IEEE fp64 in the operation order of net_utils/box_util.py with contraction off (the strict
// `inside` predicate must not see fused products).  Every loop is bounded at compile time, so NaN and degenerate boxes
// cannot make a lane loop or write outside its own slots.  No barrier: lanes are independent.
#pragma once
#include "p2r_common.h"

constexpr int IOU_CAP = 16;     // vertex slots per polygon (_CAP of box_util.py; a convex quad clipped by four
                                // half-planes has <= 8 vertices, the slack absorbs rounding artefacts)

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

// What the pair body reads of one box: the footprint (corners 3,2,6,7 on (x, z), counter-clockwise for any heading), the
// height of corner 7 (top) and corner 4 (bottom), and the volume from three edge lengths.
struct ObbFoot {
  double x[4], y[4];
  double top, bottom, vol;
};

// c: the 8 corners (24 doubles) in the get_box_corners order
__device__ __forceinline__ void obb_foot_load(const double *c, ObbFoot &f) {
  constexpr int FOOT[4] = {3, 2, 6, 7};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    f.x[i] = c[FOOT[i] * 3 + 0];
    f.y[i] = c[FOOT[i] * 3 + 2];
  }
  f.top = c[7 * 3 + 1];
  f.bottom = c[4 * 3 + 1];
  f.vol = iou_edge(c + 21, c + 18) * iou_edge(c + 18, c + 6) * iou_edge(c + 21, c + 12);
}

// -> IoU in 3D of box a (the subject of the clip) and box b (the clip polygon); iou2d: the IoU of the footprints (a
// caller that drops it pays nothing: the function is inlined).  s_v: the two vertex buffers of the clip in LDS, one
// column per lane: lane l touches only [..][..][..][l], consecutive lanes are consecutive 8-byte words (no bank
// conflict), and a slot index is checked against IOU_CAP before every store.  A private array indexed by the running
// vertex count would live in scratch.
template <int LANES>
__device__ __forceinline__ double obb_pair_iou(const ObbFoot &a, const ObbFoot &b, double (&s_v)[2][IOU_CAP][2][LANES],
                                               int lane, double &iou2d) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    s_v[0][i][0][lane] = a.x[i];
    s_v[0][i][1][lane] = a.y[i];
  }

  // Sutherland-Hodgman (box_util.py:22-69): subject = footprint of a, clip = footprint of b
  int cnt = 4;
  double cp1x = b.x[3], cp1y = b.y[3];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int cur = j & 1, nxt = cur ^ 1;
    const double cp2x = b.x[j], cp2y = b.y[j];
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

  const double a1 = iou_quad_area(a.x, a.y), a2 = iou_quad_area(b.x, b.y);
  iou2d = inter / (a1 + a2 - inter);
  const double ymax = iou_min(a.top, b.top);
  const double ymin = iou_max(a.bottom, b.bottom);
  const double h = iou_max(ymax - ymin, 0.0);
  const double inter_vol = inter * h;
  return inter_vol / (a.vol + b.vol - inter_vol);
}
