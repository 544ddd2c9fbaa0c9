// parse_boxes.hip -- prediction parsing up to the NMS in one launch (include/p2r_parse.h: p2r_parse_boxes).
// net_utils/ap_helper.py::parse_predictions does this with several dozen ATen launches in float64; its far-box filter
// materialises three (N, K, T, 3) f64 tensors for one bit per box.  Here one workgroup owns one sample and PB = 16
// consecutive proposals:
//   1. lanes 0..15 each form one box: size, heading, corners, AABB, NMS row, objectness probability, class.  A few
//      dozen flops and ~300 bytes of plain stores per box; the box frame the scan needs (centre, c, s, enlarged
//      half-extents) goes to an LDS table.
//   2. the far-box scan, N * K * T point tests, is the only real work.  The positions of joint `origin_joint` sit 12 * J
//      bytes apart in HBM (636 at 53 joints), one cache line per frame, so they are fetched once per workgroup, one frame
//      per thread, and staged into LDS as three float arrays in chunks of CH = 256 frames.  Each of the four waves owns
//      four of the boxes; its lanes stride over the frames of the chunk (conflict-free dword reads) against a box frame
//      read from LDS at a uniform address.  The loads of chunk i + 1 are in flight while chunk i is tested.
//   3. after each chunk a ballot per box says whether the box has found a frame; a wave whose boxes are all decided
//      skips the tests, and when all four waves say so (four LDS flags read after the barrier that the restaging needs
//      anyway) the workgroup leaves the loop: a workgroup-uniform branch.  Every loop is bounded by T, K or C.
// LDS: 3 KB of positions + 1 KB of box frames + flags, independent of T.  No atomics, no scratch buffer.
// Why 16 boxes: at B = 32, K = 128 that is 256 workgroups, one per CU; every workgroup of a sample fetches the sample's
// T lines again (from L2 after the first), so fewer boxes per workgroup would multiply that traffic and more would leave
// CUs idle at the batch size the evaluation runs.  DESIGN.md has the measurements.
#include "p2r_common.h"

#include "../../include/p2r_parse.h"

namespace {

constexpr int PB_THREADS = 256;
constexpr int PB_WAVES = PB_THREADS / P2R_WAVE;
constexpr int PB = 16;                        // proposals per workgroup
constexpr int PB_PER_WAVE = PB / PB_WAVES;    // 4
constexpr int CH = PB_THREADS;                // frames per chunk: one per thread
constexpr int CH_STEPS = CH / P2R_WAVE;       // 4 frames per lane and chunk
constexpr int FR = 8;                         // doubles of a box frame: centre (3), c, s, hf (3)

enum { DECIDED_EMPTY = 0, DECIDED_NONEMPTY = 1, NEEDS_SCAN = 2 };

// torch.min / torch.max over a dimension keep a NaN
__device__ __forceinline__ double min_nan(double m, double v) { return (v < m || v != v) ? v : m; }
__device__ __forceinline__ double max_nan(double m, double v) { return (v > m || v != v) ? v : m; }

// One box: every output but `nonempty`; its frame into fr[0..7]; -> whether its sizes pass the bounds.
__device__ __forceinline__ bool form_box(long long b, int C, const float *__restrict__ center,
                                         const float *__restrict__ size_log, const double *__restrict__ heading_sc,
                                         const float *__restrict__ objectness, const float *__restrict__ sem_scores,
                                         const long long *__restrict__ cls_in, float contact, int nms_mode,
                                         double *__restrict__ corners, double *__restrict__ boxes,
                                         float *__restrict__ obj_prob, long long *__restrict__ pred_cls, double *fr) {
  float size[3], halff[3];
  double ctr[3], half[3];
  bool ok = true;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    size[a] = expf(size_log[b * 3 + a]);
    halff[a] = size[a] / 2.0f;
    half[a] = (double)halff[a];
    ctr[a] = (double)center[b * 3 + a];
    ok = ok && !(size[a] < 0.01f) && !(size[a] > 10.0f);
  }
  const double theta = atan2(heading_sc[b * 2], heading_sc[b * 2 + 1]);
  const double c = cos(theta), s = sin(theta);
  const double R[3][3] = {{c, 0.0, -s}, {0.0, 1.0, 0.0}, {s, 0.0, c}};
  double v[3][3];      // row i = half_i * R_i
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) v[i][j] = half[i] * R[i][j];

  double mn[3], mx[3];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    // corner order of get_box_corners: signs of (v0, v1, v2)
    const double g0 = ((i & 3) == 1 || (i & 3) == 2) ? 1.0 : -1.0;
    const double g1 = (i & 2) ? 1.0 : -1.0;
    const double g2 = (i & 4) ? 1.0 : -1.0;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const double x = ((ctr[j] + g0 * v[0][j]) + g1 * v[1][j]) + g2 * v[2][j];
      corners[b * 24 + i * 3 + j] = x;
      mn[j] = i == 0 ? x : min_nan(mn[j], x);
      mx[j] = i == 0 ? x : max_nan(mx[j], x);
    }
  }

  const float l0 = objectness[b * 2], l1 = objectness[b * 2 + 1];
  const float m = (l1 > l0 || l1 != l1) ? l1 : l0;
  const float e0 = expf(l0 - m), e1 = expf(l1 - m);
  const float prob = e1 / (e0 + e1);
  obj_prob[b] = prob;

  long long cls;
  if (cls_in) {
    cls = cls_in[b];
  } else {
    int best = 0;
    float bx = sem_scores[b * C];
    for (int k = 1; k < C; ++k) {
      const float x = sem_scores[b * C + k];
      if (x > bx || (x != x && bx == bx)) best = k, bx = x;
    }
    cls = best;
  }
  pred_cls[b] = cls;

  const double score = (double)prob;
  if (nms_mode == 2) {
    double *row = boxes + b * 7;
    row[0] = mn[0], row[1] = 0.0, row[2] = mn[2], row[3] = mx[0], row[4] = 1.0, row[5] = mx[2], row[6] = score;
  } else {
    double *row = boxes + b * (nms_mode == 1 ? 8 : 7);
    row[0] = mn[0], row[1] = mn[1], row[2] = mn[2], row[3] = mx[0], row[4] = mx[1], row[5] = mx[2], row[6] = score;
    if (nms_mode == 1) row[7] = (double)cls;
  }

  fr[0] = ctr[0], fr[1] = ctr[1], fr[2] = ctr[2], fr[3] = c, fr[4] = s;
#pragma unroll
  for (int a = 0; a < 3; ++a) fr[5 + a] = (double)(halff[a] + contact);
  return ok;
}

__global__ __launch_bounds__(PB_THREADS) void parse_boxes_kernel(
    const float *__restrict__ center, const float *__restrict__ size_log, const double *__restrict__ heading_sc,
    const float *__restrict__ objectness, const float *__restrict__ sem_scores, const long long *__restrict__ cls_in,
    const float *__restrict__ joints, int K, int C, int Bj, int T, int J, int origin_joint, float contact,
    int remove_far_box, int nms_mode, int groups, double *__restrict__ corners, double *__restrict__ boxes,
    float *__restrict__ obj_prob, long long *__restrict__ pred_cls, unsigned char *__restrict__ nonempty) {
  __shared__ float lds_p[3][CH];
  __shared__ double lds_fr[PB][FR];
  __shared__ int lds_state[PB];
  __shared__ int lds_done[PB_WAVES];

  const int tid = threadIdx.x, lane = tid & (P2R_WAVE - 1), wave = tid / P2R_WAVE;
  const int n = blockIdx.x / groups, k0 = (blockIdx.x % groups) * PB;

  if (tid < PB) {
    int state = DECIDED_EMPTY;
    if (k0 + tid < K) {
      const bool ok = form_box((long long)n * K + k0 + tid, C, center, size_log, heading_sc, objectness, sem_scores,
                               cls_in, contact, nms_mode, corners, boxes, obj_prob, pred_cls, lds_fr[tid]);
      state = !remove_far_box ? DECIDED_NONEMPTY : (ok ? NEEDS_SCAN : DECIDED_EMPTY);
    }
    lds_state[tid] = state;
  }

  // the positions this thread stages: frame t0 + tid of joints row n % Bj
  const float *hip = nullptr;
  float p[3] = {0.0f, 0.0f, 0.0f};
  if (remove_far_box) {
    hip = joints + (((long long)(n % Bj) * T) * J + origin_joint) * 3;
    if (tid < T) {
#pragma unroll
      for (int a = 0; a < 3; ++a) p[a] = hip[(long long)tid * J * 3 + a];
    }
  }
  __syncthreads();

  // bit q: box wave * 4 + q still looks for a frame / has found one; uniform over the wave
  unsigned pending = 0, hit = 0;
#pragma unroll
  for (int q = 0; q < PB_PER_WAVE; ++q)
    if (lds_state[wave * PB_PER_WAVE + q] == NEEDS_SCAN) pending |= 1u << q;

  if (remove_far_box) {
    for (int t0 = 0; t0 < T; t0 += CH) {
#pragma unroll
      for (int a = 0; a < 3; ++a) lds_p[a][tid] = p[a];
      __syncthreads();
      const int nf = T - t0 < CH ? T - t0 : CH;      // frames of this chunk
      const long long tn = (long long)t0 + CH + tid;
      if (tn < T) {
#pragma unroll
        for (int a = 0; a < 3; ++a) p[a] = hip[tn * J * 3 + a];
      }
      if (pending) {
        double px[CH_STEPS], py[CH_STEPS], pz[CH_STEPS];
#pragma unroll
        for (int i = 0; i < CH_STEPS; ++i) {
          const int f = i * P2R_WAVE + lane;
          px[i] = (double)lds_p[0][f], py[i] = (double)lds_p[1][f], pz[i] = (double)lds_p[2][f];
        }
#pragma unroll
        for (int q = 0; q < PB_PER_WAVE; ++q) {
          if (!(pending >> q & 1)) continue;
          const double *fr = lds_fr[wave * PB_PER_WAVE + q];
          const double cx = fr[0], cy = fr[1], cz = fr[2], c = fr[3], s = fr[4], h0 = fr[5], h1 = fr[6], h2 = fr[7];
          const double ns = -s;
          bool in = false;
#pragma unroll
          for (int i = 0; i < CH_STEPS; ++i) {
            const double rx = px[i] - cx, ry = py[i] - cy, rz = pz[i] - cz;
            const double l0 = rx * c + rz * ns, l2 = rx * s + rz * c;
            in = in || (i * P2R_WAVE + lane < nf && fabs(l0) <= h0 && fabs(ry) <= h1 && fabs(l2) <= h2);
          }
          if (__ballot(in) != 0ull) hit |= 1u << q, pending &= ~(1u << q);
        }
      }
      if (lane == 0) lds_done[wave] = pending == 0;
      __syncthreads();
      int all_done = 1;
#pragma unroll
      for (int w = 0; w < PB_WAVES; ++w) all_done &= lds_done[w];
      if (all_done) break;
    }
  }

  if (lane < PB_PER_WAVE) {
    const int q = wave * PB_PER_WAVE + lane;
    if (k0 + q < K) {
      const int state = lds_state[q];
      nonempty[(long long)n * K + k0 + q] = state == DECIDED_NONEMPTY || (state == NEEDS_SCAN && (hit >> lane & 1));
    }
  }
}

}  // namespace

extern "C" int p2r_parse_boxes(const float *center, const float *size_log, const double *heading_sc,
                               const float *objectness, const float *sem_scores, const long long *cls_in,
                               const float *joints, int N, int K, int C, int Bj, int T, int J, int origin_joint,
                               double contact_dist, int remove_far_box, int nms_mode, double *corners, double *boxes,
                               float *obj_prob, long long *pred_cls, unsigned char *nonempty, void *stream) {
  if (!center || !size_log || !heading_sc || !objectness || !corners || !boxes || !obj_prob || !pred_cls || !nonempty ||
      N < 1 || K < 1 || nms_mode < 0 || nms_mode > 2)
    return P2R_EINVAL;
  if (!cls_in && (!sem_scores || C < 1)) return P2R_EINVAL;
  if (remove_far_box && (!joints || Bj < 1 || T < 1 || J < 1 || origin_joint < 0 || origin_joint >= J ||
                         (long long)Bj * T > (1LL << 40) / J))
    return P2R_EINVAL;
  const int groups = p2r_cdiv(K, PB);
  if ((long long)N * groups > 0x7fffffffLL) return P2R_EINVAL;
  hipLaunchKernelGGL(parse_boxes_kernel, dim3((unsigned)(N * groups)), dim3(PB_THREADS), 0, p2r_stream(stream), center,
                     size_log, heading_sc, objectness, sem_scores, cls_in, joints, K, C, Bj, T, J, origin_joint,
                     (float)contact_dist, remove_far_box, nms_mode, groups, corners, boxes, obj_prob, pred_cls, nonempty);
  P2R_LAUNCH_CHECK();
  return P2R_OK;
}
