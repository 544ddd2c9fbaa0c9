// batch_assemble_body.h -- the body of the batch-assembly kernels: batch_assemble.hip (p2r_assemble_batch, the vote rows
// of an item are loaded from the store) and vote_labels.hip (p2r_assemble_batch_lean, they are derived from the item's
// joint and the sample's contact boxes).  The arithmetic contract and the layout are in the header comment of
// batch_assemble.hip; both kernels run this one body, so whatever votes an item has go through the same transform.
#pragma once
#include "p2r_common.h"

namespace p2r_ab {

constexpr int AB_THREADS = 256;

struct Vec3 { double x, y, z; };

__device__ __forceinline__ Vec3 lin(const Vec3 &v, const double *M) {
  return Vec3{((0.0 + v.x * M[0]) + v.y * M[3]) + v.z * M[6], ((0.0 + v.x * M[1]) + v.y * M[4]) + v.z * M[7],
              ((0.0 + v.x * M[2]) + v.y * M[5]) + v.z * M[8]};
}

__device__ __forceinline__ int source_frame(int t, int T0, int T) {
  if (T == 1) return 0;
  if (t == T - 1) return T0 - 1;
  const double step = (double)(T0 - 1) / (double)(T - 1);
  return (int)rint((double)t * step + 0.0);
}

// One (frame, joint) item: the raw joint jf and its raw vote row vf (column 0 = mask) -> the four joint columns oj
// (oj[3] = height above `floor`, the sample's two floor_height entries) and the nine vote columns ov.
__device__ __forceinline__ void transform_item(const float (&jf)[3], const float (&vf)[10], int augment, int flip,
                                               const double *R, double off, const double *floor, float (&oj)[4],
                                               float (&ov)[9]) {
  if (augment) {
    const double F[9] = {0.0, 0.0, 1.0, 0.0, 1.0, 0.0, 1.0, 0.0, 0.0};
    Vec3 base{(double)jf[0], (double)jf[1], (double)jf[2]}, end[3];
    if (flip) {
      base = lin(base, F);
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const Vec3 w = lin(Vec3{(double)vf[1 + 3 * k], (double)vf[2 + 3 * k], (double)vf[3 + 3 * k]}, F);
        const Vec3 v{(double)(float)w.x, (double)(float)w.y, (double)(float)w.z};
        end[k] = lin(Vec3{base.x + v.x, base.y + v.y, base.z + v.z}, R);
      }
    } else {
#pragma unroll
      for (int k = 0; k < 3; ++k)
        end[k] = lin(Vec3{(double)(jf[0] + vf[1 + 3 * k]), (double)(jf[1] + vf[2 + 3 * k]),
                          (double)(jf[2] + vf[3 + 3 * k])}, R);
    }
    Vec3 q = lin(base, R);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      ov[3 * k] = (float)(end[k].x - q.x);
      ov[3 * k + 1] = (float)(end[k].y - q.y);
      ov[3 * k + 2] = (float)(end[k].z - q.z);
    }
    q.x = q.x + off;
    q.y = q.y + 0.0 * off;
    q.z = q.z + off;
    oj[0] = (float)q.x;
    oj[1] = (float)q.y;
    oj[2] = (float)q.z;
    oj[3] = (float)(q.y - floor[0]);
  } else {
#pragma unroll
    for (int c = 0; c < 3; ++c) oj[c] = jf[c];
#pragma unroll
    for (int c = 0; c < 9; ++c) ov[c] = vf[1 + c];
    oj[3] = jf[1] - (float)floor[1];
  }
}

// Box row k of batch sample b (store sample id): the variant's centre plus the offset, and the label columns.
__device__ __forceinline__ void box_row(const p2r_sample_store &s, const p2r_batch_out &o, int b, long long id, int k,
                                        int variant, int augment, double off) {
  const int K = s.K;
  const long long bk = (long long)b * K + k, sk = id * K + k, vk = (id * P2R_BOX_VARIANTS + variant) * K + k;
  const double *c = s.box_center + vk * 3;
  const bool real = s.box_mask[sk] != 0.0f;
  const double dx = augment && real ? off : 0.0;
  o.center_label[bk * 3] = (float)(real ? c[0] + dx : c[0]);
  o.center_label[bk * 3 + 1] = (float)(real && augment ? c[1] + 0.0 * off : c[1]);
  o.center_label[bk * 3 + 2] = (float)(real ? c[2] + dx : c[2]);
#pragma unroll
  for (int i = 0; i < 3; ++i) o.size[bk * 3 + i] = s.box_size[sk * 3 + i];
  o.heading[bk * 2] = s.box_heading[vk * 2];
  o.heading[bk * 2 + 1] = s.box_heading[vk * 2 + 1];
  o.box_label_mask[bk] = s.box_mask[sk];
  o.sem_cls_label[bk] = s.box_cls[sk];
}

// The whole workgroup of either kernel.  votes(row, jf, vf) fills the raw vote row of store row `row`, whose joint is
// jf.  lds_j holds AB_THREADS * 4 floats and lds_v AB_THREADS * 9.  Every lane of the workgroup must call it: it has a
// barrier (the id test is uniform over the workgroup).
template <typename VoteSource>
__device__ __forceinline__ void assemble_body(const p2r_sample_store &s, const long long *__restrict__ sel,
                                              const double *__restrict__ aug, int augment, int use_height, int T,
                                              const p2r_batch_out &o, float *lds_j, float *lds_v, const VoteSource &votes) {
  const int b = blockIdx.y, tid = threadIdx.x;
  const long long id = sel[3 * b];
  if (id < 0 || id >= s.n_samples) return;
  const int J = s.J, C = use_height ? 4 : 3, K = s.K;
  const long long TJ = (long long)T * J, p0 = (long long)blockIdx.x * AB_THREADS;
  const int n = TJ - p0 < AB_THREADS ? (int)(TJ - p0) : AB_THREADS;
  const int T0 = s.n_frames[id];
  const long long f0 = s.frame_offset[id];
  int flip = 0, variant = P2R_BOX_VARIANTS - 1;
  double R[9], off = 0.0;
  if (augment) {
    flip = (int)sel[3 * b + 1];
    variant = (int)sel[3 * b + 2];
#pragma unroll
    for (int i = 0; i < 9; ++i) R[i] = aug[10 * b + i];
    off = aug[10 * b + 9];
  }

  if (tid < n) {
    const long long p = p0 + tid;
    const int t = (int)(p / J), j = (int)(p - (long long)t * J);
    const long long row = (f0 + source_frame(t, T0, T)) * J + j;
    const float *xj = s.joints + row * 3;
    float jf[3], vf[10];
#pragma unroll
    for (int c = 0; c < 3; ++c) jf[c] = xj[c];
    votes(row, jf, vf);
    float oj[4], ov[9];
    transform_item(jf, vf, augment, flip, R, off, s.floor_height + 2 * id, oj, ov);
    for (int c = 0; c < C; ++c) lds_j[tid * C + c] = oj[c];
#pragma unroll
    for (int c = 0; c < 9; ++c) lds_v[tid * 9 + c] = ov[c];
    o.vote_label_mask[b * TJ + p] = (long long)vf[0];
  }
  __syncthreads();
  float *dj = o.input_joints + (b * TJ + p0) * C, *dv = o.vote_label + (b * TJ + p0) * 9;
  for (int k = tid; k < n * C; k += AB_THREADS) dj[k] = lds_j[k];
  for (int k = tid; k < n * 9; k += AB_THREADS) dv[k] = lds_v[k];

  if (blockIdx.x == 0 && tid < K) box_row(s, o, b, id, tid, variant, augment, off);
}

// What p2r_assemble_batch and p2r_assemble_batch_lean check alike, the votes pointer aside.  -> P2R_OK to launch,
// P2R_EINVAL, or 1 for an empty batch (nothing to launch, no error).
static inline int check_arguments(const p2r_sample_store *store, int B, const long long *sel, const double *aug,
                                  int augment, int use_height, int num_frames, const p2r_batch_out *out) {
  if (!store || !out || B < 0 || B > 65535 || num_frames < 1 || (augment != 0 && augment != 1) ||
      (use_height != 0 && use_height != 1))
    return P2R_EINVAL;
  const p2r_sample_store &s = *store;
  const p2r_batch_out &o = *out;
  if (s.n_samples < 1 || s.J < 1 || s.K < 0 || s.K > AB_THREADS || s.n_frames_total < 1 || !s.joints ||
      !s.frame_offset || !s.n_frames || !s.floor_height || (s.K > 0 && (!s.box_center || !s.box_heading ||
      !s.box_size || !s.box_mask || !s.box_cls)))
    return P2R_EINVAL;
  if (B == 0) return 1;
  if (!sel || (augment && !aug) || !o.input_joints || !o.vote_label || !o.vote_label_mask ||
      (s.K > 0 && (!o.center_label || !o.size || !o.heading || !o.box_label_mask || !o.sem_cls_label)))
    return P2R_EINVAL;
  if ((long long)num_frames * s.J > 0x7fffffffLL * AB_THREADS / 2) return P2R_EINVAL;
  return P2R_OK;
}

}  // namespace p2r_ab
