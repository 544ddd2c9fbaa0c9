// batch_assemble.hip -- one training / evaluation batch built on the device from a device-resident sample store
// (include/p2r_hip.h: p2r_assemble_batch).  The reference builds each sample in NumPy on the host (dataloader.py:31-147,
// `augment_data` + `__getitem__`) and stacks them (`collate_fn`); this launch does all of it for a whole batch.
//
// Arithmetic (the contract that pose2room_amd/p2rnet/device_loader.py's `transform_reference` mirrors and the tests pin
// bit for bit against augment_sample + sample_to_tensors).  lin(x, M)[c] = ((0 + x0 M[0][c]) + x1 M[1][c]) + x2 M[2][c]
// in f64, never contracted (the library builds with -ffp-contract=off).  The leading +0 is the zeroed accumulator of the
// BLAS product behind np.dot: it turns an all-(-0) sum into +0, so a joint at y = -0 comes out at +0.
//   frames    src(t) = rint(t * step + 0.0), step = (T0 - 1) / (num_frames - 1) in f64, src(num_frames - 1) = T0 - 1,
//             src = 0 for num_frames == 1: np.linspace(0, T0 - 1, num_frames).round().  The transform is per frame, so
//             it runs on the num_frames gathered frames only.
//   flip      joints64 = lin(f64(joints), FLIP);  v_k = f32(lin(f64(v_k), FLIP))
//   rotate    base = joints64 (flipped) or the f32 joints;  end_k = lin(base + v_k, R) with the sum in f64 (flipped) or
//             f32;  joints64 = lin(base, R);  v_k = f32(end_k - joints64)
//   translate joints64 += (off, 0.0 * off, off);  input_joints = f32(joints64)
//   height    f32(joints64.y - floor) (augmented, f64 floor) or joints.y - floor in f32 (plain)
//   vote mask int64(trunc(votes[..., 0]))
// Without augmentation the joints and votes are a gather and a cast.
//
// Layout: a workgroup owns 256 consecutive (frame, joint) items of one batch sample (blockIdx.y), one per lane.  The
// mask goes out as one 8-byte store per lane; joints and votes are staged in LDS and leave as consecutive dwords, so
// every store instruction of the workgroup covers a contiguous span.  Workgroup 0 of a sample also writes its box rows.
#include "p2r_common.h"

namespace {

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

__global__ __launch_bounds__(AB_THREADS) void assemble_kernel(p2r_sample_store s, const long long *__restrict__ sel,
                                                              const double *__restrict__ aug, int augment,
                                                              int use_height, int T, p2r_batch_out o) {
  __shared__ float lds_j[AB_THREADS * 4];
  __shared__ float lds_v[AB_THREADS * 9];
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
    const float *xj = s.joints + row * 3, *xv = s.votes + row * 10;
    float jf[3], vf[10];
#pragma unroll
    for (int c = 0; c < 3; ++c) jf[c] = xj[c];
#pragma unroll
    for (int c = 0; c < 10; ++c) vf[c] = xv[c];
    float oj[4], ov[9];
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
      oj[3] = (float)(q.y - s.floor_height[2 * id]);
    } else {
#pragma unroll
      for (int c = 0; c < 3; ++c) oj[c] = jf[c];
#pragma unroll
      for (int c = 0; c < 9; ++c) ov[c] = vf[1 + c];
      oj[3] = jf[1] - (float)s.floor_height[2 * id + 1];
    }
    for (int c = 0; c < C; ++c) lds_j[tid * C + c] = oj[c];
#pragma unroll
    for (int c = 0; c < 9; ++c) lds_v[tid * 9 + c] = ov[c];
    o.vote_label_mask[b * TJ + p] = (long long)vf[0];
  }
  __syncthreads();
  float *dj = o.input_joints + (b * TJ + p0) * C, *dv = o.vote_label + (b * TJ + p0) * 9;
  for (int k = tid; k < n * C; k += AB_THREADS) dj[k] = lds_j[k];
  for (int k = tid; k < n * 9; k += AB_THREADS) dv[k] = lds_v[k];

  if (blockIdx.x == 0 && tid < K) {
    const int k = tid;
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
}

}  // namespace

extern "C" int p2r_assemble_batch(const p2r_sample_store *store, int B, const long long *sel, const double *aug,
                                  int augment, int use_height, int num_frames, const p2r_batch_out *out,
                                  void *stream) {
  if (!store || !out || B < 0 || B > 65535 || num_frames < 1 || (augment != 0 && augment != 1) ||
      (use_height != 0 && use_height != 1))
    return P2R_EINVAL;
  const p2r_sample_store &s = *store;
  const p2r_batch_out &o = *out;
  if (s.n_samples < 1 || s.J < 1 || s.K < 0 || s.K > AB_THREADS || s.n_frames_total < 1 || !s.joints || !s.votes ||
      !s.frame_offset || !s.n_frames || !s.floor_height || (s.K > 0 && (!s.box_center || !s.box_heading ||
      !s.box_size || !s.box_mask || !s.box_cls)))
    return P2R_EINVAL;
  if (B == 0) return P2R_OK;
  if (!sel || (augment && !aug) || !o.input_joints || !o.vote_label || !o.vote_label_mask ||
      (s.K > 0 && (!o.center_label || !o.size || !o.heading || !o.box_label_mask || !o.sem_cls_label)))
    return P2R_EINVAL;
  const long long TJ = (long long)num_frames * s.J;
  if (TJ > 0x7fffffffLL * AB_THREADS / 2) return P2R_EINVAL;
  hipLaunchKernelGGL(assemble_kernel, dim3((unsigned)p2r_cdiv(TJ, AB_THREADS), (unsigned)B), dim3(AB_THREADS), 0,
                     p2r_stream(stream), s, sel, aug, augment, use_height, num_frames, o);
  P2R_LAUNCH_CHECK();
  return P2R_OK;
}
