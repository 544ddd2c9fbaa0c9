// vote_labels.hip -- vote labels derived on the device (include/p2r_vote_labels.h: p2r_vote_labels,
// p2r_assemble_batch_lean).  The reference makes them on the host, once per sample, when it writes its sample files
// (utils/virtualhome/3_generate_samples.py:56-79,176-187, `get_votes`): a Delaunay hull test of every joint against
// every object box enlarged by the contact distance.  For a box with orthonormal axes the hull test is the closed form
// below, and a vote row is a pure function of the joint and its sample's box table, so it can be computed where it is
// needed: for a whole packed store in one launch, or per gathered item inside the batch assembly, which then needs no
// stored votes at all.
//
// Arithmetic (the contract pose2room_amd/net_utils/vote_labels.py's `vote_labels_reference` mirrors), f64 throughout,
// never contracted (the library builds with -ffp-contract=off).  For the boxes i = 0 .. n-1 of the sample in list order,
// c the centroid, R the row-major 3x3 axes, h = size / 2 + contact distance (computed on the host), p the f32 joint
// widened to f64:
//   d = p - c;  local_a = ((0.0 + d0 R[a][0]) + d1 R[a][1]) + d2 R[a][2];  inside_i = |local_a| <= h_a for all three a
//   vote_i = f32(c - p);  hits = the number of earlier boxes with inside
//   on inside_i: column 0 = 1; slot min(hits, 2) = vote_i; with hits == 0 slots 1 and 2 = vote_i as well
// A joint inside no box has ten +0.0f.
//
// Layout: one (frame, joint) item per lane, 256 per workgroup.  The sample a lane works on is uniform over the
// workgroup -- p2r_assemble_batch_lean: the batch sample of blockIdx.y; p2r_vote_labels: the loop variable of a walk
// over the samples the workgroup's items span -- so a box row (15 doubles: c, R, h) is read with uniform addresses
// through the scalar cache into scalar registers: no LDS table, no barrier around it.  (A table staged in LDS per
// workgroup was measured too and is no faster: 41.8-43.1 us per lean launch at bs=32, T=1024 against 40.7-41.5 us.
// What the lean launch adds over the 30-32 us of the stored votes is the fp64 arithmetic of the box loop, about 30
// instructions per box and item, on top of the transform's.)
// p2r_vote_labels: a workgroup owns 256 consecutive (frame, joint) items of the PACKED store.  The frame counts are
// device data the host cannot size a per-sample grid by, so each lane finds its sample by a binary search of
// frame_offset, and the workgroup walks the samples its items span (at most 256, each has J >= 1 items; one for all
// but a workgroup at a seam).  The ten floats of a lane are staged in LDS and leave as consecutive dwords.
// p2r_assemble_batch_lean: the body of assemble_kernel (batch_assemble_body.h) with a vote source that derives the row
// instead of loading it.
#include "batch_assemble_body.h"

#include "../../include/p2r_vote_labels.h"

using namespace p2r_ab;

namespace {

constexpr int VL_THREADS = AB_THREADS;
constexpr int VL_MAX_K = 256;

// The table rows of one sample (uniform over the workgroup) and its box count, clamped to 0..K.
struct BoxRows {
  const double *c, *R, *h;
  int nb;
};

__device__ __forceinline__ BoxRows rows_of(const p2r_contact_boxes &bx, long long id) {
  const int nb = bx.n_boxes[id];
  const long long row = id * bx.K;
  return BoxRows{bx.centroid + row * 3, bx.R_mat + row * 9, bx.half + row * 3, nb < 0 ? 0 : (nb > bx.K ? bx.K : nb)};
}

// The vote row of joint jf against the boxes of its sample.
__device__ __forceinline__ void derive_votes(const float (&jf)[3], const BoxRows &b, float (&vf)[10]) {
#pragma unroll
  for (int c = 0; c < 10; ++c) vf[c] = 0.0f;
  const double p0 = (double)jf[0], p1 = (double)jf[1], p2 = (double)jf[2];
  int hits = 0;
  for (int i = 0; i < b.nb; ++i) {
    const double *c = b.c + 3 * i, *R = b.R + 9 * i, *h = b.h + 3 * i;
    const double c0 = c[0], c1 = c[1], c2 = c[2];
    const double d0 = p0 - c0, d1 = p1 - c1, d2 = p2 - c2;
    bool inside = true;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const double local = ((0.0 + d0 * R[3 * a]) + d1 * R[3 * a + 1]) + d2 * R[3 * a + 2];
      inside = inside && fabs(local) <= h[a];
    }
    if (inside) {
      const float v0 = (float)(c0 - p0), v1 = (float)(c1 - p1), v2 = (float)(c2 - p2);
      vf[0] = 1.0f;
      if (hits == 0) {
        vf[1] = v0, vf[2] = v1, vf[3] = v2;
      }
      if (hits <= 1) {
        vf[4] = v0, vf[5] = v1, vf[6] = v2;
      }
      if (hits != 1) {
        vf[7] = v0, vf[8] = v1, vf[9] = v2;
      }
      ++hits;
    }
  }
}

// index of the last sample whose first frame is <= frame, -1 if there is none (frame_offset ascending)
__device__ __forceinline__ int sample_of_frame(const long long *__restrict__ frame_offset, int N, long long frame) {
  int lo = 0, hi = N;
  while (lo < hi) {
    const int mid = lo + ((hi - lo) >> 1);
    if (frame_offset[mid] <= frame) lo = mid + 1; else hi = mid;
  }
  return lo - 1;
}

__global__ __launch_bounds__(VL_THREADS) void vote_labels_kernel(const float *__restrict__ joints,
                                                                 const long long *__restrict__ frame_offset,
                                                                 const int *__restrict__ n_frames, int N, int J,
                                                                 long long FJ, p2r_contact_boxes bx,
                                                                 float *__restrict__ votes) {
  __shared__ float lds_v[VL_THREADS * 10];
  const int tid = threadIdx.x;
  const long long p0 = (long long)blockIdx.x * VL_THREADS;
  const int n = FJ - p0 < VL_THREADS ? (int)(FJ - p0) : VL_THREADS;
  // the samples this workgroup's items span: the same two searches in every lane, so the walk below is uniform
  int s_lo = sample_of_frame(frame_offset, N, p0 / J);
  const int s_hi = sample_of_frame(frame_offset, N, (p0 + n - 1) / J);
  if (s_lo < 0) s_lo = 0;

  int sid = -1;
  float jf[3] = {0.0f, 0.0f, 0.0f}, vf[10];
#pragma unroll
  for (int c = 0; c < 10; ++c) vf[c] = 0.0f;
  if (tid < n) {
    const long long p = p0 + tid, frame = p / J;
    sid = sample_of_frame(frame_offset, N, frame);
    if (sid >= 0 && frame - frame_offset[sid] >= (long long)n_frames[sid]) sid = -1;      // a frame of no sample
#pragma unroll
    for (int c = 0; c < 3; ++c) jf[c] = joints[p * 3 + c];
  }
  for (int s = s_lo; s <= s_hi; ++s) {      // s is uniform: the rows of sample s come through scalar loads
    const BoxRows rows = rows_of(bx, s);
    if (sid == s) derive_votes(jf, rows, vf);
  }
  if (tid < n) {
#pragma unroll
    for (int c = 0; c < 10; ++c) lds_v[tid * 10 + c] = vf[c];
  }
  __syncthreads();
  float *dv = votes + p0 * 10;
  for (int k = tid; k < n * 10; k += VL_THREADS) dv[k] = lds_v[k];
}

// the vote row of an item derived from its joint and the boxes of its sample
struct DerivedVotes {
  BoxRows rows;
  __device__ __forceinline__ void operator()(long long, const float (&jf)[3], float (&vf)[10]) const {
    derive_votes(jf, rows, vf);
  }
};

__global__ __launch_bounds__(AB_THREADS) void assemble_lean_kernel(p2r_sample_store s, p2r_contact_boxes bx,
                                                                   const long long *__restrict__ sel,
                                                                   const double *__restrict__ aug, int augment,
                                                                   int use_height, int T, p2r_batch_out o) {
  __shared__ float lds_j[AB_THREADS * 4];
  __shared__ float lds_v[AB_THREADS * 9];
  const long long id = sel[3 * blockIdx.y];
  if (id < 0 || id >= s.n_samples) return;          // uniform over the workgroup; assemble_body tests it again
  assemble_body(s, sel, aug, augment, use_height, T, o, lds_j, lds_v, DerivedVotes{rows_of(bx, id)});
}

// K in range, the count array there, and the three tables there when a box can be
bool boxes_ok(const p2r_contact_boxes *b) {
  return b && b->K >= 0 && b->K <= VL_MAX_K && b->n_boxes && (b->K == 0 || (b->centroid && b->R_mat && b->half));
}

}  // namespace

extern "C" int p2r_vote_labels(const float *joints, const long long *frame_offset, const int *n_frames, int n_samples,
                               int J, long long n_frames_total, const p2r_contact_boxes *boxes, float *votes,
                               void *stream) {
  if (!joints || !frame_offset || !n_frames || !votes || !boxes_ok(boxes) || n_samples < 1 || J < 1 ||
      n_frames_total < 1 || n_frames_total > 0x7fffffffLL * VL_THREADS / J)
    return P2R_EINVAL;
  const long long FJ = n_frames_total * J;
  hipLaunchKernelGGL(vote_labels_kernel, dim3((unsigned)p2r_cdiv(FJ, VL_THREADS)), dim3(VL_THREADS), 0,
                     p2r_stream(stream), joints, frame_offset, n_frames, n_samples, J, FJ, *boxes, votes);
  P2R_LAUNCH_CHECK();
  return P2R_OK;
}

extern "C" int p2r_assemble_batch_lean(const p2r_sample_store *store, const p2r_contact_boxes *boxes, int B,
                                       const long long *sel, const double *aug, int augment, int use_height,
                                       int num_frames, const p2r_batch_out *out, void *stream) {
  if (!store || store->votes || !boxes_ok(boxes)) return P2R_EINVAL;
  const int st = check_arguments(store, B, sel, aug, augment, use_height, num_frames, out);
  if (st != P2R_OK) return st < 0 ? st : P2R_OK;
  const long long TJ = (long long)num_frames * store->J;
  hipLaunchKernelGGL(assemble_lean_kernel, dim3((unsigned)p2r_cdiv(TJ, AB_THREADS), (unsigned)B), dim3(AB_THREADS), 0,
                     p2r_stream(stream), *store, *boxes, sel, aug, augment, use_height, num_frames, *out);
  P2R_LAUNCH_CHECK();
  return P2R_OK;
}
