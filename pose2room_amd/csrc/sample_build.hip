// sample_build.hip -- trainable samples made of raw recordings on the device (include/p2r_sample_build.h:
// p2r_recording_scan, p2r_build_samples, p2r_floor_percentile).  The reference does this on the host, one recording per
// pool process, when it writes its sample files (utils/virtualhome/3_generate_samples.py, run(), lines 96-187): trim
// the frames before the body enters the room, reject a recording that never comes near an object, recentre on the
// room's floor, write 8 flip / quarter-turn variants and derive the votes of each.  The arithmetic contract is the
// header's comment; pose2room_amd/net_utils/sample_build.py's `build_reference` mirrors it in NumPy.
//
// p2r_recording_scan: one workgroup of 1024 lanes per recording, a lane per frame.  A lane meets its frames in ascending
// order, so its first frame in the room is its smallest and its last frame near an object its largest; the workgroup
// reduces min(first in room) and max(last near an object) in a fixed order (wave butterflies, then 16 LDS slots), and
// "some frame f >= first is near an object" is max >= min -- one pass, no second walk from `first` on.  Room and object
// rows are uniform over the workgroup and come through the scalar cache.  The non-finite test reads every coordinate of
// the recording, coalesced, and looks at the exponent bits.
// p2r_build_samples: the layout of vote_labels.hip's vote_labels_kernel -- a workgroup owns 256 consecutive (frame,
// joint) items of the packed OUTPUT, finds their samples by a binary search of out_offset and walks the samples its
// items span (uniform, so a box row of 15 doubles is read with uniform addresses into scalar registers).  The vote rule
// is that kernel's with the f64 position q in place of the widened f32 joint.  The 3 + 10 floats of a lane are staged in
// LDS and leave as consecutive dwords.
// p2r_floor_percentile: one workgroup per sample selects up to four order statistics of the sample's heights at once.
// A height becomes a 32-bit key that orders like the float (sign flipped for positives, all bits for negatives, -0 first
// made +0); four passes over the 8-bit digits from the top count, per target rank, the keys that share the target's
// prefix into an LDS histogram of 256 bins (integer atomics: counts do not depend on their order), and a lane per target
// walks the bins to the one that holds its rank.  Targets with the same prefix share one histogram.  After the fourth
// pass the prefix is the key of the order statistic.
#include "p2r_common.h"

#include "../../include/p2r_sample_build.h"

namespace {

constexpr int SB_MAX_K = 256;
constexpr int SCAN_THREADS = 1024;
constexpr int BUILD_THREADS = 256;
constexpr int FLOOR_THREADS = 1024;
constexpr int NO_FRAME = 0x7fffffff;

// the frames of recording r, or none when its row is outside the limits of p2r_recordings
__device__ __forceinline__ int frames_of(const p2r_recordings &rc, int r, long long &off) {
  off = rc.frame_offset[r];
  const int F = rc.n_frames[r];
  if (F < 1 || F > rc.max_frames || off < 0 || off > rc.n_frames_total - F) return 0;
  return F;
}

// |R (p - c)| <= h per axis, c, R, h uniform
__device__ __forceinline__ bool inside_box(double p0, double p1, double p2, const double *c, const double *R,
                                           const double *h) {
  const double d0 = p0 - c[0], d1 = p1 - c[1], d2 = p2 - c[2];
  bool inside = true;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const double local = ((0.0 + d0 * R[3 * a]) + d1 * R[3 * a + 1]) + d2 * R[3 * a + 2];
    inside = inside && fabs(local) <= h[a];
  }
  return inside;
}

__device__ __forceinline__ int clamp_boxes(const p2r_contact_boxes &bx, long long row) {
  if (bx.K <= 0) return 0;
  const int nb = bx.n_boxes[row];
  return nb < 0 ? 0 : (nb > bx.K ? bx.K : nb);
}

__global__ __launch_bounds__(SCAN_THREADS) void scan_kernel(p2r_recordings rc, int origin,
                                                            const double *__restrict__ room, p2r_contact_boxes ob,
                                                            int *__restrict__ first, int *__restrict__ status) {
  __shared__ int lds_min[SCAN_THREADS / P2R_WAVE], lds_max[SCAN_THREADS / P2R_WAVE], lds_bad[SCAN_THREADS / P2R_WAVE];
  const int r = blockIdx.x, tid = threadIdx.x, J = rc.J;
  long long off;
  const int F = frames_of(rc, r, off);
  const double *rm = room + (long long)r * 15;
  const int nb = clamp_boxes(ob, r);
  const long long brow = (long long)r * ob.K;
  const double *bc = ob.centroid + brow * 3, *bR = ob.R_mat + brow * 9, *bh = ob.half + brow * 3;

  int my_first = NO_FRAME, my_near = -1;
  for (int f0 = 0; f0 < F; f0 += SCAN_THREADS) {          // F <= max_frames
    const int f = f0 + tid;
    if (f < F) {
      const double *p = rc.joints + ((off + f) * J + origin) * 3;
      const double p0 = p[0], p1 = p[1], p2 = p[2];
      if (my_first == NO_FRAME && inside_box(p0, p1, p2, rm, rm + 3, rm + 12)) my_first = f;
      bool near = false;
      for (int i = 0; i < nb; ++i) near = near || inside_box(p0, p1, p2, bc + 3 * i, bR + 9 * i, bh + 3 * i);
      if (near) my_near = f;
    }
  }
  // a coordinate is not finite iff its exponent bits are all ones
  int bad = 0;
  const unsigned long long *bits = (const unsigned long long *)(rc.joints + off * J * 3);
  const long long total = (long long)F * J * 3;
  for (long long i = tid; i < total; i += SCAN_THREADS)
    bad |= (bits[i] & 0x7ff0000000000000ULL) == 0x7ff0000000000000ULL;

#pragma unroll
  for (int m = P2R_WAVE / 2; m >= 1; m >>= 1) {
    my_first = min(my_first, __shfl_xor(my_first, m));
    my_near = max(my_near, __shfl_xor(my_near, m));
    bad |= __shfl_xor(bad, m);
  }
  if ((tid & (P2R_WAVE - 1)) == 0) {
    lds_min[tid / P2R_WAVE] = my_first;
    lds_max[tid / P2R_WAVE] = my_near;
    lds_bad[tid / P2R_WAVE] = bad;
  }
  __syncthreads();
  if (tid == 0) {
    int fst = NO_FRAME, near = -1, b = 0;
    for (int w = 0; w < SCAN_THREADS / P2R_WAVE; ++w) {
      fst = min(fst, lds_min[w]);
      near = max(near, lds_max[w]);
      b |= lds_bad[w];
    }
    const bool in_room = fst != NO_FRAME;
    first[r] = in_room ? fst : -1;
    status[r] = (in_room ? 0 : 1) | (in_room && near >= fst ? 0 : 2) | (b ? 4 : 0);
  }
}

// The table rows of one output sample (uniform over the workgroup) and its box count, clamped to 0..K.
struct BoxRows {
  const double *c, *R, *h;
  int nb;
};

__device__ __forceinline__ BoxRows rows_of(const p2r_contact_boxes &bx, long long id) {
  const long long row = id * bx.K;
  return BoxRows{bx.centroid + row * 3, bx.R_mat + row * 9, bx.half + row * 3, clamp_boxes(bx, id)};
}

// The vote row of the f64 position q against the boxes of its sample (the rule of p2r_vote_labels.h with p = q).
__device__ __forceinline__ void derive_votes(const double (&q)[3], const BoxRows &b, float (&vf)[10]) {
  int hits = 0;
  for (int i = 0; i < b.nb; ++i) {
    const double *c = b.c + 3 * i;
    const double c0 = c[0], c1 = c[1], c2 = c[2];
    if (inside_box(q[0], q[1], q[2], c, b.R + 9 * i, b.h + 3 * i)) {
      const float v0 = (float)(c0 - q[0]), v1 = (float)(c1 - q[1]), v2 = (float)(c2 - q[2]);
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

// index of the last sample whose first frame is <= frame, -1 if there is none (out_offset ascending)
__device__ __forceinline__ int sample_of_frame(const long long *__restrict__ out_offset, int S, long long frame) {
  int lo = 0, hi = S;
  while (lo < hi) {
    const int mid = lo + ((hi - lo) >> 1);
    if (out_offset[mid] <= frame) lo = mid + 1; else hi = mid;
  }
  return lo - 1;
}

__global__ __launch_bounds__(BUILD_THREADS) void build_kernel(p2r_recordings rc, p2r_sample_plan pl,
                                                              p2r_contact_boxes bx, long long FJ,
                                                              float *__restrict__ joints, float *__restrict__ votes) {
  __shared__ float lds_j[BUILD_THREADS * 3];
  __shared__ float lds_v[BUILD_THREADS * 10];
  const int tid = threadIdx.x, J = rc.J;
  const long long p0 = (long long)blockIdx.x * BUILD_THREADS;
  const int n = FJ - p0 < BUILD_THREADS ? (int)(FJ - p0) : BUILD_THREADS;
  // the samples this workgroup's items span: the same two searches in every lane, so the walk below is uniform
  int s_lo = sample_of_frame(pl.out_offset, pl.S, p0 / J);
  const int s_hi = sample_of_frame(pl.out_offset, pl.S, (p0 + n - 1) / J);
  if (s_lo < 0) s_lo = 0;

  int sid = -1;
  double q[3] = {0.0, 0.0, 0.0};
  float vf[10];
#pragma unroll
  for (int c = 0; c < 10; ++c) vf[c] = 0.0f;
  if (tid < n) {
    const long long p = p0 + tid, frame = p / J;
    const int j = (int)(p - frame * J);
    sid = sample_of_frame(pl.out_offset, pl.S, frame);
    if (sid >= 0) {
      const int r = pl.recording[sid], fst = pl.first[sid], a = pl.variant[sid];
      const long long local = frame - pl.out_offset[sid];
      long long off = 0;
      const int F = r >= 0 && r < rc.R ? frames_of(rc, r, off) : 0;
      if (fst < 0 || fst >= F || local >= (long long)(F - fst) || a < 0 || a > 7) {
        sid = -1;                                               // a frame of no sample
      } else {
        const double *src = rc.joints + ((off + fst + local) * J + j) * 3;
        const double *sh = pl.shift + 3 * (long long)sid;
        q[0] = src[0] - sh[0], q[1] = src[1] - sh[1], q[2] = src[2] - sh[2];
        if (a > 3) {
          const double t = q[0];
          q[0] = q[2], q[2] = t;
        }
#pragma unroll
        for (int k = 0; k < 3; ++k)
          if (k < (a & 3)) {
            const double t = q[0];
            q[0] = q[2], q[2] = -t;
          }
      }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) lds_j[tid * 3 + c] = (float)q[c];
  }
  if (votes) {
    // s is uniform: the rows of sample s come through scalar loads.  At most 256 trips (each sample has J >= 1 items)
    // when out_offset ascends strictly; samples that repeat an offset are walked too, so never more than S
    for (int s = s_lo; s <= s_hi; ++s) {
      const BoxRows rows = rows_of(bx, s);
      if (sid == s) derive_votes(q, rows, vf);
    }
    if (tid < n) {
#pragma unroll
      for (int c = 0; c < 10; ++c) lds_v[tid * 10 + c] = vf[c];
    }
  }
  __syncthreads();
  float *dj = joints + p0 * 3;
  for (int k = tid; k < n * 3; k += BUILD_THREADS) dj[k] = lds_j[k];
  if (votes) {
    float *dv = votes + p0 * 10;
    for (int k = tid; k < n * 10; k += BUILD_THREADS) dv[k] = lds_v[k];
  }
}

// a key that orders like the float; -0.0 and +0.0 get the same one
__device__ __forceinline__ unsigned key_of(float y) {
  const unsigned u = y == 0.0f ? 0u : __float_as_uint(y);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__device__ __forceinline__ float float_of(unsigned key) {
  return __uint_as_float((key & 0x80000000u) ? (key ^ 0x80000000u) : ~key);
}

__global__ __launch_bounds__(FLOOR_THREADS) void floor_kernel(const float *__restrict__ joints,
                                                              const long long *__restrict__ frame_offset,
                                                              const int *__restrict__ n_frames, int J, int max_frames,
                                                              long long F_total, double *__restrict__ floors) {
  __shared__ unsigned hist[4][256];
  __shared__ unsigned prefix[4], rank[4];
  __shared__ int has_nan;
  const int s = blockIdx.x, tid = threadIdx.x;
  const long long off = frame_offset[s];
  const int nf = n_frames[s];
  const double nan = __longlong_as_double(0x7ff8000000000000LL);
  if (nf < 1 || nf > max_frames || off < 0 || off > F_total - nf) {      // uniform over the workgroup
    if (tid == 0) floors[2 * s] = nan, floors[2 * s + 1] = nan;
    return;
  }
  const int n = nf * J;                                   // < 2^24
  const float *y = joints + off * J * 3 + 1;

  const double v64 = (double)(n - 1) * (0.99 / 100.0);
  const double k64 = floor(v64), g64 = v64 - k64;
  const float q32 = 0.99f / 100.0f;
  const float v32 = (float)(n - 1) * q32;
  const float k32 = floorf(v32), g32 = v32 - k32;
  if (tid < 4) {
    const int k = tid < 2 ? (int)k64 : (int)k32;
    const int want = k + (tid & 1);
    rank[tid] = (unsigned)(want < n - 1 ? want : n - 1);
    prefix[tid] = 0u;
  }
  if (tid == 0) has_nan = 0;

  for (int pass = 0; pass < 4; ++pass) {
    const int shift = 24 - 8 * pass;
    for (int k = tid; k < 4 * 256; k += FLOOR_THREADS) hist[k >> 8][k & 255] = 0u;
    __syncthreads();
    unsigned pre[4];
    bool own[4];                          // target t counts for itself: no earlier target has its prefix
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      pre[t] = prefix[t];
      own[t] = true;
      for (int u = 0; u < t; ++u) own[t] = own[t] && pre[u] != pre[t];
    }
    int saw_nan = 0;
    for (int i = tid; i < n; i += FLOOR_THREADS) {
      const float h = y[3 * (long long)i];
      saw_nan |= h != h;
      const unsigned key = key_of(h);
      const unsigned head = pass == 0 ? 0u : key >> (shift + 8);
#pragma unroll
      for (int t = 0; t < 4; ++t)
        if (own[t] && head == pre[t]) atomicAdd(&hist[t][(key >> shift) & 255u], 1u);
    }
    if (pass == 0 && saw_nan) has_nan = 1;
    __syncthreads();
    if (tid < 4) {
      int rep = tid;                      // the earliest target with this prefix holds the histogram
      for (int u = tid - 1; u >= 0; --u)
        if (pre[u] == pre[tid]) rep = u;
      unsigned left = rank[tid], bin = 255u;
      for (unsigned b = 0; b < 256u; ++b) {
        const unsigned c = hist[rep][b];
        if (left < c) {
          bin = b;
          break;
        }
        left -= c;
      }
      rank[tid] = left;
      prefix[tid] = (pre[tid] << 8) | bin;
    }
    __syncthreads();
  }
  if (tid == 0) {
    if (has_nan) {
      floors[2 * s] = nan, floors[2 * s + 1] = nan;
    } else {
      {
        const double a = (double)float_of(prefix[0]), b = (double)float_of(prefix[1]);
        const double d = b - a;
        double r = a + d * g64;
        if (g64 >= 0.5) r = b - d * (1.0 - g64);
        floors[2 * s] = r;
      }
      {
        const float a = float_of(prefix[2]), b = float_of(prefix[3]);
        const float d = b - a;
        float r = a + d * g32;
        if (g32 >= 0.5f) r = b - d * (1.0f - g32);
        floors[2 * s + 1] = (double)r;
      }
    }
  }
}

bool recordings_ok(const p2r_recordings *rc) {
  return rc && rc->joints && rc->frame_offset && rc->n_frames && rc->R >= 1 && rc->J >= 1 && rc->J <= P2R_SB_MAX_J &&
         rc->max_frames >= 1 && rc->max_frames <= P2R_SB_MAX_FRAMES && rc->n_frames_total >= 1;
}

// K in range, the count array there, and the three tables there when a box can be
bool boxes_ok(const p2r_contact_boxes *b) {
  return b && b->K >= 0 && b->K <= SB_MAX_K && b->n_boxes && (b->K == 0 || (b->centroid && b->R_mat && b->half));
}

}  // namespace

extern "C" int p2r_recording_scan(const p2r_recordings *rec, int origin_joint, const double *room,
                                  const p2r_contact_boxes *objects, int *first, int *status, void *stream) {
  if (!recordings_ok(rec) || !room || !boxes_ok(objects) || !first || !status || origin_joint < 0 ||
      origin_joint >= rec->J)
    return P2R_EINVAL;
  hipLaunchKernelGGL(scan_kernel, dim3((unsigned)rec->R), dim3(SCAN_THREADS), 0, p2r_stream(stream), *rec, origin_joint,
                     room, *objects, first, status);
  P2R_LAUNCH_CHECK();
  return P2R_OK;
}

extern "C" int p2r_build_samples(const p2r_recordings *rec, const p2r_sample_plan *plan, const p2r_contact_boxes *boxes,
                                 float *joints, float *votes, void *stream) {
  if (!recordings_ok(rec) || !plan || !plan->recording || !plan->first || !plan->variant || !plan->out_offset ||
      !plan->shift || plan->S < 1 || plan->n_frames_out < 1 ||
      plan->n_frames_out > 0x7fffffffLL * BUILD_THREADS / rec->J || !joints || (votes && !boxes_ok(boxes)))
    return P2R_EINVAL;
  const long long FJ = plan->n_frames_out * rec->J;
  p2r_contact_boxes bx = {nullptr, nullptr, nullptr, nullptr, 0};
  if (votes) bx = *boxes;
  hipLaunchKernelGGL(build_kernel, dim3((unsigned)p2r_cdiv(FJ, BUILD_THREADS)), dim3(BUILD_THREADS), 0,
                     p2r_stream(stream), *rec, *plan, bx, FJ, joints, votes);
  P2R_LAUNCH_CHECK();
  return P2R_OK;
}

extern "C" int p2r_floor_percentile(const float *joints, const long long *frame_offset, const int *n_frames,
                                    int n_samples, int J, int max_frames, long long n_frames_total, double *floors,
                                    void *stream) {
  if (!joints || !frame_offset || !n_frames || !floors || n_samples < 1 || J < 1 || J > P2R_SB_MAX_J ||
      max_frames < 1 || max_frames > P2R_SB_MAX_FRAMES || n_frames_total < 1)
    return P2R_EINVAL;
  hipLaunchKernelGGL(floor_kernel, dim3((unsigned)n_samples), dim3(FLOOR_THREADS), 0, p2r_stream(stream), joints,
                     frame_offset, n_frames, J, max_frames, n_frames_total, floors);
  P2R_LAUNCH_CHECK();
  return P2R_OK;
}
