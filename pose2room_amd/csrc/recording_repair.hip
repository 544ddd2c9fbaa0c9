// recording_repair.hip -- raw recordings with missing joints conditioned on the device (include/p2r_recording_repair.h:
// p2r_joint_valid_bits, p2r_gap_fill, p2r_smooth_frames).  The reference has no such stage: its poses come out of a
// simulator and are always finite.  The arithmetic contract is the header's comment;
// pose2room_amd/net_utils/recording_repair.py's `repair_reference` mirrors it in NumPy.
//
// p2r_joint_valid_bits: a workgroup of 256 lanes owns one word, 64 frames of one recording, which it finds by a search
// of word_offset.  A frame is J * 3 doubles, so a lane per frame would stride by J * 24 bytes; instead the 64 frames are
// read as the consecutive doubles they are, and each leaves one byte in LDS: its exponent bits are all ones.  A wave then
// takes 16 joints at a time, lane i looks at frame i, one ballot forms the (word, joint); lane q keeps the word of the
// q-th joint and the 16 words leave as 128 consecutive bytes.
// p2r_gap_fill: the layout of sample_build.hip's build_kernel -- a workgroup owns 256 consecutive (frame, joint) items of
// the packed recordings, whose 768 doubles come in and leave through LDS as consecutive doubles.  A lane finds its
// recording by a search of frame_offset, reads its word of `bits` (consecutive lanes, consecutive joints: consecutive
// words) and, when its bit is clear, finds its neighbours with clz / ctz on its own word and at most max_gap / 64 + 1
// words to either side.  The counts and the longest run are integer atomics: into LDS slots for the first recordings the
// workgroup spans, one global atomic per slot and workgroup afterwards; into global memory for the others.
// p2r_smooth_frames: a workgroup owns 112 packed frames by 32 columns of the J * 3; the frames and 8 to either side sit
// in LDS (32 KB), a lane per frame finds the window its recording leaves it, and every element sums its taps in ascending
// order.  The 17 taps are compile-time positions of an unrolled loop, so the weights stay in scalar registers.
#include "p2r_common.h"

#include "../../include/p2r_recording_repair.h"

namespace {

constexpr int RR_THREADS = 256;
constexpr int BITS_JOINTS = 16;                  // joints a wave ballots before it stores their words
constexpr int FILL_SLOTS = 4;                    // recordings of a workgroup whose statistics are gathered in LDS
constexpr int SM_COLS = 32;
constexpr int SM_FRAMES = 112;
constexpr int SM_ROWS = SM_FRAMES + 2 * P2R_RR_MAX_HALF;
constexpr int TRUNCATED = 0x7fffffff;            // no neighbour within the words searched: the gap exceeds max_gap
constexpr unsigned long long EXPONENT = 0x7ff0000000000000ULL;
constexpr unsigned long long QUIET_NAN = 0x7ff8000000000000ULL;

struct Taps {
  double w[2 * P2R_RR_MAX_HALF + 1];             // w[k + 8] = the weight of frame f + k; unused positions are never read
};

// index of the last of the n ascending entries of t that is <= x, -1 if there is none (at most 32 trips)
__device__ __forceinline__ int last_le(const long long *__restrict__ t, int n, long long x) {
  int lo = 0, hi = n;
  for (int trip = 0; trip < 32 && lo < hi; ++trip) {
    const int mid = lo + ((hi - lo) >> 1);
    if (t[mid] <= x) lo = mid + 1; else hi = mid;
  }
  return lo - 1;
}

// the frames of recording r and its first frame, or none when its row is outside the limits of p2r_recordings
__device__ __forceinline__ int frames_of(const p2r_recordings &rc, int r, long long &off) {
  off = rc.frame_offset[r];
  const int F = rc.n_frames[r];
  if (F < 1 || F > rc.max_frames || off < 0 || off > rc.n_frames_total - F) return 0;
  return F;
}

// the same with its first word; none as well when its words do not lie inside 0 .. n_words_total - 1
__device__ __forceinline__ int span_of(const p2r_recordings &rc, const long long *__restrict__ word_offset,
                                       long long n_words_total, int r, long long &off, long long &word) {
  word = word_offset[r];
  const int F = frames_of(rc, r, off);
  if (F == 0 || word < 0 || word > n_words_total - ((F + 63) >> 6)) return 0;
  return F;
}

__global__ __launch_bounds__(RR_THREADS) void bits_kernel(p2r_recordings rc, const long long *__restrict__ word_offset,
                                                          long long n_words_total,
                                                          unsigned long long *__restrict__ bits) {
  extern __shared__ unsigned char bad[];          // 64 frames x J * 3 coordinates: the coordinate is not finite
  const long long w = blockIdx.x;
  const int tid = threadIdx.x, J = rc.J, J3 = 3 * rc.J;
  // everything up to `nf` is uniform over the workgroup
  const int r = last_le(word_offset, rc.R, w);
  long long off = 0, word = 0;
  const int F = r >= 0 ? span_of(rc, word_offset, n_words_total, r, off, word) : 0;
  const long long k = w - word;
  int nf = 0;                                     // the frames of this word: 0 for a word of no recording
  if (F > 0 && k >= 0 && k < ((F + 63) >> 6)) nf = F - 64 * (int)k < 64 ? F - 64 * (int)k : 64;
  if (nf > 0) {
    const unsigned long long *src = (const unsigned long long *)(rc.joints + (off + 64 * k) * J3);
    const int total = nf * J3;                    // <= 64 * 768
    for (int i = tid; i < total; i += RR_THREADS) bad[i] = (src[i] & EXPONENT) == EXPONENT;
  }
  __syncthreads();
  const int lane = tid & (P2R_WAVE - 1), wave = tid / P2R_WAVE;
  for (int j0 = wave * BITS_JOINTS; j0 < J; j0 += (RR_THREADS / P2R_WAVE) * BITS_JOINTS) {     // wave-uniform
    unsigned long long mine = 0;
#pragma unroll 4
    for (int q = 0; q < BITS_JOINTS; ++q) {
      const int j = j0 + q;
      bool valid = false;
      if (j < J && lane < nf) {
        const unsigned char *b = bad + lane * J3 + 3 * j;
        valid = (b[0] | b[1] | b[2]) == 0;
      }
      const unsigned long long m = __ballot(valid);
      if (lane == q) mine = m;
    }
    if (lane < BITS_JOINTS && j0 + lane < J) bits[w * J + j0 + lane] = mine;
  }
}

__global__ __launch_bounds__(RR_THREADS) void fill_kernel(p2r_recordings rc, const long long *__restrict__ word_offset,
                                                          long long n_words_total,
                                                          const unsigned long long *__restrict__ bits, int max_gap,
                                                          int hold_ends, long long FJ,
                                                          unsigned long long *__restrict__ out,
                                                          unsigned char *__restrict__ how, int *__restrict__ stats) {
  __shared__ unsigned long long lds[RR_THREADS * 3];          // the coordinates as bit patterns: a copy changes no bit
  __shared__ int lds_stats[FILL_SLOTS * 4];
  const int tid = threadIdx.x, J = rc.J;
  const long long p0 = (long long)blockIdx.x * RR_THREADS;
  const int n = FJ - p0 < RR_THREADS ? (int)(FJ - p0) : RR_THREADS;
  const unsigned long long *src = (const unsigned long long *)rc.joints + p0 * 3;
  for (int k = tid; k < n * 3; k += RR_THREADS) lds[k] = src[k];
  // the first recording this workgroup's items can belong to (uniform): recordings ascend with the frames
  int r_lo = last_le(rc.frame_offset, rc.R, p0 / J);
  if (r_lo < 0) r_lo = 0;
  if (tid < FILL_SLOTS * 4) lds_stats[tid] = 0;
  __syncthreads();

  if (tid < n) {
    const long long p = p0 + tid, g = p / J;
    const int j = (int)(p - g * J);
    const int r = last_le(rc.frame_offset, rc.R, g);
    long long off = 0, word = 0;
    const int F = r >= 0 ? span_of(rc, word_offset, n_words_total, r, off, word) : 0;
    const long long fl = g - off;
    unsigned char h = 0;
    if (F == 0 || fl >= F) {                                  // a frame of no recording
      lds[3 * tid] = 0ULL, lds[3 * tid + 1] = 0ULL, lds[3 * tid + 2] = 0ULL;
    } else {
      const int f = (int)fl, nw = (F + 63) >> 6, kw = f >> 6, bit = f & 63;
      const unsigned long long *bw = bits + word * J + j;     // word k of this joint: bw[k * J]
      // bits past the last frame are 0 by contract; masked here too, so that no neighbour lies outside the recording
      const int tail = F - 64 * (nw - 1);
      const unsigned long long tail_mask = tail < 64 ? (1ULL << tail) - 1ULL : ~0ULL;
      const unsigned long long own = bw[(long long)kw * J] & (kw == nw - 1 ? tail_mask : ~0ULL);
      if (!((own >> bit) & 1ULL)) {
        const int side = max_gap / 64 + 1;                    // <= 65
        int a = TRUNCATED, b = TRUNCATED;
        unsigned long long m = own & ((1ULL << bit) - 1ULL);
        if (m) {
          a = 64 * kw + 63 - __builtin_clzll(m);
        } else {
          for (int s = 1; s <= side + 1; ++s) {
            const int k = kw - s;
            if (k < 0) {
              a = -1;                                         // the recording begins inside the gap
              break;
            }
            if (s > side) break;                              // `side` full words without a valid frame
            m = bw[(long long)k * J];
            if (m) {
              a = 64 * k + 63 - __builtin_clzll(m);
              break;
            }
          }
        }
        m = own & ~((2ULL << bit) - 1ULL);                    // bit 63: 2 << 63 wraps to 0, the mask to all ones
        if (m) {
          b = 64 * kw + __builtin_ctzll(m);
        } else {
          for (int s = 1; s <= side + 1; ++s) {
            const int k = kw + s;
            if (k >= nw) {
              b = F;                                          // the recording ends inside the gap
              break;
            }
            if (s > side) break;                              // `side` words, none the last, so all of them full
            m = bw[(long long)k * J] & (k == nw - 1 ? tail_mask : ~0ULL);
            if (m) {
              b = 64 * k + __builtin_ctzll(m);
              break;
            }
          }
        }
        // b - a - 1 is the gap's length in all of its places: a = -1 in front, b = F at the end
        const bool cut = a == TRUNCATED || b == TRUNCATED;
        const int run = cut || b - a - 1 > max_gap ? max_gap + 1 : b - a - 1;
        const bool short_enough = run <= max_gap;
        const bool no_a = a == -1, no_b = b == F;
        unsigned long long v0 = QUIET_NAN, v1 = QUIET_NAN, v2 = QUIET_NAN;
        h = 3;
        if (short_enough && !no_a && !no_b) {
          const double *pa = rc.joints + ((off + a) * J + j) * 3, *pb = rc.joints + ((off + b) * J + j) * 3;
          const double span = (double)b - (double)a, at = (double)f - (double)a;
          double v[3];
#pragma unroll
          for (int c = 0; c < 3; ++c) {
            const double ya = pa[c], yb = pb[c];
            const double slope = (yb - ya) / span;
            v[c] = slope * at + ya;
          }
          v0 = (unsigned long long)__double_as_longlong(v[0]);
          v1 = (unsigned long long)__double_as_longlong(v[1]);
          v2 = (unsigned long long)__double_as_longlong(v[2]);
          h = 1;
        } else if (short_enough && hold_ends && no_a != no_b) {
          const unsigned long long *pe =
              (const unsigned long long *)rc.joints + ((off + (no_a ? b : a)) * J + j) * 3;
          v0 = pe[0], v1 = pe[1], v2 = pe[2];
          h = 2;
        }
        lds[3 * tid] = v0, lds[3 * tid + 1] = v1, lds[3 * tid + 2] = v2;
        const int slot = r - r_lo;
        if (slot >= 0 && slot < FILL_SLOTS) {
          int *s = lds_stats + 4 * slot;
          atomicAdd(s, 1);
          atomicAdd(s + (h == 3 ? 2 : 1), 1);
          atomicMax(s + 3, run);
        } else {
          int *s = stats + 4 * (long long)r;
          atomicAdd(s, 1);
          atomicAdd(s + (h == 3 ? 2 : 1), 1);
          atomicMax(s + 3, run);
        }
      }
    }
    how[p] = h;
  }
  __syncthreads();
  unsigned long long *dst = out + p0 * 3;
  for (int k = tid; k < n * 3; k += RR_THREADS) dst[k] = lds[k];
  if (tid < FILL_SLOTS * 4) {
    const int r = r_lo + (tid >> 2), v = lds_stats[tid];
    if (r < rc.R && v != 0) {
      if ((tid & 3) == 3) atomicMax(stats + 4 * (long long)r + 3, v);
      else atomicAdd(stats + 4 * (long long)r + (tid & 3), v);
    }
  }
}

__global__ __launch_bounds__(RR_THREADS) void smooth_kernel(p2r_recordings rc, int half, Taps taps,
                                                            double *__restrict__ out) {
  __shared__ double x[SM_ROWS][SM_COLS];
  __shared__ int k_lo[SM_FRAMES], k_hi[SM_FRAMES];            // the taps of a frame that lie inside its recording
  const int tid = threadIdx.x, J3 = 3 * rc.J;
  const long long g0 = (long long)blockIdx.x * SM_FRAMES;
  const int c0 = blockIdx.y * SM_COLS;
  const int nc = J3 - c0 < SM_COLS ? J3 - c0 : SM_COLS;
  const int nfr = rc.n_frames_total - g0 < SM_FRAMES ? (int)(rc.n_frames_total - g0) : SM_FRAMES;
  const int col = tid & (SM_COLS - 1), row = tid / SM_COLS;
  constexpr int STEP = RR_THREADS / SM_COLS;
  for (int i = row; i < nfr + 2 * P2R_RR_MAX_HALF; i += STEP) {        // row i = packed frame g0 - 8 + i
    const long long g = g0 - P2R_RR_MAX_HALF + i;
    if (col < nc && g >= 0 && g < rc.n_frames_total) x[i][col] = rc.joints[g * J3 + c0 + col];
  }
  if (tid < nfr) {
    const long long g = g0 + tid;
    const int r = last_le(rc.frame_offset, rc.R, g);
    long long off = 0;
    const int F = r >= 0 ? frames_of(rc, r, off) : 0;
    int lo = 1, hi = 0;                                       // empty: a frame of no recording
    if (F > 0 && g - off < F) {
      const int f = (int)(g - off);
      lo = f < half ? -f : -half;
      hi = F - 1 - f < half ? F - 1 - f : half;
    }
    k_lo[tid] = lo, k_hi[tid] = hi;
  }
  __syncthreads();
  for (int i = row; i < nfr; i += STEP) {
    if (col < nc) {
      const int lo = k_lo[i], hi = k_hi[i];
      double acc = 0.0, ws = 0.0;
#pragma unroll
      for (int k = -P2R_RR_MAX_HALF; k <= P2R_RR_MAX_HALF; ++k) {
        if (k >= lo && k <= hi) {                             // |k| <= half: a frame inside its recording, loaded above
          const double wk = taps.w[k + P2R_RR_MAX_HALF];
          acc = acc + wk * x[i + P2R_RR_MAX_HALF + k][col];
          ws = ws + wk;
        }
      }
      out[(g0 + i) * J3 + c0 + col] = lo <= hi ? acc / ws : 0.0;
    }
  }
}

bool recordings_ok(const p2r_recordings *rc) {
  return rc && rc->joints && rc->frame_offset && rc->n_frames && rc->R >= 1 && rc->J >= 1 && rc->J <= P2R_SB_MAX_J &&
         rc->max_frames >= 1 && rc->max_frames <= P2R_SB_MAX_FRAMES && rc->n_frames_total >= 1;
}

}  // namespace

extern "C" int p2r_joint_valid_bits(const p2r_recordings *rec, const long long *word_offset, long long n_words_total,
                                    unsigned long long *bits, void *stream) {
  if (!recordings_ok(rec) || !word_offset || !bits || n_words_total < 1 || n_words_total > 0x7fffffffLL)
    return P2R_EINVAL;
  const size_t lds = ((size_t)64 * 3 * rec->J + 15) & ~(size_t)15;           // <= 48 KB
  hipLaunchKernelGGL(bits_kernel, dim3((unsigned)n_words_total), dim3(RR_THREADS), lds, p2r_stream(stream), *rec,
                     word_offset, n_words_total, bits);
  P2R_LAUNCH_CHECK();
  return P2R_OK;
}

extern "C" int p2r_gap_fill(const p2r_recordings *rec, const long long *word_offset, long long n_words_total,
                            const unsigned long long *bits, int max_gap, int hold_ends, double *out,
                            unsigned char *how, int *stats, void *stream) {
  if (!recordings_ok(rec) || !word_offset || !bits || !out || !how || !stats || out == rec->joints ||
      n_words_total < 1 || n_words_total > 0x7fffffffLL || max_gap < 0 || max_gap > P2R_RR_MAX_GAP ||
      rec->n_frames_total > 0x7fffffffLL * RR_THREADS / rec->J)
    return P2R_EINVAL;
  const hipError_t e = hipMemsetAsync(stats, 0, sizeof(int) * 4 * (size_t)rec->R, p2r_stream(stream));
  if (e != hipSuccess) return (int)e;
  const long long FJ = rec->n_frames_total * rec->J;
  hipLaunchKernelGGL(fill_kernel, dim3((unsigned)p2r_cdiv(FJ, RR_THREADS)), dim3(RR_THREADS), 0, p2r_stream(stream),
                     *rec, word_offset, n_words_total, bits, max_gap, hold_ends != 0, FJ, (unsigned long long *)out,
                     how, stats);
  P2R_LAUNCH_CHECK();
  return P2R_OK;
}

extern "C" int p2r_smooth_frames(const p2r_recordings *rec, int half_width, double *out, void *stream) {
  if (!recordings_ok(rec) || !out || out == rec->joints || half_width < 1 || half_width > P2R_RR_MAX_HALF ||
      rec->n_frames_total > 0x7fffffffLL * SM_FRAMES)
    return P2R_EINVAL;
  // w_k = C(2h, k + h) / 4^h: integers below 2^14 over a power of two, exact
  Taps taps;
  for (int i = 0; i <= 2 * P2R_RR_MAX_HALF; ++i) taps.w[i] = 0.0;
  double c = 1.0, scale = 1.0;
  for (int i = 0; i < half_width; ++i) scale *= 4.0;
  for (int i = 0; i <= 2 * half_width; ++i) {
    taps.w[i - half_width + P2R_RR_MAX_HALF] = c / scale;
    c = c * (double)(2 * half_width - i) / (double)(i + 1);                  // C(2h, i + 1), an integer at every step
  }
  const dim3 grid((unsigned)p2r_cdiv(rec->n_frames_total, SM_FRAMES), (unsigned)p2r_cdiv(3 * rec->J, SM_COLS));
  hipLaunchKernelGGL(smooth_kernel, grid, dim3(RR_THREADS), 0, p2r_stream(stream), *rec, half_width, taps, out);
  P2R_LAUNCH_CHECK();
  return P2R_OK;
}
