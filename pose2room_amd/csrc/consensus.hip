// consensus.hip -- the consensus scene of H hypotheses on the device (include/p2r_consensus.h): greedy-leader clustering
// of the pooled oriented boxes of every sample, and per-cluster statistics.
//
// The cost is the pair test: H * K pooled boxes per sample, a Sutherland-Hodgman clip in fp64 per pair.  Two launches.
//
//   consensus_link_kernel     one wave per 64 x 64 tile (ti <= tj) of a sample's pool, in POOL order: whether i precedes j
//                             is a comparison of two scores, so no workgroup needs the ranking of the whole pool.  Lane l
//                             rebuilds the corners of row item l and of column item l (sin / cos once per item and tile,
//                             2 * 64 items for 4096 pairs) into LDS.  64 ballots prefilter the pairs -- another class,
//                             or strictly disjoint axis-aligned bounds -- and compact the survivors into a list, so the
//                             clip runs on full waves however few pairs survive (after a per-hypothesis NMS nearly all
//                             pairs of a scene are disjoint).  Link bits are collected in LDS (integer OR) and leave as
//                             one 64-bit word per row and tile: word (p, tj) and word (q, ti) have one writer each in the
//                             whole grid.  The diagonal tile owns its 64 items and stores their footprints for launch 2.
//   consensus_cluster_kernel  one workgroup of four waves per sample.  Rank by counting (nms3d.hip), then wave 0 walks the
//                             ranks: lane w holds word w of the `taken` bitset; the rows of eight ranks are loaded ahead
//                             of the walk (they do not depend on `taken`), so the latency of a row is paid once per
//                             eight steps.  Then every thread takes members (their IoU with the leader) and clusters
//                             (sums in ascending pool index, by walking the set bits of the leader's row).
#include "p2r_common.h"
#include "obb_iou_body.h"

#include "../../include/p2r_consensus.h"

namespace {

constexpr int CS_TILE = 64;                     // items per tile side = bits per word = lanes of the link kernel
constexpr int CS_REC = 12;                      // doubles per item in the workspace: ObbFoot (11) and the IoU with its leader
constexpr int CS_THREADS = 256;                 // cluster kernel
constexpr int CS_AHEAD = 8;                     // rows loaded ahead of the walk

__device__ __forceinline__ double cs_neg_inf() { return -__longlong_as_double(0x7ff0000000000000LL); }

// i precedes j: higher score first, equal scores: lower pool index first (scores with NaN already mapped to -inf)
__device__ __forceinline__ bool cs_precedes(float si, int pi, float sj, int pj) {
  return si > sj || (si == sj && pi < pj);
}

__device__ __forceinline__ float cs_score(float s) { return s != s ? (float)cs_neg_inf() : s; }

// s_off[h] = pool index of (h, 0), s_off[H .. 64] = the pool size.  All 64 lanes of wave 0 call it; one barrier.
__device__ __forceinline__ void cs_offsets(int H, int B, int K, int b, const int *__restrict__ count, int *s_off) {
  const int t = threadIdx.x;
  if (t < P2R_WAVE) {
    int c = 0;
    if (t < H) {
      c = count[(long long)t * B + b];
      c = c < 0 ? 0 : (c > K ? K : c);
    }
    s_off[t + 1] = c;
  }
  __syncthreads();
  if (t == 0) {
    int run = 0;
    s_off[0] = 0;
    for (int h = 0; h < P2R_WAVE; ++h) {
      run += s_off[h + 1];
      s_off[h + 1] = run;
    }
  }
  __syncthreads();
}

// pool index p < pool size -> the node slot (h * B + b) * K + s and h * K + s
__device__ __forceinline__ long long cs_node(int p, int H, int B, int K, int b, const int *s_off, int &hk) {
  int h = 0;
  for (int u = 1; u < H; ++u) h += s_off[u] <= p;
  const int s = p - s_off[h];
  hk = h * K + s;
  return ((long long)h * B + b) * K + s;
}

// params_to_corners (net_utils/multi_modal_eval.py) in its operation order
__device__ __forceinline__ void cs_corners(const double *__restrict__ o, double (&c)[24]) {
  const double h = o[6];
  const double ch = cos(h), sh = sin(h);
  const double R[3][3] = {{ch, 0.0, -sh}, {0.0, 1.0, 0.0}, {sh, 0.0, ch}};
  constexpr double SG[8][3] = {{-1, -1, -1}, {1, -1, -1}, {1, 1, -1}, {-1, 1, -1},
                               {-1, -1, 1},  {1, -1, 1},  {1, 1, 1},  {-1, 1, 1}};
  double v[3][3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double half = o[3 + k] / 2.0;
#pragma unroll
    for (int a = 0; a < 3; ++a) v[k][a] = half * R[k][a];
  }
#pragma unroll
  for (int i = 0; i < 8; ++i) {
#pragma unroll
    for (int a = 0; a < 3; ++a) c[i * 3 + a] = ((o[a] + SG[i][0] * v[0][a]) + SG[i][1] * v[1][a]) + SG[i][2] * v[2][a];
  }
}

__global__ __launch_bounds__(CS_TILE) void consensus_link_kernel(
    int H, int B, int K, int W, const int *__restrict__ count, const double *__restrict__ node_obbs,
    const long long *__restrict__ node_cls, const float *__restrict__ node_score, double thr, int class_aware,
    double *__restrict__ rec, unsigned long long *__restrict__ bits) {
  __shared__ double s_v[2][IOU_CAP][2][CS_TILE];       // 32 KiB: the clip's vertex buffers
  __shared__ ObbFoot s_foot[2][CS_TILE];               // [0]: the row items (tile ti), [1]: the column items (tile tj)
  __shared__ double s_bb[2][CS_TILE][4];               // x min, x max, z min, z max of the footprint
  __shared__ long long s_cls[2][CS_TILE];
  __shared__ float s_sc[2][CS_TILE];
  __shared__ unsigned long long s_bits[2][CS_TILE];    // [0][i]: bit j = row item i links column item j; [1][j]: bit i
  __shared__ unsigned short s_list[CS_TILE * CS_TILE]; // the pairs that pass the prefilter: i | j << 6
  __shared__ int s_off[P2R_WAVE + 1];
  const int lane = threadIdx.x;
  const int tj = blockIdx.x % W, ti = (blockIdx.x / W) % W, b = blockIdx.x / (W * W);
  if (ti > tj) return;
  cs_offsets(H, B, K, b, count, s_off);
  const int m = s_off[P2R_WAVE];
  if (tj * CS_TILE >= m) return;                       // uniform; ti <= tj
  const int Mc = H * K;

#pragma unroll
  for (int side = 0; side < 2; ++side) {
    const int p = (side == 0 ? ti : tj) * CS_TILE + lane;
    ObbFoot f = {};
    double bb[4] = {0.0, 0.0, 0.0, 0.0};
    long long cl = 0;
    float sc = 0.0f;
    if (p < m) {
      int hk;
      const long long node = cs_node(p, H, B, K, b, s_off, hk);
      double c[24];
      cs_corners(node_obbs + node * 7, c);
      obb_foot_load(c, f);
      bb[0] = bb[1] = f.x[0];
      bb[2] = bb[3] = f.y[0];
#pragma unroll
      for (int i = 1; i < 4; ++i) {
        bb[0] = f.x[i] < bb[0] ? f.x[i] : bb[0];
        bb[1] = f.x[i] > bb[1] ? f.x[i] : bb[1];
        bb[2] = f.y[i] < bb[2] ? f.y[i] : bb[2];
        bb[3] = f.y[i] > bb[3] ? f.y[i] : bb[3];
      }
      cl = node_cls[node];
      sc = cs_score(node_score[node]);
      if (side == 0 && ti == tj) {                     // the diagonal tile owns its items
        double *r = rec + ((long long)b * Mc + p) * CS_REC;
#pragma unroll
        for (int i = 0; i < 4; ++i) r[i] = f.x[i], r[4 + i] = f.y[i];
        r[8] = f.top, r[9] = f.bottom, r[10] = f.vol;
      }
    }
    s_foot[side][lane] = f;
#pragma unroll
    for (int i = 0; i < 4; ++i) s_bb[side][lane][i] = bb[i];
    s_cls[side][lane] = cl;
    s_sc[side][lane] = sc;
    s_bits[side][lane] = 0ull;
  }
  __syncthreads();

  // the prefilter: one row of the tile per step, lane = column.  A comparison with a NaN is false: such a pair stays.
  int n = 0;
  const int qj = tj * CS_TILE + lane;
  for (int i = 0; i < CS_TILE; ++i) {
    const int pi = ti * CS_TILE + i;
    bool ok = pi < m && qj < m && (ti < tj || i < lane);
    if (ok) {
      ok = !class_aware || s_cls[0][i] == s_cls[1][lane];
      const bool apart = s_bb[0][i][1] < s_bb[1][lane][0] || s_bb[1][lane][1] < s_bb[0][i][0] ||
                         s_bb[0][i][3] < s_bb[1][lane][2] || s_bb[1][lane][3] < s_bb[0][i][2] ||
                         s_foot[0][i].top < s_foot[1][lane].bottom || s_foot[1][lane].top < s_foot[0][i].bottom;
      ok = ok && !apart;
    }
    const unsigned long long mask = __ballot(ok);
    if (ok) s_list[n + __popcll(mask & ((1ull << lane) - 1ull))] = (unsigned short)(i | (lane << 6));
    n += __popcll(mask);                               // <= 64 per step: n <= 4096
  }
  __syncthreads();

  for (int k0 = 0; k0 < n; k0 += CS_TILE) {
    const int k = k0 + lane;
    if (k < n) {
      const int e = s_list[k], i = e & 63, j = e >> 6;
      const ObbFoot fi = s_foot[0][i], fj = s_foot[1][j];
      const bool first = cs_precedes(s_sc[0][i], ti * CS_TILE + i, s_sc[1][j], tj * CS_TILE + j);
      double unused;
      const double iou = first ? obb_pair_iou<CS_TILE>(fi, fj, s_v, lane, unused)
                               : obb_pair_iou<CS_TILE>(fj, fi, s_v, lane, unused);
      if (iou > thr) {
        atomicOr(&s_bits[0][i], 1ull << j);
        atomicOr(&s_bits[1][j], 1ull << i);
      }
    }
  }
  __syncthreads();

  const int pi = ti * CS_TILE + lane;
  unsigned long long *brow = bits + (long long)b * Mc * W;
  if (ti == tj) {
    if (pi < m) brow[(long long)pi * W + ti] = s_bits[0][lane] | s_bits[1][lane];
  } else {
    if (pi < m) brow[(long long)pi * W + tj] = s_bits[0][lane];
    if (qj < m) brow[(long long)qj * W + ti] = s_bits[1][lane];
  }
}

__device__ __forceinline__ unsigned long long cs_shfl64(unsigned long long v, int src) {
  const unsigned lo = (unsigned)__shfl((int)(unsigned)v, src), hi = (unsigned)__shfl((int)(unsigned)(v >> 32), src);
  return ((unsigned long long)hi << 32) | lo;
}

__global__ __launch_bounds__(CS_THREADS) void consensus_cluster_kernel(
    int H, int B, int K, int W, const int *__restrict__ count, const double *__restrict__ node_obbs,
    const long long *__restrict__ node_cls, const float *__restrict__ node_score, int *__restrict__ n_clusters,
    int *__restrict__ leader_node, int *__restrict__ members, int *__restrict__ support,
    long long *__restrict__ hyp_mask, double *__restrict__ box, long long *__restrict__ cls, float *__restrict__ score,
    double *__restrict__ score_mean, double *__restrict__ center_mean, double *__restrict__ center_rms,
    double *__restrict__ iou_mean, int *__restrict__ cluster_of, double *rec, const unsigned long long *bits) {
  extern __shared__ double lds_clip[];                 // [2][IOU_CAP][2][CS_THREADS]: 128 KiB
  __shared__ int s_order[P2R_CONSENSUS_MAX_POOL];      // rank -> pool index
  __shared__ int s_cl[P2R_CONSENSUS_MAX_POOL];         // pool index -> cluster, from the walk on
  __shared__ int s_lead[P2R_CONSENSUS_MAX_POOL];       // cluster -> pool index of its leader
  float *s_sc = reinterpret_cast<float *>(s_cl);       // score by pool index, until the ranks are known (24 KiB of
                                                       // tables and the 128 KiB of the clip fill the 160 KiB of a CU)
  __shared__ int s_off[P2R_WAVE + 1];
  __shared__ int s_ncl;
  const int tid = threadIdx.x, lane = tid & (P2R_WAVE - 1);
  const int b = blockIdx.x, Mc = H * K;
  cs_offsets(H, B, K, b, count, s_off);
  const int m = s_off[P2R_WAVE], Wm = (m + 63) >> 6;
  const unsigned long long *brow = bits + (long long)b * Mc * W;
  double *brec = rec + (long long)b * Mc * CS_REC;

  for (int p = tid; p < m; p += CS_THREADS) {
    int hk;
    s_sc[p] = cs_score(node_score[cs_node(p, H, B, K, b, s_off, hk)]);
  }
  __syncthreads();
  for (int p = tid; p < m; p += CS_THREADS) {
    const float sp = s_sc[p];
    int rank = 0;
    for (int u = 0; u < m; ++u) rank += cs_precedes(s_sc[u], u, sp, p);
    s_order[rank] = p;                                 // a total order: every rank 0 .. m-1 exactly once
  }
  __syncthreads();

  if (tid < P2R_WAVE) {                                // the walk: lane w holds word w of `taken`
    unsigned long long taken = 0ull;
    int ncl = 0;
    for (int r0 = 0; r0 < m; r0 += CS_AHEAD) {
      int p[CS_AHEAD];
      unsigned long long row[CS_AHEAD];
#pragma unroll
      for (int u = 0; u < CS_AHEAD; ++u) {
        p[u] = r0 + u < m ? s_order[r0 + u] : -1;
        row[u] = (p[u] >= 0 && lane < Wm) ? brow[(long long)p[u] * W + lane] : 0ull;
      }
#pragma unroll
      for (int u = 0; u < CS_AHEAD; ++u) {
        if (p[u] < 0) continue;                        // uniform
        const int pw = p[u] >> 6;
        const unsigned long long pb = 1ull << (p[u] & 63);
        if (cs_shfl64(taken, pw) & pb) continue;       // uniform: a member of an earlier leader
        unsigned long long claim = row[u] & ~taken;
        if (lane == pw) claim |= pb;
        if (lane >= Wm) claim = 0ull;
        taken |= claim;
        while (claim) {
          const int q = lane * 64 + __ffsll((long long)claim) - 1;
          claim &= claim - 1ull;
          if (q < m) s_cl[q] = ncl;
        }
        if (lane == 0) s_lead[ncl] = p[u];
        ++ncl;                                         // <= m: one per leader
      }
    }
    if (lane == 0) s_ncl = ncl;
  }
  __syncthreads();
  const int ncl = s_ncl;

  // the IoU of every member with its leader, the leader as the subject: one lane per member
  auto &s_v = *reinterpret_cast<double(*)[2][IOU_CAP][2][CS_THREADS]>(lds_clip);
  for (int q = tid; q < m; q += CS_THREADS) {
    const int L = s_lead[s_cl[q]];
    if (L == q) continue;
    ObbFoot fl, fq;
    const double *rl = brec + (long long)L * CS_REC, *rq = brec + (long long)q * CS_REC;
#pragma unroll
    for (int i = 0; i < 4; ++i) fl.x[i] = rl[i], fl.y[i] = rl[4 + i], fq.x[i] = rq[i], fq.y[i] = rq[4 + i];
    fl.top = rl[8], fl.bottom = rl[9], fl.vol = rl[10];
    fq.top = rq[8], fq.bottom = rq[9], fq.vol = rq[10];
    double unused;
    brec[(long long)q * CS_REC + 11] = obb_pair_iou<CS_THREADS>(fl, fq, s_v, tid, unused);
  }
  __syncthreads();                                     // slot 11 of a member is read by its cluster's thread below

  for (int c = tid; c < Mc; c += CS_THREADS) {
    const long long o = (long long)b * Mc + c;
    int lead_hk = -1, n = 0;
    unsigned long long hm = 0ull;
    double bx[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, mean[3] = {0.0, 0.0, 0.0};
    double smean = 0.0, rms = 0.0, imean = 0.0;
    long long lcls = 0;
    float lscore = 0.0f;
    if (c < ncl) {
      const int L = s_lead[c];
      const long long lnode = cs_node(L, H, B, K, b, s_off, lead_hk);
#pragma unroll
      for (int a = 0; a < 7; ++a) bx[a] = node_obbs[lnode * 7 + a];
      lcls = node_cls[lnode];
      lscore = node_score[lnode];
      double ssum = 0.0, csum[3] = {0.0, 0.0, 0.0}, isum = 0.0, dsum = 0.0;
      for (int pass = 0; pass < 2; ++pass) {
        for (int w = 0; w < Wm; ++w) {
          unsigned long long word = brow[(long long)L * W + w];
          if (w == (L >> 6)) word |= 1ull << (L & 63);
          while (word) {
            const int q = w * 64 + __ffsll((long long)word) - 1;
            word &= word - 1ull;
            if (q >= m || s_cl[q] != c) continue;
            int hk;
            const long long node = cs_node(q, H, B, K, b, s_off, hk);
            const double x = node_obbs[node * 7], y = node_obbs[node * 7 + 1], z = node_obbs[node * 7 + 2];
            if (pass == 0) {
              ++n;
              hm |= 1ull << (K > 0 ? hk / K : 0);
              ssum += (double)node_score[node];
              csum[0] += x, csum[1] += y, csum[2] += z;
              if (q != L) isum += brec[(long long)q * CS_REC + 11];
            } else {
              const double dx = x - mean[0], dy = y - mean[1], dz = z - mean[2];
              dsum += (dx * dx + dy * dy) + dz * dz;
            }
          }
        }
        if (pass == 0) {
          smean = ssum / (double)n;
#pragma unroll
          for (int a = 0; a < 3; ++a) mean[a] = csum[a] / (double)n;
          imean = n > 1 ? isum / (double)(n - 1) : 0.0;
        } else {
          rms = sqrt(dsum / (double)n);
        }
      }
    }
    leader_node[o] = lead_hk;
    members[o] = n;
    support[o] = __popcll(hm);
    hyp_mask[o] = (long long)hm;
#pragma unroll
    for (int a = 0; a < 7; ++a) box[o * 7 + a] = bx[a];
    cls[o] = lcls;
    score[o] = lscore;
    score_mean[o] = smean;
#pragma unroll
    for (int a = 0; a < 3; ++a) center_mean[o * 3 + a] = mean[a];
    center_rms[o] = rms;
    iou_mean[o] = imean;
  }
  for (int e = tid; e < Mc; e += CS_THREADS) {         // every node slot of this sample's H rows
    const int h = e / K, s = e - h * K;
    const int cnt = s_off[h + 1] - s_off[h];
    cluster_of[((long long)h * B + b) * K + s] = s < cnt ? s_cl[s_off[h] + s] : -1;
  }
  if (tid == 0) n_clusters[b] = ncl;
}

bool fits_int(long long v) { return v >= 0 && v <= 0x7fffffffLL; }

bool sizes_ok(int H, int B, int K) {
  if (H < 1 || H > P2R_CONSENSUS_MAX_H || B < 0 || K < 0 || K > P2R_CONSENSUS_MAX_K) return false;
  const long long Mc = (long long)H * K, W = (Mc + 63) / 64;
  return Mc <= P2R_CONSENSUS_MAX_POOL && fits_int((long long)B * Mc) && fits_int((long long)B * W * W);
}

}  // namespace

extern "C" unsigned long long p2r_consensus_workspace_bytes(int H, int B, int K) {
  if (!sizes_ok(H, B, K)) return 0ull;
  const unsigned long long Mc = (unsigned long long)H * K, W = (Mc + 63) / 64;
  return (unsigned long long)B * Mc * (CS_REC + W) * 8ull;
}

extern "C" int p2r_consensus(int H, int B, int K, const int *count, const double *node_obbs, const long long *node_cls,
                             const float *node_score, double iou_thresh, int class_aware, int *n_clusters,
                             int *leader_node, int *members, int *support, long long *hyp_mask, double *box,
                             long long *cls, float *score, double *score_mean, double *center_mean, double *center_rms,
                             double *iou_mean, int *cluster_of, void *workspace, unsigned long long workspace_bytes,
                             void *stream) {
  if (!sizes_ok(H, B, K) || !(iou_thresh >= 0.0)) return P2R_EINVAL;
  const unsigned long long need = p2r_consensus_workspace_bytes(H, B, K);
  if (workspace_bytes < need) return P2R_EINVAL;
  if (need > 0 && (!workspace || ((uintptr_t)workspace & 7u) != 0)) return P2R_EINVAL;
  if (B > 0 && (!count || !n_clusters)) return P2R_EINVAL;
  const int Mc = H * K;
  if ((long long)B * Mc > 0 &&
      (!node_obbs || !node_cls || !node_score || !leader_node || !members || !support || !hyp_mask || !box || !cls ||
       !score || !score_mean || !center_mean || !center_rms || !iou_mean || !cluster_of))
    return P2R_EINVAL;
  if (B == 0) return P2R_OK;
  const int W = (Mc + 63) / 64;
  double *rec = static_cast<double *>(workspace);
  unsigned long long *bits = reinterpret_cast<unsigned long long *>(rec + (size_t)B * Mc * CS_REC);
  if (Mc > 0) {
    hipLaunchKernelGGL(consensus_link_kernel, dim3((unsigned)(B * W * W)), dim3(CS_TILE), 0, p2r_stream(stream), H, B, K,
                       W, count, node_obbs, node_cls, node_score, iou_thresh, class_aware, rec, bits);
    P2R_LAUNCH_CHECK();
  }
  // 128 KiB of dynamic LDS beside 24 KiB of tables: the attribute is set to what the kernel takes, since the two together
  // must stay inside the 160 KiB of a CU
  constexpr int clip_bytes = (int)sizeof(double) * 2 * IOU_CAP * 2 * CS_THREADS;
  static unsigned char lds_ok[P2R_MAX_DEVICES];
  const hipError_t e = p2r_allow_big_lds(consensus_cluster_kernel, lds_ok, clip_bytes);
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(consensus_cluster_kernel, dim3((unsigned)B), dim3(CS_THREADS), clip_bytes, p2r_stream(stream), H, B, K,
                     W, count, node_obbs, node_cls, node_score, n_clusters, leader_node, members, support, hyp_mask, box,
                     cls, score, score_mean, center_mean, center_rms, iou_mean, cluster_of, rec,
                     (const unsigned long long *)bits);
  P2R_LAUNCH_CHECK();
  return P2R_OK;
}
