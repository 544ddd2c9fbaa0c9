// stgcn_gcn3_dcoef_body.h -- adjacency gradient of the fused graph convolution, statically scheduled for the P2RNet
// skeleton (gfx950): what stgcn_gcn3_grad.hip (exact) and stgcn_gcn3h_grad.hip (split16) have in common -- the work list,
// the data movement, the wave reduction, the kernel and the host-side launch.  No translation unit or ABI entry of its
// own.  The including file explains its arithmetic and provides, in an anonymous namespace in front of the include:
//   D3A, D3B, D3W          A-operand set and B operand of one slot (registers); element type of the W operand in memory
//   D3Extra                the parameter fields of its own (a base of D3Params)
//   d3_product(h, a, b)    h = the Y tile of one (plane, joint) unit
//   d3_load_a(a, W, k, ph, lane)          a = A operands of plane k, output rows 16 ph .. 16 ph + 15
//   d3_read_x(b, xr, joint, sl, xscale)   the four channels of the staged X slice `sl` into their places in b (below)
//   d3_copy_a(dst, src)                   one A-operand set to the other
//   d3_scales(extra, xscale, inv)         scale of X as an operand; factor on the table at write-out (1, 1: exact)
//   D3_FENCED              constexpr bool: scheduling fences around the product
//   D3_KERNEL              the kernel's name (profiles and tools key on it)
//   D3_TRACE_TILE, D3_MARK cycle-trace points (optional)
#include "gcn3_sched.inc"

#ifndef D3_MARK
#define D3_TRACE_TILE(tile)
#define D3_MARK(i)
#endif
namespace {

// the shared tile (stgcn_tile.h); a slice here is 16 rows of dZ or X
constexpr int D3_F = TILE_F, D3_NW = TILE_NW, D3_SLOTS = TILE_SLOTS, D3_V = TILE_V;
constexpr int D3_RS = TILE_RS, D3_BUF = TILE_BUF, D3_NV4 = TILE_NV4, D3_PW = TILE_PW;
static_assert(G3_V == TILE_V, "schedule generated for another skeleton");

struct D3Common {
  int T, ltot;
  int tiles_per_seq, total_tiles;
};
struct D3Params : D3Common, D3Extra {};

constexpr int d3_slot_joints[D3_NW][D3_SLOTS] = G3_SLOT_JOINTS_1;
constexpr int d3_plane0[D3_NW] = G3_PLANE0_1;

// dv[j][q] = dZ slice row (4 g + q), frame r, joint of entry j  (LDS row 4 q + g: offset q * 4 * RS floats)
template <int NE, int O0, int O1, int O2, int O3, int O4, int O5>
__device__ __forceinline__ void d3_gather(const char *xl, float (&dv)[6][4]) {
  constexpr int off[6] = {O0, O1, O2, O3, O4, O5};
#pragma unroll
  for (int j = 0; j < NE; ++j)
#pragma unroll
    for (int q = 0; q < 4; ++q) dv[j][q] = *reinterpret_cast<const float *>(xl + off[j] + q * 4 * D3_RS * 4);
}

// Wave reduction of the step's per-lane products.  VALU work is matrix-pipe time on gfx950 (fp32 MFMAs issue through
// the vector datapath), so the reduction is built to need as few vector instructions per entry as possible:
//   * products as packed pairs (v_pk_mul / v_pk_fma on the register pairs the MFMA tile and the 2-address LDS reads
//     deliver) + one add;
//   * entries are reduced TWO per register: v_permlane32_swap exchanges the upper half of entry A with the lower half
//     of entry B, one add folds both -- lanes 0-31 then carry A, lanes 32-63 carry B through the same four DPP row
//     stages, and one row_bcast15 add leaves A's total in lane 31 and B's in lane 63;
//   * an unpaired entry takes row_bcast15 + row_bcast31 (total in lane 63) instead of two lane swaps;
//   * all chains of a step advance stage by stage, so independent instructions fill the DPP wait states;
//   * lanes 31 / 63 add the totals into the workgroup's LDS table (no return value: nothing waits for the atomic).
template <int CTRL>
__device__ __forceinline__ float d3_add_dpp(float v) {      // bound_ctrl: lanes without a source add 0
  return v + __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xf, 0xf, true));
}
// ds_add_f32 of ONE lane (exec = `mask` for the one instruction) at an immediate offset of the table base: no VALU,
// no branch.  The code around it is wave-uniform, so exec is all ones before and after.
template <int OFF>
__device__ __forceinline__ void d3_lane_add(unsigned base, float v, unsigned long long mask) {
  asm volatile("s_mov_b64 exec, %2\n\tds_add_f32 %0, %1 offset:%3\n\ts_mov_b64 exec, -1"
               : : "v"(base), "v"(v), "s"(mask), "n"(OFF) : "memory");
}
template <int NE, int C0, int C1, int C2, int C3, int C4, int C5>
__device__ __forceinline__ void d3_reduce(const f32x4 &h, const float (&dv)[6][4], unsigned dcs) {
  constexpr unsigned long long L31 = 1ull << 31, L63 = 1ull << 63;
  constexpr int NP = NE / 2, NV = NP + (NE & 1);
  const f32x2 h01 = {h[0], h[1]}, h23 = {h[2], h[3]};
  float t[NE];
#pragma unroll
  for (int j = 0; j < NE; ++j) {
    f32x2 pr = h01 * f32x2{dv[j][0], dv[j][1]};
    pr = __builtin_elementwise_fma(h23, f32x2{dv[j][2], dv[j][3]}, pr);
    t[j] = pr.x + pr.y;
  }
  float v[NV];
#pragma unroll
  for (int q = 0; q < NP; ++q) {
    auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(t[2 * q]), __float_as_uint(t[2 * q + 1]), false, false);
    v[q] = __uint_as_float(sw[0]) + __uint_as_float(sw[1]);
  }
  if (NE & 1) v[NP] = t[NE - 1];
#pragma unroll
  for (int q = 0; q < NV; ++q) v[q] = d3_add_dpp<0xB1>(v[q]);      // quad_perm [1,0,3,2]
#pragma unroll
  for (int q = 0; q < NV; ++q) v[q] = d3_add_dpp<0x4E>(v[q]);      // quad_perm [2,3,0,1]
#pragma unroll
  for (int q = 0; q < NV; ++q) v[q] = d3_add_dpp<0x141>(v[q]);     // row_half_mirror
#pragma unroll
  for (int q = 0; q < NV; ++q) v[q] = d3_add_dpp<0x140>(v[q]);     // row_mirror: every lane of a row holds the row sum
#pragma unroll
  for (int q = 0; q < NV; ++q) v[q] = d3_add_dpp<0x142>(v[q]);     // row_bcast15: rows 1 / 3 += rows 0 / 2
  if (NE & 1) v[NP] = d3_add_dpp<0x143>(v[NP]);                    // row_bcast31: rows 2, 3 += lane 31: total in lane 63
  if (NP > 0) { d3_lane_add<4 * C0>(dcs, v[0], L31); d3_lane_add<4 * C1>(dcs, v[0], L63); }
  if (NP > 1) { d3_lane_add<4 * C2>(dcs, v[1], L31); d3_lane_add<4 * C3>(dcs, v[1], L63); }
  if (NP > 2) { d3_lane_add<4 * C4>(dcs, v[2], L31); d3_lane_add<4 * C5>(dcs, v[2], L63); }
  if (NE == 1) d3_lane_add<4 * C0>(dcs, v[0], L63);
  if (NE == 3) d3_lane_add<4 * C2>(dcs, v[1], L63);
  if (NE == 5) d3_lane_add<4 * C4>(dcs, v[2], L63);
}

#define D3_VISIT(set, plane, next, wrap, piece)                                      \
  {                                                                                  \
    load_a(aS[(set) ^ 1], next, (wrap) ? ((ph + 1) & 3) : ph);                        \
    if ((piece) >= 0 && copy) dma_piece(piece);                                      \
  }
#define D3_STEP(set, slot, ne, o0, c0, o1, c1, o2, c2, o3, c3, o4, c4, o5, c5)   \
  {                                                                              \
    float dv_[6][4];                                                             \
    d3_gather<ne, o0, o1, o2, o3, o4, o5>(xl, dv_);                              \
    if (D3_FENCED) __builtin_amdgcn_sched_barrier(0);                            \
    d3_product(h, aS[set], bz[slot]);                                            \
    if (D3_FENCED) __builtin_amdgcn_sched_barrier(0);                            \
    d3_reduce<ne, c0, c1, c2, c3, c4, c5>(h, dv_, dcs_off);                      \
  }
#define D3_CONT(ne, o0, c0, o1, c1, o2, c2, o3, c3, o4, c4, o5, c5)   \
  {                                                                   \
    float dv_[6][4];                                                  \
    d3_gather<ne, o0, o1, o2, o3, o4, o5>(xl, dv_);                   \
    d3_reduce<ne, c0, c1, c2, c3, c4, c5>(h, dv_, dcs_off);           \
  }
#define D3_END(parity, pieces)                                                            \
  {                                                                                       \
    if (copy) { _Pragma("unroll") for (int i_ = pieces; i_ < D3_PW; ++i_) dma_piece(i_); } \
    if (parity) d3_copy_a(aS[0], aS[1]);                                                  \
  }

template <int WAVE>
__device__ __forceinline__ void d3_wave_main(const D3Params &p, float *lds, const float *__restrict__ x,
                                             const float *__restrict__ dz, const D3W *__restrict__ W, float xscale) {
  constexpr int V = D3_V, RS = D3_RS, BUF = D3_BUF, NW = D3_NW, SLOTS = D3_SLOTS;
  constexpr int wave = WAVE;
  // [ltot][V] accumulated gradient of this workgroup, addressed off a VGPR base the compiler cannot fold (a known
  // base makes every entry address its own hoisted scalar constant: hundreds of spilled SGPRs)
  unsigned dcs_off = (unsigned)(2 * BUF * sizeof(float));
  asm volatile("" : "+v"(dcs_off));
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int g = lane >> 4, r = lane & 15;
  constexpr const int (&sj)[SLOTS] = d3_slot_joints[WAVE];

  const size_t row_stride = (size_t)p.T * V;
  const char *xl0 = reinterpret_cast<const char *>(lds + g * RS + r * V);   // lane's gather base (LDS row g, frame r)

  // this wave's DMA pieces of a 16-row slice; LDS row l = 4 q + g holds slice row 4 g + q
  int doff[D3_PW];
#pragma unroll
  for (int i = 0; i < D3_PW; ++i) {
    const int pc = i * NW + wave;
    const int e = pc * 64 + lane;
    const int lrow = e / (RS / 4), c4 = e - lrow * (RS / 4);
    const int row = 4 * (lrow & 3) + (lrow >> 2);
    doff[i] = (pc < TILE_PIECES && e < D3_NV4) ? (int)(((size_t)row * row_stride + 4 * c4) * sizeof(float)) : -1;
  }
  D3B bz[SLOTS];                                      // X[all 64 channels][frame r][joint of the slot]
  D3A aS[2];                                          // two A-operand sets: W_k[16 p + r][all 64 channels]
  f32x4 h;
  // (a lambda around the hook: called directly from the schedule, the force-inlined hook leaves both kernels with the
  // same instructions in another order -- DESIGN.md section 9)
  auto load_a = [&](D3A &a, int k, int ph) { d3_load_a(a, W, k, ph, lane); };

  int tile = blockIdx.x;
  if (tile < p.total_tiles) {       // prologue: slice 0 of the first tile, A operands of the first plane
    const int seq = tile / p.tiles_per_seq, t0 = (tile % p.tiles_per_seq) * D3_F;
    const float *dr = dz + (size_t)seq * 64 * row_stride + (size_t)t0 * V;
#pragma unroll
    for (int i = 0; i < D3_PW; ++i)
      if (doff[i] >= 0) tile_dma16(dr, doff[i], lds + (i * NW + wave) * 256);
  }
  load_a(aS[0], d3_plane0[WAVE], 0);

  for (; tile < p.total_tiles; tile += gridDim.x) {
    const int seq = tile / p.tiles_per_seq, t0 = (tile % p.tiles_per_seq) * D3_F;
    const float *dg = dz + (size_t)seq * 64 * row_stride + (size_t)t0 * V;
    const int ntile = tile + gridDim.x;
    const bool has_next = ntile < p.total_tiles;
    const int nseq = has_next ? ntile / p.tiles_per_seq : 0, nt0 = has_next ? (ntile % p.tiles_per_seq) * D3_F : 0;
    const float *ndg = dz + (size_t)nseq * 64 * row_stride + (size_t)nt0 * V;
    D3_TRACE_TILE(tile);
    D3_MARK(0);

    // B operands of the tile: X[4 kk + g][frame r][joint of the slot] for all 64 input channels, register-resident for
    // the whole tile.  They come through LDS: buffer 1 is free between the last phase of one tile and the second of
    // the next, and the four 16-channel slices of X pass through it one after the other as LDS-DMA pieces (whole
    // 1 KB rows per instruction, the layout of the dZ slices: LDS row 4 g + kappa holds slice row 4 kappa + g), each
    // read back with 28 immediate-offset ds_reads per lane (d3_read_x: the float of row kappa, joint j is at
    // xr + (kappa * RS + j) * 4).  Loaded straight from global memory (a 16- or 12-byte run of joints per lane and
    // channel), a load instruction touched ~100 cache lines for 1 KB of data and the 32 of them per wave kept the
    // address path of the CU busy for 15-37 thousand cycles per tile with nothing else to run (cycle trace, round 3).
    {
      float *xb = lds + BUF;
      const char *xr = reinterpret_cast<const char *>(xb + 4 * g * RS + r * V);      // kappa = 0: + kappa * RS floats
      const float *xs = x + (size_t)seq * 64 * row_stride + (size_t)t0 * V;
#pragma unroll
      for (int sl = 0; sl < 4; ++sl) {
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __syncthreads();                                    // nobody reads buffer 1 any more
#pragma unroll
        for (int i = 0; i < D3_PW; ++i)
          if (doff[i] >= 0) tile_dma16(xs + (size_t)sl * 16 * row_stride, doff[i], xb + (i * NW + wave) * 256);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
#pragma unroll
        for (int i = 0; i < SLOTS; ++i)
          if (sj[i] >= 0) d3_read_x(bz[i], xr, sj[i], sl, xscale);
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // the phase-0 barrier follows: buffer 1 is written next
    }

#pragma unroll 1
    for (int ph = 0; ph < 4; ++ph) {
      D3_MARK(1 + 3 * ph);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // own pieces of slice `ph` (and, first phase, the B operands)
      D3_MARK(2 + 3 * ph);
      __syncthreads();
      D3_MARK(3 + 3 * ph);
      float *buf_nxt = lds + ((ph + 1) & 1) * BUF;
      const char *xl = xl0 + (ph & 1) * BUF * sizeof(float);
      const bool copy = ph + 1 < 4 || has_next;
      const float *src = (ph + 1 < 4) ? dg + (size_t)(ph + 1) * 16 * row_stride : ndg;
      auto dma_piece = [&](int i) {
        if (doff[i] >= 0) tile_dma16(src, doff[i], buf_nxt + (i * NW + wave) * 256);
      };
      if constexpr (WAVE == 0) { D3_BODY_0 } else if constexpr (WAVE == 1) { D3_BODY_1 }
      else if constexpr (WAVE == 2) { D3_BODY_2 } else if constexpr (WAVE == 3) { D3_BODY_3 }
      else if constexpr (WAVE == 4) { D3_BODY_4 } else if constexpr (WAVE == 5) { D3_BODY_5 }
      else if constexpr (WAVE == 6) { D3_BODY_6 } else { D3_BODY_7 }
    }
    D3_MARK(13);
  }
}

__global__ __launch_bounds__(D3_NW * 64, 2) void D3_KERNEL(D3Params p, const float *__restrict__ x,
                                                           const float *__restrict__ dz, const D3W *__restrict__ W,
                                                           float *__restrict__ dcoef_partial) {
  extern __shared__ float lds[];
  float *dcs = lds + 2 * D3_BUF;
  const int tid = threadIdx.x;
  for (int e = tid; e < p.ltot * D3_V; e += D3_NW * 64) dcs[e] = 0.f;
  float xscale, inv;
  d3_scales(p, xscale, inv);      // in front of the barrier (behind it: same instructions in another order)
  __syncthreads();
  switch (__builtin_amdgcn_readfirstlane(tid >> 6)) {
    case 0: d3_wave_main<0>(p, lds, x, dz, W, xscale); break;
    case 1: d3_wave_main<1>(p, lds, x, dz, W, xscale); break;
    case 2: d3_wave_main<2>(p, lds, x, dz, W, xscale); break;
    case 3: d3_wave_main<3>(p, lds, x, dz, W, xscale); break;
    case 4: d3_wave_main<4>(p, lds, x, dz, W, xscale); break;
    case 5: d3_wave_main<5>(p, lds, x, dz, W, xscale); break;
    case 6: d3_wave_main<6>(p, lds, x, dz, W, xscale); break;
    default: d3_wave_main<7>(p, lds, x, dz, W, xscale); break;
  }
  __syncthreads();
  float *out = dcoef_partial + (size_t)blockIdx.x * p.ltot * D3_V;
  for (int e = tid; e < p.ltot * D3_V; e += D3_NW * 64) out[e] = dcs[e] * inv;
}

// What the two entry points check and do in common (each refuses its own operands first): the shape the schedule was
// generated for, whole tiles, dz as 16-byte DMA pieces, the LDS budget; N == 0 is a memset; else the launch.
int d3_launch(int N, int T, int V, int K, int ltot, const float *x, const float *dz, const D3W *W, int n_blocks,
              float *dcoef_partial, void *stream, const D3Extra &extra) {
  if (N < 0 || T <= 0 || V != D3_V || K != G3_K || ltot <= 0 || n_blocks < 1) return P2R_EINVAL;
  if (T % D3_F != 0 || ((uintptr_t)dz % 16) != 0) return P2R_EINVAL;
  if (N == 0) return hipMemsetAsync(dcoef_partial, 0, (size_t)n_blocks * ltot * V * sizeof(float), p2r_stream(stream));
  D3Params p;
  static_cast<D3Extra &>(p) = extra;
  p.T = T; p.ltot = ltot;
  p.tiles_per_seq = T / D3_F;
  const long long tiles = (long long)N * p.tiles_per_seq;
  if (tiles > 0x7fffffffLL) return P2R_EINVAL;
  p.total_tiles = (int)tiles;
  const size_t lds = (size_t)2 * D3_BUF * sizeof(float) + (size_t)ltot * V * sizeof(float);
  if (lds > 160 * 1024) return P2R_EINVAL;
  return p2r_launch_big_lds<D3_KERNEL>(n_blocks, D3_NW * 64, lds, stream, p, x, dz, W, dcoef_partial);
}

}  // namespace
