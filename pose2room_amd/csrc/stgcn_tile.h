// stgcn_tile.h -- the tile skeleton shared by the 53-joint ST-GCN kernels of the second and third generation
// (stgcn_gcn2 / gcn3 / gcn3_dw / tconv2 / tconv3; gcn3_grad / gcn3h_grad, whose common body is stgcn_gcn3_dcoef_body.h;
// gcn3h_fwd / gcn3h_dx, whose common body is stgcn_gcn3h_body.h), gfx950.
//
// The skeleton: a tile of 16 frames x 53 joints, LDS rows of 16 * 53 = 848 floats (848 == 16 mod 32: the two channel
// rows of a 32-lane read group use disjoint banks); the 64 input channels in four phases of 16 rows through two slice
// buffers; a slice = 53 LDS-DMA pieces of 1 KB, dealt round-robin to 8 waves (7 per wave); up to 7 accumulator slots
// (joints) per wave; A operands in the order [plane][phase][m-tile][lane][4].  Everything here is force-inlined into
// its caller: no translation unit, kernel or ABI entry of its own.
//
// Kept per kernel ("Which generation serves what", has the reasons): the per-wave piece table, the
// accumulator start from the bias table, the staged row epilogue and the (count, mean, M2) merge; the three-tap window
// of tconv3 and every assembly string that names a register (tools/check_reserved_vgprs.py reads the .hip sources,
// not their headers).
#pragma once
#include "p2r_common.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

constexpr int TILE_V = 53;                    // joints of the skeleton
constexpr int TILE_F = 16;                    // frames per tile = columns of an MFMA n-tile
constexpr int TILE_CP = 16;                   // channels per phase
constexpr int TILE_NPH = 4;                   // phases (64 channels)
constexpr int TILE_NW = 8;                    // waves per workgroup
constexpr int TILE_SLOTS = 7;                 // accumulator slots (joints) per wave
constexpr int TILE_RS = TILE_F * TILE_V;      // LDS row stride (floats): 848 == 16 (mod 32)
constexpr int TILE_BUF = TILE_CP * TILE_RS;   // floats per 16-row slice
// piece arithmetic of a slice / tile of nv4 float4 elements: 64-lane pieces of 1 KB, round-robin over the waves
constexpr int tile_pieces(int nv4) { return (nv4 + 63) / 64; }
constexpr int tile_pw(int nv4) { return (tile_pieces(nv4) + TILE_NW - 1) / TILE_NW; }
constexpr int TILE_NV4 = TILE_BUF / 4;               // 3392 = 53 pieces of 64
constexpr int TILE_PIECES = tile_pieces(TILE_NV4);   // 53: piece i of wave w = float4 elements (i * 8 + w) * 64 + lane
constexpr int TILE_PW = tile_pw(TILE_NV4);           // 7 per wave
static_assert(TILE_RS % 32 == 16 && TILE_PIECES * 64 == TILE_NV4 && TILE_PW == 7, "tile geometry");

// ---- LDS-DMA -------------------------------------------------------------------------------------------------------
// Pieces as inline assembly: with the builtin, hipcc treats every later LDS read as possibly aliasing the copy in
// flight and puts `s_waitcnt vmcnt(0)` in front of it -- which would stall every operand fetch on the piece just
// issued.  The copies land in the buffer nobody reads during the current phase; the issuing wave waits for them
// (vmcnt(0)) right before the phase barrier.  M0 = LDS destination of lane 0 (saved and restored); a piece is 64 lanes
// x 16 (or 4) bytes, lane l landing at dst + 16 l (4 l).
__device__ __forceinline__ unsigned tile_lds_addr(const float *p) {
  return (unsigned)(size_t)(const __attribute__((address_space(3))) float *)p;
}
// flat form: a 64-bit address per lane (gcn2, tconv2: ragged tiles compute their addresses piece by piece)
__device__ __forceinline__ void tile_dma16(const float *src, float *lds_dst) {
  unsigned keep;
  const unsigned dst = __builtin_amdgcn_readfirstlane(tile_lds_addr(lds_dst));
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
               : "=&s"(keep) : "v"(src), "s"(dst) : "memory");
}
__device__ __forceinline__ void tile_dma4(const float *src, float *lds_dst) {
  unsigned keep;
  const unsigned dst = __builtin_amdgcn_readfirstlane(tile_lds_addr(lds_dst));
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dword %1, off\n\ts_mov_b32 m0, %0"
               : "=&s"(keep) : "v"(src), "s"(dst) : "memory");
}
// scalar form: wave-uniform base + per-lane byte offset (every statically scheduled kernel: the offsets of a wave's
// pieces are computed once per kernel)
__device__ __forceinline__ void tile_dma16(const float *base, unsigned voff, float *lds_dst) {
  unsigned keep;
  const unsigned dst = __builtin_amdgcn_readfirstlane(tile_lds_addr(lds_dst));
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2\n\ts_mov_b32 m0, %0"
               : "=&s"(keep) : "v"(voff), "s"(base), "s"(dst) : "memory");
}

// ---- operands --------------------------------------------------------------------------------------------------------
// A operands of (plane k, phase ph) in the permuted-plane layout W'[k][ph][m][lane][s]: four 16-byte loads per lane,
// 1 KB contiguous per wave and m-tile
__device__ __forceinline__ void tile_load_a(float (&a)[4][4], const float *Wp, int k, int ph, int lane) {
  const float4 *wp = reinterpret_cast<const float4 *>(Wp) + ((size_t)(k * TILE_NPH + ph) * 4) * 64 + lane;
#pragma unroll
  for (int m = 0; m < 4; ++m) {
    const float4 u = wp[m * 64];
    a[m][0] = u.x; a[m][1] = u.y; a[m][2] = u.z; a[m][3] = u.w;
  }
}

// ---- end of the kernel: the per-wave statistics entries rowstat[NW][64][ST] -> one row of stats_partial, as plain
// sums [64][2] (the BatchNorm-backward launches; every launch of the second generation with ST = 2)
template <int ST>
__device__ __forceinline__ void tile_write_sums(const float *rowstat, float *stats_partial, int tid) {
  if (tid < 128) {
    float t = 0.f;
#pragma unroll
    for (int w = 0; w < TILE_NW; ++w) t += rowstat[(w * 64 + (tid >> 1)) * ST + (tid & 1)];
    stats_partial[(size_t)blockIdx.x * 128 + tid] = t;
  }
}
