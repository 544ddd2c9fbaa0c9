// stgcn_gcn3_grad.hip -- adjacency gradient of the fused graph convolution, statically scheduled (gfx950).
//
//   dcoef[k][j][v] = sum over (n, t, c) of Y_k[c, t, v] * dZ[c, t, w_j(k, v)],     Y_k = W_k . X
// at the non-zero entries (k, v, w_j) of the adjacency (the gradient reaching `A * importance`,
// reference models/p2rnet/modules/stgcn.py:134 / stgcn_layers.py:62-65 through autograd) -- the operator of
// gcn_dcoef_kernel in stgcn_gcn.hip, rebuilt on the skeleton of stgcn_gcn3.hip:
//
//   * MFMA n-tile = 16 frames of ONE joint v (no gather on the MFMA side at all: the B operand of the product
//     Y_k(v) = W_k . X(v) is X itself).  A wave owns up to 7 joints and keeps their B operands -- all 64 input channels
//     of 16 frames -- in registers for the whole tile (16 VGPRs per joint, loaded once per tile straight from HBM/L2).
//   * The product is split along its OUTPUT rows: phase p computes rows 16p..16p+15 of Y_k(v) (16 k-steps into one
//     4-register tile) and reduces them at once against rows 16p..16p+15 of dZ at the row-list joints -- so of dZ
//     only a 16-row slice has to be resident (two 53 KB LDS buffers, filled by LDS-DMA like the X slices of the
//     forward kernel), and nothing of size 64 rows x tile ever is.  The slice is stored with its rows permuted
//     (LDS row 4q+g holds row 4g+q) so that the accumulator layout of the MFMA (lane (g, r) holds rows 4g..4g+3 of
//     frame r) reads it bank-conflict-free with immediate offsets.
//   * The (plane, joint) units of the ROW lists that are empty (214 of 583) are skipped exactly; the work list is
//     code generated at build time (tools/gen_gcn_sched.py, D3_BODY_<wave>), as in stgcn_gcn3.hip.
//   * Each product is reduced over the wave with DPP row sums + two lane swaps; one lane accumulates it into the
//     workgroup's LDS table [ltot][V] (owned entries: no contention), written out once per workgroup.
#include "stgcn_tile.h"

// Cycle trace (profiling hook, off in the product build; see stgcn_tconv3.hip): -DP2R_CYCLE_TRACE, tools/dev_g3_trace.py
#ifdef P2R_CYCLE_TRACE
__device__ unsigned long long d3_trace[8 * 32];
#define D3_TRACE_TILE(tile) const bool trace_on = blockIdx.x == 7 && (tile) == 7 + 3 * (int)gridDim.x
#define D3_MARK(i) do { if (trace_on && lane == 0) d3_trace[wave * 32 + (i)] = __builtin_readcyclecounter(); } while (0)
#endif
#define D3_KERNEL gcn3_dcoef_kernel
namespace {

// what stgcn_gcn3_dcoef_body.h asks of this file
typedef float D3A[16];            // W_k[16 p + r][4 kk + g], kk = 0..15 (plain arrays: the assembly takes single registers)
typedef float D3B[16];            // X[4 kk + g][frame r][joint of the slot]
typedef float D3W;
struct D3Extra {};
constexpr bool D3_FENCED = true;
__device__ __forceinline__ void d3_scales(const D3Extra &, float &xscale, float &inv) { xscale = 1.f; inv = 1.f; }
__device__ __forceinline__ void d3_copy_a(D3A &dst, const D3A &src) {
#pragma unroll
  for (int e = 0; e < 16; ++e) dst[e] = src[e];
}

// Y tile of one (plane, joint) unit: 16 k-steps (all 64 input channels) into ONE accumulator; the first MFMA starts
// from the inline constant 0.  Two assembly blocks of 8 (operand-count limit of one asm statement).
__device__ __forceinline__ void d3_product(f32x4 &h, const D3A &a, const D3B &b) {
  asm volatile(
      "s_nop 1\n\t"
      "v_mfma_f32_16x16x4_f32 %0, %1, %9, 0\n\tv_mfma_f32_16x16x4_f32 %0, %2, %10, %0\n\t"
      "v_mfma_f32_16x16x4_f32 %0, %3, %11, %0\n\tv_mfma_f32_16x16x4_f32 %0, %4, %12, %0\n\t"
      "v_mfma_f32_16x16x4_f32 %0, %5, %13, %0\n\tv_mfma_f32_16x16x4_f32 %0, %6, %14, %0\n\t"
      "v_mfma_f32_16x16x4_f32 %0, %7, %15, %0\n\tv_mfma_f32_16x16x4_f32 %0, %8, %16, %0"
      : "=&v"(h)
      : "v"(a[0]), "v"(a[1]), "v"(a[2]), "v"(a[3]), "v"(a[4]), "v"(a[5]), "v"(a[6]), "v"(a[7]),
        "v"(b[0]), "v"(b[1]), "v"(b[2]), "v"(b[3]), "v"(b[4]), "v"(b[5]), "v"(b[6]), "v"(b[7]));
  asm volatile(
      "v_mfma_f32_16x16x4_f32 %0, %1, %9, %0\n\tv_mfma_f32_16x16x4_f32 %0, %2, %10, %0\n\t"
      "v_mfma_f32_16x16x4_f32 %0, %3, %11, %0\n\tv_mfma_f32_16x16x4_f32 %0, %4, %12, %0\n\t"
      "v_mfma_f32_16x16x4_f32 %0, %5, %13, %0\n\tv_mfma_f32_16x16x4_f32 %0, %6, %14, %0\n\t"
      "v_mfma_f32_16x16x4_f32 %0, %7, %15, %0"
      : "+v"(h)
      : "v"(a[8]), "v"(a[9]), "v"(a[10]), "v"(a[11]), "v"(a[12]), "v"(a[13]), "v"(a[14]), "v"(a[15]),
        "v"(b[8]), "v"(b[9]), "v"(b[10]), "v"(b[11]), "v"(b[12]), "v"(b[13]), "v"(b[14]), "v"(b[15]));
  // the last one through the builtin: the compiler then knows that `h` comes out of the matrix pipe and provides
  // the MFMA -> VALU wait states itself (filling them with independent instructions where it can)
  h = __builtin_amdgcn_mfma_f32_16x16x4f32(a[15], b[15], h, 0, 0, 0);
}

__device__ __forceinline__ void d3_load_a(D3A &a, const float *__restrict__ Wp, int k, int ph, int lane) {
  // forward planes in kernel order: Wp[k][ph'][m][lane][s] = W_k[16 m + r][16 ph' + 4 s + g]; here m = ph, kk = 4 ph' + s
#pragma unroll
  for (int pp = 0; pp < 4; ++pp) {
    const float4 u = reinterpret_cast<const float4 *>(Wp)[((size_t)(k * 4 + pp) * 4 + ph) * 64 + lane];
    a[4 * pp + 0] = u.x; a[4 * pp + 1] = u.y; a[4 * pp + 2] = u.z; a[4 * pp + 3] = u.w;
  }
}
// slice sl = channels 16 sl + 4 kp + g: kk = 4 sl + kp
__device__ __forceinline__ void d3_read_x(D3B &b, const char *xr, int joint, int sl, float) {
#pragma unroll
  for (int kp = 0; kp < 4; ++kp) b[4 * sl + kp] = *reinterpret_cast<const float *>(xr + (kp * TILE_RS + joint) * 4);
}

}  // namespace
#include "stgcn_gcn3_dcoef_body.h"

#ifdef P2R_CYCLE_TRACE
extern "C" int p2r_debug_d3_trace(unsigned long long *dst) {
  return (int)hipMemcpyFromSymbol(dst, HIP_SYMBOL(d3_trace), sizeof(d3_trace));
}
#endif

// Adjacency gradient at the row-list entries, statically scheduled for the P2RNet skeleton (the caller checks
// p2r_stgcn_gcn3_signature(1) against its row tables first).
//   x   (N,64,T,53): input of the graph conv            dz (N,64,T,53): gradient of its output
//   Wp  [K][4][4][64][4]: the forward planes in kernel order (as for p2r_stgcn_gcn3_forward, form 0)
//   dcoef_partial [n_blocks][ltot][53]: per-workgroup sums in the layout of the row coefficient table
//     (entry (lofs_k + j, v) <-> A[k][v][w_j(k, v)]); padded slots stay 0; the caller sums over the leading axis.
// T % 16 == 0 and x, dz 16-byte aligned (P2R_EINVAL otherwise: use p2r_stgcn_gcn_coef_grad).
extern "C" int p2r_stgcn_gcn3_coef_grad(int N, int T, int V, int K, int ltot, const float *x, const float *dz,
                                        const float *Wp, int n_blocks, float *dcoef_partial, void *stream) {
  if (T > (1 << 20) || ((uintptr_t)x % 4) != 0) return P2R_EINVAL;
  return d3_launch(N, T, V, K, ltot, x, dz, Wp, n_blocks, dcoef_partial, stream, D3Extra{});
}
