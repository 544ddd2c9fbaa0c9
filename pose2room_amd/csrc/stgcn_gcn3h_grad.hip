// stgcn_gcn3h_grad.hip -- adjacency gradient of the fused graph convolution in `split16` arithmetic (opt-in mode;
// split16.h), statically scheduled (gfx950).  Same operator, work list and data movement as stgcn_gcn3_grad.hip:
//
//   dcoef[k][j][v] = sum over (n, t, c) of Y_k[c, t, v] * dZ[c, t, w_j(k, v)],     Y_k = W_k . X
// at the non-zero entries (k, v, w_j) of the adjacency (reference models/p2rnet/modules/stgcn.py:134 /
// stgcn_layers.py:62-65 through autograd).  What changes is the MFMA product Y_k(v) = W_k . X(v) -- 16 output rows x 16
// frames, K = the 64 input channels: SIX v_mfma_f32_16x16x32_f16 (two k-steps x three products of two-part fp16 operands,
// 96 matrix-pipe cycles) instead of SIXTEEN v_mfma_f32_16x16x4_f32 (512 cycles).  The reduction of the product against
// the gathered dZ rows stays what it was -- fp32 vector arithmetic on the fp32 dZ slice, so the heavy tail of the
// gradient never meets fp16 -- and now runs BESIDE the matrix pipe instead of in its issue slots: on gfx950 an fp32 MFMA
// issues through the vector datapath, a 16-bit one does not (tools/ubench/mfma16_valu_overlap.hip).  The exact kernel
// spent 21 % of its wave time waiting with the matrix pipe 64 % busy; here the vector reduction is the critical path.
//   * B operands (X of the wave's joints, register-resident for a tile) are converted to fp16 parts when they are read
//     from the staging slices: 16 registers per joint, as before.  K index (kg, i) of a k-step ks <-> channel
//     32 ks + 16 (i >> 2) + 4 (i & 3) + kg: the slices' LDS layout and read pattern of the exact kernel serve unchanged.
//   * A operands arrive pre-split from the host (prepare_chain) in that K order: Wd[k][ph][part][ks][lane][8].
//   * X is scaled by the power of two of its range word when it is converted, W by its own; the products are scaled back
//     when the workgroup's table is written out.
// MFMAs through the builtin (the exact kernel's two assembly blocks are gone).
#include "stgcn_tile.h"
#include "split16.h"

// (d3_reduce indexes small arrays behind compile-time conditions that the front end does not fold before it warns)
#pragma clang diagnostic ignored "-Warray-bounds"

#define D3_KERNEL gcn3h_dcoef_kernel
namespace {

// what stgcn_gcn3_dcoef_body.h asks of this file
struct D3A { p2r_h8 p[2], q[2]; };            // [k-step]: parts of W_k rows 16 ph + r
struct D3B { p2r_h8 p[2], q[2]; };            // [k-step]: parts of X (channels of the k-step, frame r, the slot's joint)
typedef p2r_h8 D3W;
struct D3Extra {
  const unsigned *x_amax;
  const float *winv;
};
#ifdef D3_NO_FENCE                            // ablation: the compiler may move the reduction across the product
constexpr bool D3_FENCED = false;
#else
constexpr bool D3_FENCED = true;
#endif
__device__ __forceinline__ void d3_scales(const D3Extra &e, float &xscale, float &inv) {
  float xinv;
  p2r_split_scale(e.x_amax, xscale, xinv);
  inv = xinv * e.winv[0];                     // the products carry 2^(S_x + S_w)
}
__device__ __forceinline__ void d3_copy_a(D3A &dst, const D3A &src) { dst = src; }

// Y tile of one (plane, joint) unit: two k-steps (all 64 input channels) x three products into ONE accumulator
__device__ __forceinline__ void d3_product(f32x4 &h, const D3A &a, const D3B &b) {
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int ks = 0; ks < 2; ++ks) {
    acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(a.p[ks], b.q[ks], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(a.q[ks], b.p[ks], acc, 0, 0, 0);
  }
#pragma unroll
  for (int ks = 0; ks < 2; ++ks) acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(a.p[ks], b.p[ks], acc, 0, 0, 0);
  h = acc;
}

__device__ __forceinline__ void d3_load_a(D3A &a, const p2r_h8 *__restrict__ Wd, int k, int ph, int lane) {
  // Wd[k][ph][part][ks][lane] (16 bytes each)
  const p2r_h8 *wd = Wd + ((size_t)(k * 4 + ph) * 2 * 2) * 64 + lane;
  a.p[0] = wd[0]; a.p[1] = wd[64]; a.q[0] = wd[128]; a.q[1] = wd[192];
}
// slice sl = channels 16 sl + 4 kp + g: K values i = 4 (sl & 1) + kp of k-step sl >> 1 (see the top)
__device__ __forceinline__ void d3_read_x(D3B &b, const char *xr, int joint, int sl, float xscale) {
  float v4[4];
#pragma unroll
  for (int kp = 0; kp < 4; ++kp) v4[kp] = *reinterpret_cast<const float *>(xr + (kp * TILE_RS + joint) * 4) * xscale;
#pragma unroll
  for (int kp = 0; kp < 4; kp += 2) {
    p2r_f2 xx = {v4[kp], v4[kp + 1]};
    asm volatile("" : "+v"(xx));                  // the split sees VALUES (split16.h)
    const p2r_h2 ph_ = __builtin_convertvector(xx, p2r_h2);
    const p2r_h2 qh_ = __builtin_convertvector(xx - __builtin_convertvector(ph_, p2r_f2), p2r_h2);
    b.p[sl >> 1][4 * (sl & 1) + kp] = ph_.x; b.p[sl >> 1][4 * (sl & 1) + kp + 1] = ph_.y;
    b.q[sl >> 1][4 * (sl & 1) + kp] = qh_.x; b.q[sl >> 1][4 * (sl & 1) + kp + 1] = qh_.y;
  }
}

}  // namespace
#include "stgcn_gcn3_dcoef_body.h"

// Adjacency gradient at the row-list entries in split16 arithmetic: arguments and result of p2r_stgcn_gcn3_coef_grad with
//   Wd     fp16 [K][4 ph][2 parts][2 ks][64 lanes][8]: the parts of 2^S_w W_k (forward planes) in A-operand order,
//          Wd[k][ph][part][ks][16 kg + r][i] = part of 2^S_w W_k[16 ph + r][32 ks + 16 (i >> 2) + 4 (i & 3) + kg]
//   winv   device float 2^-S_w;   x_amax: range word of x (NULL: scale 1).  dz is used in fp32 (no range word).
extern "C" int p2r_stgcn_gcn3h_coef_grad(int N, int T, int V, int K, int ltot, const float *x, const float *dz,
                                         const void *Wd, const float *winv, int n_blocks, float *dcoef_partial,
                                         const unsigned *x_amax, void *stream) {
  if (!Wd || !winv || T > (1 << 19) || ((uintptr_t)x % 16) != 0 || ((uintptr_t)Wd % 16) != 0) return P2R_EINVAL;
  if (n_blocks > 65535) return P2R_EINVAL;                    // as p2r_stgcn_gcn3h_weight_grad: one partial row per workgroup
  return d3_launch(N, T, V, K, ltot, x, dz, reinterpret_cast<const p2r_h8 *>(Wd), n_blocks, dcoef_partial, stream,
                   D3Extra{x_amax, winv});
}
