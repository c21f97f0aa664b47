// What the conv sources (conv_fwd.hip, conv_halo.hip, conv_level0.hip, conv_pack.hip, conv_wgrad.hip) share: the
// geometry struct every conv kernel takes, the tap -> input pixel map, the packed-weight layout, the epilogue loads,
// the tile constants the forward planner reads, and the launchers conv_fwd_launch calls in the other sources.
#pragma once
#include "common.h"
#include "cesm_hip.h"

namespace {

struct ConvGeom {
  int Nb, Hi, Wi, Ho, Wo;
  int C1, C2;       // input channels from source 1 / source 2 (concat on channel axis)
  int Cout, Co1;    // output channels; [0,Co1) -> y1, [Co1,Cout) -> y2
  int KH, KW, S, P, U;
  int wch = 0;      // packed weights in the chunked layout (wpk_chunked)
};

__device__ __forceinline__ bool tap_src(const ConvGeom& g, int oy, int ox, int ky, int kx, int& iy, int& ix) {
  int ny = oy * g.S - g.P + ky;
  int nx = ox * g.S - g.P + kx;
  if (g.U != 1) {
    if ((ny % g.U) != 0 || (nx % g.U) != 0) return false;  // negative remainders are non-zero too
    ny /= g.U;
    nx /= g.U;
  }
  iy = ny;
  ix = nx;
  return (unsigned)ny < (unsigned)g.Hi && (unsigned)nx < (unsigned)g.Wi;
}

// Packed conv weights (cesm_conv_pack): row-major Wp[co][tap][ci], or -- bf16 3x3 / 4x4 weights with Cout % 64 == 0 and
// Cin % 32 == 0, the operands of the halo convs -- "chunked": one contiguous block per (64-co block, 32-channel chunk)
// holding [tap][co % 64][ci % 32]: the weight tile a halo conv stages per K step is one contiguous block (3x3) or
// 4-KB runs per live tap (4x4 stride-2), where the row-major layout gave 64-B pieces at a stride of Cin * 2 bytes.
// The halo conv micro ran 7-22 % faster at levels 1-3, the step's halo conv calls 2-8 % (profiles/r6late_h3_*.txt).
__host__ __device__ inline bool wpk_chunked(bool bf16_dtype, int Cout, int Cin, int KH, int KW) {
  return bf16_dtype && ((KH == 3 && KW == 3) || (KH == 4 && KW == 4)) && Cout % 64 == 0 && Cin % 32 == 0;
}
__host__ __device__ inline int64_t wpk_index(bool chunked, int co, int tap, int ci, int Cin, int NT) {
  if (!chunked) return ((int64_t)co * NT + tap) * Cin + ci;
  return ((((int64_t)(co >> 6) * (Cin >> 5) + (ci >> 5)) * NT + tap) * 64 + (co & 63)) * 32 + (ci & 31);
}

// ----------------------------------------------------------------------------------------
// Conv epilogue loads, issued together and unpredicated.  Under lane predicates (pixel valid,
// channel half, residual present) every bias / residual load became a branch with its own
// vmcnt(0), i.e. one full memory round trip per (pixel group, channel tile) in sequence.
// ----------------------------------------------------------------------------------------
__device__ __forceinline__ void epi_bias(const float* __restrict__ bias, int co, float (&bv)[4]) {
  if (bias) {  // uniform (kernel argument)
    load4(bias + co, bv);
  } else {
    bv[0] = bv[1] = bv[2] = bv[3] = 0.f;
  }
}
// residual of output pixel m (ok: inside the image), channels co..co+3, from res (co < Co1) or res2;
// kept as raw bf16 (2 registers) until the epilogue adds it
__device__ __forceinline__ bf16x4 epi_res(const bf16* __restrict__ res, const bf16* __restrict__ res2, int64_t m, int co,
                                          int Co1, int Co2, bool ok) {
  const bool first = co < Co1;
  const bf16* rp = first ? res : res2;
  const bool use = ok && rp != nullptr;
  const bf16* base = use ? rp : (res ? res : res2);  // some valid address; the value is discarded
  const int64_t off = use ? (first ? m * Co1 + co : m * Co2 + (co - Co1)) : 0;
  const bf16x4 t = *reinterpret_cast<const bf16x4*>(base + off);
  return use ? t : bf16x4{};
}
__device__ __forceinline__ float b2f(bf16x4 v, int r) { return (float)v[r]; }

// Tile constants the forward planner (conv_fwd.hip) reads; the kernels that own them are in conv_halo.hip (H3_*) and
// conv_level0.hip (CP_*, WS_*)
constexpr int H3_TH = 8, H3_TW = 32;     // halo conv: default tile (TH x TW is chosen per level: c2_tile, h3_big_tile)
constexpr int H3_BN = 64;                // halo conv: output channels per block
constexpr int CP_TH = 14;                // conv3x3p: max tile rows: (14 + 2) * 40 = 640 halo rows
constexpr int WS_MAXTH = 8;              // conv3x3ws: tile rows: (8 + 2) * 40 = 400 halo rows
constexpr int WS_PIX = 256;              // conv3x3ws: pixels per item (4 waves x 4 groups of 16)

}  // namespace

// Arguments of the launchers below.  conv_fwd_launch (conv_fwd.hip) plans every forward conv and launches the generic
// and 1x1 kernels itself; the halo and level-0 kernels live in other sources, where ConvGeom (local to each source) cannot
// cross, so their launchers take this plain struct and fill a ConvGeom of their own.  All of them are bf16.
struct ConvLaunchArgs {
  const bf16 *x1, *x2, *wp;
  const float* bias;
  const bf16 *res, *res2;
  bf16 *y1, *y2;
  int Nb, Hi, Wi, Ho, Wo, C1, C2, Cout, Co1, KH, KW, S, P, U;
  int TH, TW;       // the plan's tile
  float* gnp;       // GroupNorm statistics partials (cesm_conv_fwd_gn), or null
  int gn_fimg;      // images per sample of the partials
  int* queue;       // work queue of conv3x3ws
  hipStream_t stream;
};

namespace {
inline ConvGeom conv_geom(const ConvLaunchArgs& a) {
  ConvGeom g{a.Nb, a.Hi, a.Wi, a.Ho, a.Wo, a.C1, a.C2, a.Cout, a.Co1, a.KH, a.KW, a.S, a.P, a.U};
  g.wch = wpk_chunked(true, a.Cout, a.C1 + a.C2, a.KH, a.KW);
  return g;
}
}  // namespace

// Not part of the ABI: hidden, so the library's dynamic symbols stay exactly the cesm_* of cesm_hip.h.
#pragma GCC visibility push(hidden)
void conv_halo3_launch(const ConvLaunchArgs& a);  // conv_halo.hip: conv3x3_bf16_kernel (CFV_HALO*)
void conv_s2_launch(const ConvLaunchArgs& a);     // conv_halo.hip: convs2_bf16_kernel (CFV_S2*)
void conv_p32_launch(const ConvLaunchArgs& a);    // conv_level0.hip: conv3x3p_kernel (CFV_P32_RW)
void conv_ws_launch(const ConvLaunchArgs& a);     // conv_level0.hip: conv3x3ws_kernel (CFV_WS*)
#pragma GCC visibility pop
