// Implicit-GEMM convolutions on MFMA for the video_net U-Net (all convs are per-frame
// (1,k,k), so the frame axis folds into the batch: Nb = B*F "images").
//
// Activations are channels-last [Nb][H][W][C].  One generic forward kernel covers every
// conv in the net and every data-gradient (replaces ATen conv3d / conv_transpose3d at
// video_net.py:215 (Block.proj), :246 (res_conv), :61-62 (Downsample), :65-66 (Upsample),
// :380/:381 + :322/:323 (attention projections, as 1x1 convs), and their dgrads):
//
//   out[m=(n,oy,ox)][co] = bias[co] + res[m][co]
//                        + sum_{ky,kx,ci} W[co][ky*KW+kx][ci] * X[n][iy][ix][ci]
//   iy = (oy*S - P + ky) / U   (only when (oy*S - P + ky) % U == 0), likewise ix.
//
// U = 1 is an ordinary strided conv; U = 2 with flipped taps is a stride-2 transposed conv.
// The GEMM is computed transposed (D = W * X^T) so each lane's accumulator holds 4
// consecutive output channels of one pixel -> vectorised channels-last stores.
//
// This source: the generic fp32 / bf16 kernels, the 1x1 GEMM, and the forward planner (conv_fwd_plan) with its launch
// switch (conv_fwd_launch) and ABI entries.  The kernels the plan picks for particular shapes are in conv_halo.hip (3x3
// stride 1 and 4x4 stride 2, halo-tiled) and conv_level0.hip (the two persistent level-0 kernels), reached through the
// launchers declared in conv_common.h.  Weight packing: conv_pack.hip.  Weight gradients and the column sums:
// conv_wgrad.hip.  Stem and head: stem_head.hip.
#include "conv_common.h"

namespace {

// ----------------------------------------------------------------------------------------
// forward / dgrad kernel
// ----------------------------------------------------------------------------------------
constexpr int BK = 32;       // K per staging step (channels of one tap)
constexpr int BMP = 128;     // pixels per block

template <typename T> struct KCfg;
template <> struct KCfg<float> { static constexpr int VEC = 4; static constexpr int LDW = 36; };  // 144-B rows

// PAR (U = 2, S = 1, even KH/KW, even Ho/Wo): parity-blocked transposed conv.  Output pixels with
// (oy, ox) = (2a + py, 2b + px) only receive taps ky = (P - py) mod 2 + 2i, kx = (P - px) mod 2 + 2j,
// so each block holds pixels of ONE parity class (blockIdx.y = parity * bpp + tile; M = pixels per
// class) and loops over its KH*KW/4 live taps instead of all KH*KW (3/4 of which gather zeros).
template <typename T, int BN, bool PAR = false>
__global__ __launch_bounds__(256) void conv_fwd_kernel(const T* __restrict__ x1, const T* __restrict__ x2,
                                                       const T* __restrict__ w, const float* __restrict__ bias,
                                                       const T* __restrict__ res, const T* __restrict__ res2,
                                                       T* __restrict__ y1, T* __restrict__ y2, ConvGeom g,
                                                       int64_t M, int bpp = 0) {
  constexpr int VEC = KCfg<T>::VEC;
  constexpr int LDW = KCfg<T>::LDW;
  constexpr int VPR = BK / VEC;          // vectors per row
  constexpr int RPP = 256 / VPR;         // rows per pass
  constexpr int PX_PASS = BMP / RPP;     // pixel-tile passes per thread
  constexpr int W_PASS = BN / RPP;       // weight-tile passes per thread
  constexpr int TM = BN / 32;            // 16-row co tiles per wave (wave covers BN/2 co)
  constexpr int TN = 4;                  // 16-col pixel tiles per wave (wave covers 64 px)

  __shared__ __attribute__((aligned(16))) T lds[2][(BMP + BN) * LDW];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = tid >> 6;
  const int wr = wid >> 1, wc = wid & 1;
  // grid.x = output-channel tile (fast): the Cout/BN blocks sharing one pixel tile run adjacently,
  // so the im2col tile is re-read from L2 instead of HBM
  const int par = PAR ? (int)blockIdx.y / bpp : 0;
  const int py = par >> 1, px = par & 1;
  const int64_t m0 = (int64_t)(PAR ? (int)blockIdx.y - par * bpp : (int)blockIdx.y) * BMP;
  const int n0 = blockIdx.x * BN;
  const int Cin = g.C1 + g.C2;
  const int csteps = Cin / BK;
  const int ntap = PAR ? (g.KH / 2) * (g.KW / 2) : g.KH * g.KW;
  const int ksteps = ntap * csteps;
  const int ky0 = PAR ? (((g.P - py) % 2) + 2) % 2 : 0;
  const int kx0 = PAR ? (((g.P - px) % 2) + 2) % 2 : 0;
  const int Wg = PAR ? g.Wo / 2 : g.Wo, Hg = PAR ? g.Ho / 2 : g.Ho;  // pixel grid enumerated by m

  // per-thread staging rows
  const int vrow = tid / VPR, vk = (tid % VPR) * VEC;
  int pn[PX_PASS], poy[PX_PASS], pox[PX_PASS];
  bool pval[PX_PASS];
#pragma unroll
  for (int p = 0; p < PX_PASS; ++p) {
    const int64_t m = m0 + vrow + p * RPP;
    pval[p] = m < M;
    const int64_t mm = pval[p] ? m : 0;
    pox[p] = (int)(mm % Wg);
    const int64_t t = mm / Wg;
    poy[p] = (int)(t % Hg);
    pn[p] = (int)(t / Hg);
    if constexpr (PAR) {
      poy[p] = 2 * poy[p] + py;
      pox[p] = 2 * pox[p] + px;
    }
  }

  float xr[PX_PASS][VEC];
  float wreg[W_PASS][VEC];

  auto gload = [&](int ks) {
    const int t = ks / csteps;
    const int c0 = (ks - t * csteps) * BK;
    int ky, kx;
    if constexpr (PAR) {
      const int hw = g.KW / 2;
      ky = ky0 + 2 * (t / hw);
      kx = kx0 + 2 * (t - (t / hw) * hw);
    } else {
      ky = t / g.KW;
      kx = t - ky * g.KW;
    }
    const int tap = ky * g.KW + kx;
    const T* src;
    int cs, cc;
    if (c0 < g.C1) { src = x1; cs = g.C1; cc = c0; } else { src = x2; cs = g.C2; cc = c0 - g.C1; }
#pragma unroll
    for (int p = 0; p < PX_PASS; ++p) {
      int iy, ix;
      if (pval[p] && tap_src(g, poy[p], pox[p], ky, kx, iy, ix)) {
        const T* ptr = src + ((((int64_t)pn[p] * g.Hi + iy) * g.Wi + ix) * cs + cc + vk);
        if constexpr (VEC == 8) load8(ptr, xr[p]); else load4(ptr, xr[p]);
      } else {
#pragma unroll
        for (int i = 0; i < VEC; ++i) xr[p][i] = 0.f;
      }
    }
#pragma unroll
    for (int p = 0; p < W_PASS; ++p) {
      const int co = n0 + vrow + p * RPP;
      const T* ptr = w + wpk_index(g.wch, co, tap, c0 + vk, Cin, g.KH * g.KW);
      if constexpr (VEC == 8) load8(ptr, wreg[p]); else load4(ptr, wreg[p]);
    }
  };
  auto sstore = [&](int buf) {
    T* A = lds[buf];              // weights  [BN][LDW]
    T* B = lds[buf] + BN * LDW;   // pixels   [BMP][LDW]
#pragma unroll
    for (int p = 0; p < W_PASS; ++p) {
      T* d = A + (vrow + p * RPP) * LDW + vk;
      if constexpr (VEC == 8) store8(d, wreg[p]); else store4(d, wreg[p]);
    }
#pragma unroll
    for (int p = 0; p < PX_PASS; ++p) {
      T* d = B + (vrow + p * RPP) * LDW + vk;
      if constexpr (VEC == 8) store8(d, xr[p]); else store4(d, xr[p]);
    }
  };

  f32x4 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  gload(0);
  sstore(0);
  __syncthreads();

  const int lr = lane & 15, lg = lane >> 4;
  for (int ks = 0; ks < ksteps; ++ks) {
    const int buf = ks & 1;
    if (ks + 1 < ksteps) gload(ks + 1);
    const T* A = lds[buf];
    const T* B = lds[buf] + BN * LDW;
    if constexpr (sizeof(T) == 2) {
      bf16x8 af[TM], bfr[TN];
#pragma unroll
      for (int i = 0; i < TM; ++i)
        af[i] = *reinterpret_cast<const bf16x8*>(A + (wr * (BN / 2) + i * 16 + lr) * LDW + lg * 8);
#pragma unroll
      for (int j = 0; j < TN; ++j)
        bfr[j] = *reinterpret_cast<const bf16x8*>(B + (wc * 64 + j * 16 + lr) * LDW + lg * 8);
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[i], bfr[j], acc[i][j], 0, 0, 0);
    } else {
      // fp32: lane holds k = 16h + 4*lg + s; the same permutation on both operands
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        f32x4 af[TM], bfr[TN];
#pragma unroll
        for (int i = 0; i < TM; ++i)
          af[i] = *reinterpret_cast<const f32x4*>(A + (wr * (BN / 2) + i * 16 + lr) * LDW + h * 16 + lg * 4);
#pragma unroll
        for (int j = 0; j < TN; ++j)
          bfr[j] = *reinterpret_cast<const f32x4*>(B + (wc * 64 + j * 16 + lr) * LDW + h * 16 + lg * 4);
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
          for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j)
              acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[i][s], bfr[j][s], acc[i][j], 0, 0, 0);
      }
    }
    if (ks + 1 < ksteps) sstore(buf ^ 1);
    __syncthreads();
  }

  // epilogue: lane holds co = base + 4*lg + r (r=0..3) of pixel m
  const int Co2 = g.Cout - g.Co1;
#pragma unroll
  for (int j = 0; j < TN; ++j) {
    int64_t m = m0 + wc * 64 + j * 16 + lr;
    if (m >= M) continue;
    if constexpr (PAR) {  // class-local index -> output pixel
      const int64_t b = m % Wg, t = m / Wg, a = t % Hg, n = t / Hg;
      m = (n * g.Ho + 2 * a + py) * g.Wo + 2 * b + px;
    }
#pragma unroll
    for (int i = 0; i < TM; ++i) {
      const int co = n0 + wr * (BN / 2) + i * 16 + lg * 4;
      float v[4] = {acc[i][j][0], acc[i][j][1], acc[i][j][2], acc[i][j][3]};
      if (bias) {
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] += bias[co + r];
      }
      if (co < g.Co1) {
        if (res) {
          float rv[4];
          load4(res + m * g.Co1 + co, rv);
#pragma unroll
          for (int r = 0; r < 4; ++r) v[r] += rv[r];
        }
        store4(y1 + m * g.Co1 + co, v);
      } else {
        if (res2) {
          float rv[4];
          load4(res2 + m * Co2 + (co - g.Co1), rv);
#pragma unroll
          for (int r = 0; r < 4; ++r) v[r] += rv[r];
        }
        store4(y2 + m * Co2 + (co - g.Co1), v);
      }
    }
  }
}

// ----------------------------------------------------------------------------------------
// bf16 generic implicit GEMM (strided down-sampling convs, transposed up-sampling convs in parity
// blocks, their data gradients, every conv the halo / 1x1 kernels do not take).  Same tiling and
// tap/parity enumeration as conv_fwd_kernel, but
//   * the im2col and weight tiles stay bf16 in registers (raw 16-B loads: no f32 round trip) and
//     are loaded TWO K-steps ahead (each step is only 16 MFMAs per wave, far shorter than a global
//     load's latency);
//   * LDS rows are 64 B with the 16-B chunk index XORed with bit 2 of the row (conflict-free
//     ds_read_b128 over any 16 consecutive rows; the 80-B padded rows ran 2-3-way conflicted).
// ----------------------------------------------------------------------------------------
__device__ __forceinline__ int gx_off(int row, int ch) { return row * 32 + ((ch ^ ((row >> 1) & 2)) << 3); }

template <int BN, bool PAR = false>
__global__ __launch_bounds__(256) void conv_fwd_bf16_kernel(const bf16* __restrict__ x1, const bf16* __restrict__ x2,
                                                            const bf16* __restrict__ w, const float* __restrict__ bias,
                                                            const bf16* __restrict__ res, const bf16* __restrict__ res2,
                                                            bf16* __restrict__ y1, bf16* __restrict__ y2, ConvGeom g,
                                                            int64_t M, int bpp = 0) {
  constexpr int VPR = BK / 8;            // 16-B vectors per 32-channel row
  constexpr int RPP = 256 / VPR;         // rows per pass
  constexpr int PX_PASS = BMP / RPP;
  constexpr int W_PASS = BN / RPP;
  constexpr int TM = BN / 32;
  constexpr int TN = 4;
  __shared__ __attribute__((aligned(16))) bf16 lds[2][(BMP + BN) * 32];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = tid >> 6;
  const int wr = wid >> 1, wc = wid & 1;
  const int par = PAR ? (int)blockIdx.y / bpp : 0;
  const int py = par >> 1, px = par & 1;
  const int64_t m0 = (int64_t)(PAR ? (int)blockIdx.y - par * bpp : (int)blockIdx.y) * BMP;
  const int n0 = blockIdx.x * BN;
  const int Cin = g.C1 + g.C2;
  const int csteps = Cin / BK;
  const int ntap = PAR ? (g.KH / 2) * (g.KW / 2) : g.KH * g.KW;
  const int ksteps = ntap * csteps;
  const int ky0 = PAR ? (((g.P - py) % 2) + 2) % 2 : 0;
  const int kx0 = PAR ? (((g.P - px) % 2) + 2) % 2 : 0;
  const int Wg = PAR ? g.Wo / 2 : g.Wo, Hg = PAR ? g.Ho / 2 : g.Ho;

  const int vrow = tid / VPR, vch = tid % VPR;
  int pn[PX_PASS], poy[PX_PASS], pox[PX_PASS];
  bool pval[PX_PASS];
#pragma unroll
  for (int p = 0; p < PX_PASS; ++p) {
    const int64_t m = m0 + vrow + p * RPP;
    pval[p] = m < M;
    const int64_t mm = pval[p] ? m : 0;
    pox[p] = (int)(mm % Wg);
    const int64_t t = mm / Wg;
    poy[p] = (int)(t % Hg);
    pn[p] = (int)(t / Hg);
    if constexpr (PAR) {
      poy[p] = 2 * poy[p] + py;
      pox[p] = 2 * pox[p] + px;
    }
  }

  bf16x8 xr[2][PX_PASS], wreg[2][W_PASS];  // two K-steps in flight
  auto gload = [&](int ks, int slot) {
    const int t = ks / csteps;
    const int c0 = (ks - t * csteps) * BK;
    int ky, kx;
    if constexpr (PAR) {
      const int hw = g.KW / 2;
      ky = ky0 + 2 * (t / hw);
      kx = kx0 + 2 * (t - (t / hw) * hw);
    } else {
      ky = t / g.KW;
      kx = t - ky * g.KW;
    }
    const int tap = ky * g.KW + kx;
    const bf16* src;
    int cs, cc;
    if (c0 < g.C1) { src = x1; cs = g.C1; cc = c0; } else { src = x2; cs = g.C2; cc = c0 - g.C1; }
#pragma unroll
    for (int p = 0; p < PX_PASS; ++p) {
      int iy, ix;
      bf16x8 v = {};
      if (pval[p] && tap_src(g, poy[p], pox[p], ky, kx, iy, ix))
        v = *reinterpret_cast<const bf16x8*>(src + ((((int64_t)pn[p] * g.Hi + iy) * g.Wi + ix) * cs + cc + vch * 8));
      xr[slot][p] = v;
    }
#pragma unroll
    for (int p = 0; p < W_PASS; ++p) {
      const int co = n0 + vrow + p * RPP;
      wreg[slot][p] = *reinterpret_cast<const bf16x8*>(w + wpk_index(g.wch, co, tap, c0 + vch * 8, Cin, g.KH * g.KW));
    }
  };
  auto sstore = [&](int buf, int slot) {
    bf16* A = lds[buf];            // weights [BN][32]
    bf16* B = lds[buf] + BN * 32;  // pixels  [BMP][32]
#pragma unroll
    for (int p = 0; p < W_PASS; ++p) *reinterpret_cast<bf16x8*>(A + gx_off(vrow + p * RPP, vch)) = wreg[slot][p];
#pragma unroll
    for (int p = 0; p < PX_PASS; ++p) *reinterpret_cast<bf16x8*>(B + gx_off(vrow + p * RPP, vch)) = xr[slot][p];
  };

  f32x4 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int lr = lane & 15, lg = lane >> 4;
  int aoff[TM], boff[TN];
#pragma unroll
  for (int i = 0; i < TM; ++i) aoff[i] = gx_off(wr * (BN / 2) + i * 16 + lr, lg);
#pragma unroll
  for (int j = 0; j < TN; ++j) boff[j] = BN * 32 + gx_off(wc * 64 + j * 16 + lr, lg);

  // K-steps in pairs so the register slots / LDS buffers are compile-time (a runtime slot index would
  // put the staging arrays in scratch memory)
  auto step = [&](int ks, auto bufc) {
    constexpr int buf = decltype(bufc)::value;
    // registers: slot buf held step ks (already in LDS), slot buf^1 holds step ks+1
    if (ks + 2 < ksteps) gload(ks + 2, buf);
    const bf16* L = lds[buf];
    bf16x8 af[TM], bfr[TN];
#pragma unroll
    for (int i = 0; i < TM; ++i) af[i] = *reinterpret_cast<const bf16x8*>(L + aoff[i]);
#pragma unroll
    for (int j = 0; j < TN; ++j) bfr[j] = *reinterpret_cast<const bf16x8*>(L + boff[j]);
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int j = 0; j < TN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[i], bfr[j], acc[i][j], 0, 0, 0);
    if (ks + 1 < ksteps) sstore(buf ^ 1, buf ^ 1);
    __syncthreads();
  };
  gload(0, 0);
  if (ksteps > 1) gload(1, 1);
  sstore(0, 0);
  __syncthreads();
  for (int ks = 0; ks < ksteps; ks += 2) {
    step(ks, std::integral_constant<int, 0>{});
    if (ks + 1 < ksteps) step(ks + 1, std::integral_constant<int, 1>{});
  }

  const int Co2 = g.Cout - g.Co1;
#pragma unroll
  for (int j = 0; j < TN; ++j) {
    int64_t m = m0 + wc * 64 + j * 16 + lr;
    if (m >= M) continue;
    if constexpr (PAR) {
      const int64_t b = m % Wg, t = m / Wg, a = t % Hg, n = t / Hg;
      m = (n * g.Ho + 2 * a + py) * g.Wo + 2 * b + px;
    }
#pragma unroll
    for (int i = 0; i < TM; ++i) {
      const int co = n0 + wr * (BN / 2) + i * 16 + lg * 4;
      float v[4] = {acc[i][j][0], acc[i][j][1], acc[i][j][2], acc[i][j][3]};
      if (bias) {
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] += bias[co + r];
      }
      if (co < g.Co1) {
        if (res) {
          float rv[4];
          load4(res + m * g.Co1 + co, rv);
#pragma unroll
          for (int r = 0; r < 4; ++r) v[r] += rv[r];
        }
        store4(y1 + m * g.Co1 + co, v);
      } else {
        if (res2) {
          float rv[4];
          load4(res2 + m * Co2 + (co - g.Co1), rv);
#pragma unroll
          for (int r = 0; r < 4; ++r) v[r] += rv[r];
        }
        store4(y2 + m * Co2 + (co - g.Co1), v);
      }
    }
  }
}

// ----------------------------------------------------------------------------------------
// 1x1 conv (bf16) as a GEMM: Y[m][co] = bias[co] + res[m][co] + sum_k X[m][k] W[co][k], X = [x1 | x2]
// concatenated on channels, Y = [y1 | y2] split at Co1.  Block = 128 pixels x BN output channels
// (the co blocks of a pixel tile run back to back on one XCD, sharing its X rows in L2); K in steps of 64
// through two LDS stages filled by buffer-LDS-DMA (128-B rows, 16-B chunk index XORed with row & 7,
// out-of-range rows -> zeros); 4 waves = 2 (co halves) x 2 (64-pixel halves).  The epilogue stages
// (acc + bias) as bf16 pixel rows in LDS and writes them (+ residual) with coalesced 16-B accesses.
// Replaces the generic implicit-GEMM path for every 1x1 conv: attention projections at levels with
// C >= 128, res_conv, and their data gradients.  NS = 1 (K = 64: one LDS stage, 35 KB) runs 4 blocks per
// CU instead of 2: the K = 64 projections (to_qkv 64 -> 768 of the long-window level 0) are output-store
// streams whose per-block load -> MFMA -> store phases need the extra blocks to overlap.  The X buffer
// resource covers the block's own 128 rows only, so M * K is not limited to 2^31 bytes.
// ----------------------------------------------------------------------------------------
constexpr int G1_BM = 128;
// (Measured and removed: non-temporal output stores -- GEMMs 5 % faster alone, whole step unchanged (round 3) and
// within the spread on the F = 120 leg (round 5, profiles/r5f_g1nt_f120_ab.txt); co-block-fastest block order.)
__device__ __forceinline__ int g1_off(int row, int chunk) { return (row << 7) + ((chunk ^ (row & 7)) << 4); }

template <int BN, int NS>
__global__ __launch_bounds__(256, NS == 1 ? 4 : 2) void gemm1x1_kernel(const bf16* __restrict__ x1, const bf16* __restrict__ x2,
                                                         const bf16* __restrict__ w, const float* __restrict__ bias,
                                                         const bf16* __restrict__ res, const bf16* __restrict__ res2,
                                                         bf16* __restrict__ y1, bf16* __restrict__ y2, int M, int C1,
                                                         int C2, int Cout, int Co1) {
  constexpr int STAGE = (G1_BM + BN) * 128;  // bytes
  constexpr int TM = BN / 32;                // 16-co fragments per wave
  constexpr int ELD = BN + 8;                // epilogue row (bf16)
  constexpr int LDSB = NS * STAGE > G1_BM * ELD * 2 ? NS * STAGE : G1_BM * ELD * 2;
  __shared__ __attribute__((aligned(1024))) char lds[LDSB];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int wr = wid >> 1, wc = wid & 1;
  const int lr = lane & 15, lg = lane >> 4;
  const int K = C1 + C2, nk = K / 64;
  // 1-D grid: the ncb co blocks of a pixel tile are dealt to ONE XCD back to back (linear id mod 8 = XCD), so
  // the tile's X rows are fetched into that XCD's L2 once instead of into up to ncb different L2s
  const int ncb = Cout / BN, L = blockIdx.x, jx = L >> 3;
  const int cb = jx % ncb;
  const int tile = (jx / ncb) * 8 + (L & 7);
  if (tile * G1_BM >= M) return;  // padded tiles (whole block)
  const int m0 = tile * G1_BM, n0 = cb * BN;
  const int prow = lane >> 3, pslot = lane & 7;

  auto issue = [&](int ks) {
    const int c0 = ks * 64;
    const bf16* src;
    int cs, cc;
    if (c0 < C1) { src = x1; cs = C1; cc = c0; } else { src = x2; cs = C2; cc = c0 - C1; }
    const int rows = M - m0 < G1_BM ? M - m0 : G1_BM;
    const __amdgpu_buffer_rsrc_t xrs = __builtin_amdgcn_make_buffer_rsrc(
        (void*)(src + (int64_t)m0 * cs + cc), (short)0, rows * cs * 2 - cc * 2, 0x00020000);
    const __amdgpu_buffer_rsrc_t wrs = __builtin_amdgcn_make_buffer_rsrc(
        (void*)(w + (int64_t)n0 * K + c0), (short)0, BN * K * 2 - c0 * 2, 0x00020000);
    char* sx = lds + (NS == 2 ? (ks & 1) * STAGE : 0);
    char* sw = sx + G1_BM * 128;
#pragma unroll
    for (int k = 0; k < G1_BM / 32; ++k) {  // 8-row pieces, 4 per wave
      const int q = wid + 4 * k, row = 8 * q + prow;
      const int chunk = pslot ^ (row & 7);
      const int vo = m0 + row < M ? (row * cs + chunk * 8) * 2 : 0x7ffffff0;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(xrs, (__attribute__((address_space(3))) void*)(sx + q * 1024), 16, vo, 0,
                                               0, 0);
    }
#pragma unroll
    for (int k = 0; k < BN / 32; ++k) {
      const int q = wid + 4 * k, row = 8 * q + prow;
      const int chunk = pslot ^ (row & 7);
      __builtin_amdgcn_raw_ptr_buffer_load_lds(wrs, (__attribute__((address_space(3))) void*)(sw + q * 1024), 16,
                                               (row * K + chunk * 8) * 2, 0, 0, 0);
    }
  };

  f32x4 acc[TM][4];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  issue(0);
  for (int ks = 0; ks < nk; ++ks) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();  // stage ks landed for all waves; stage ks+1's previous reads (step ks-1) are done
    if (NS == 2 && ks + 1 < nk) issue(ks + 1);
    const char* sx = lds + (NS == 2 ? (ks & 1) * STAGE : 0);
    const char* sw = sx + G1_BM * 128;
#pragma unroll
    for (int k32 = 0; k32 < 2; ++k32) {
      const int chunk = k32 * 4 + lg;
      bf16x8 af[TM], bfr[4];
#pragma unroll
      for (int i = 0; i < TM; ++i) af[i] = *reinterpret_cast<const bf16x8*>(sw + g1_off(wr * (BN / 2) + i * 16 + lr, chunk));
#pragma unroll
      for (int j = 0; j < 4; ++j) bfr[j] = *reinterpret_cast<const bf16x8*>(sx + g1_off(wc * 64 + j * 16 + lr, chunk));
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[i], bfr[j], acc[i][j], 0, 0, 0);
    }
  }
  __syncthreads();  // all fragment reads done: reuse the stages for the output tile
  bf16* so = reinterpret_cast<bf16*>(lds);
#pragma unroll
  for (int i = 0; i < TM; ++i) {
    const int co = wr * (BN / 2) + i * 16 + lg * 4;
    float bv[4] = {0.f, 0.f, 0.f, 0.f};
    if (bias) {
#pragma unroll
      for (int r = 0; r < 4; ++r) bv[r] = bias[n0 + co + r];
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int p = wc * 64 + j * 16 + lr;
      float v[4] = {acc[i][j][0] + bv[0], acc[i][j][1] + bv[1], acc[i][j][2] + bv[2], acc[i][j][3] + bv[3]};
      store4(so + p * ELD + co, v);
    }
  }
  __syncthreads();
  constexpr int CPR = BN / 8;  // 16-B chunks per pixel row
  constexpr int NIT = G1_BM * CPR / 256;
  const int Co2 = Cout - Co1;
  // residual vectors of every iteration issued together, unpredicated (clamped address, selected
  // after): under the lane predicates each was a branch with its own vmcnt(0)
  bf16x8 rv[NIT];
  if (res || res2) {  // uniform
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      const int e = it * 256 + tid;
      const int p = e / CPR, c = e - p * CPR;
      const int m = m0 + p, co = n0 + c * 8;
      const bool first = co < Co1;
      const bf16* rp = first ? res : res2;
      const bool use = m < M && rp != nullptr;
      const int64_t off = use ? (first ? (int64_t)m * Co1 + co : (int64_t)m * Co2 + (co - Co1)) : 0;
      const bf16x8 t = *reinterpret_cast<const bf16x8*>((use ? rp : (res ? res : res2)) + off);
      rv[it] = use ? t : bf16x8{};
    }
  }
#pragma unroll
  for (int it = 0; it < NIT; ++it) {
    const int e = it * 256 + tid;
    const int p = e / CPR, c = e - p * CPR;
    const int m = m0 + p;
    if (m >= M) continue;
    bf16x8 v = *reinterpret_cast<const bf16x8*>(so + p * ELD + c * 8);
    const int co = n0 + c * 8;
    bf16* dst = co < Co1 ? y1 + (int64_t)m * Co1 + co : y2 + (int64_t)m * Co2 + (co - Co1);
    if (res || res2) {
#pragma unroll
      for (int q = 0; q < 8; ++q) v[q] = (bf16)((float)v[q] + (float)rv[it][q]);
    }
    *reinterpret_cast<bf16x8*>(dst) = v;  // (round 6: non-temporal here -- isolated 1x1 convs 9 % faster, the F = 12
                                          // step and the F = 120 leg unchanged, profiles/r6late_g1_nontemporal_ab.txt)
  }
}


// ----------------------------------------------------------------------------------------
// host-side tile choosers of the halo kernels
// ----------------------------------------------------------------------------------------
constexpr int C2_HROWS = 384;                 // most halo pixels (TH+2)(TW+2) of a c2_tile tile
// tile shape for an Ho x Wo image: TW in {32, 36}, TH*TW <= 256, (TH+2)(TW+2) <= 384; maximise
// useful / computed pixels (fewest tiles on ties)
static void c2_tile(int Ho, int Wo, int& TH, int& TW) {
  double best = -1.0;
  int bt = 1 << 30;
  for (int tw : {32, 36}) {
    for (int th = 1; th * tw <= 256; ++th) {
      if ((th + 2) * (tw + 2) > C2_HROWS) break;
      const int ntile = (int)(cdiv(Ho, th) * cdiv(Wo, tw));
      const double util = (double)Ho * Wo / ((double)ntile * 256);
      // a non-32 width must buy > 10 % utilisation (32-wide tiles align with the fragment rows)
      const double u = tw == 32 ? util + 0.10 : util;
      if (u > best + 1e-9 || (u > best - 1e-9 && ntile < bt)) { best = u; bt = ntile; TH = th; TW = tw; }
    }
  }
}

// warp-specialized conv tile: TW in {32, 36} (halo width <= WS_PITCH), TH * TW <= 256; returns the pixel utilisation
static double ws_tile(int Ho, int Wo, int& TH, int& TW) {
  double best = -1.0;
  for (int tw : {32, 36}) {
    for (int th = 1; th <= WS_MAXTH && th * tw <= WS_PIX; ++th) {
      const double util = (double)Ho * Wo / ((double)cdiv(Ho, th) * cdiv(Wo, tw) * WS_PIX);
      if (util > best + 1e-9) { best = util; TH = th; TW = tw; }
    }
  }
  return best;
}

// halo-conv tile for the 448-pixel blocks (conv3x3_bf16_kernel<TW, 7>): TW in {32, 36}, TH*TW <= 448,
// TH + 2 <= 16 halo rows; the most useful / computed pixels, a 32-wide tile needs > 5 % better utilisation
static void h3_big_tile(int Ho, int Wo, int& TH, int& TW) {
  double best = -1.0;
  int bt = 1 << 30;
  for (int tw : {36, 32}) {
    for (int th = 1; th * tw <= 448 && th + 2 <= 16; ++th) {
      const int ntile = (int)(cdiv(Ho, th) * cdiv(Wo, tw));
      const double util = (double)Ho * Wo / ((double)ntile * 448);
      const double u = tw == 32 ? util - 0.05 : util;
      if (u > best + 1e-9 || (u > best - 1e-9 && ntile < bt)) { best = u; bt = ntile; TH = th; TW = tw; }
    }
  }
}

// Kernel selection of cesm_conv_fwd (host only, no GPU work): every launch and the
// cesm_conv_fwd_variant query go through this one function, so tests can assert which kernel a shape reaches.
enum ConvFwdVariant {
  CFV_INVALID = -1,
  CFV_GEMM1X1_128 = 0, CFV_GEMM1X1_64, CFV_P32_RW, CFV_HALO36, CFV_HALO32, CFV_TCONV_PAR_128, CFV_TCONV_PAR_64, CFV_GEN_BF16_128, CFV_GEN_BF16_64,
  CFV_GEN_F32_128, CFV_GEN_F32_64, CFV_S2DOWN36, CFV_S2DOWN32, CFV_S2UP36, CFV_S2UP32, CFV_WS32, CFV_WS36, CFV_COUNT
};
// (labels that tests, bench.py and the committed profiles key on; "conv3x3p_kernel<32,7,true>" keeps the arguments
// of the template it was before the kernel was specialised to its one instantiation)
static const char* const kConvFwdVariantName[CFV_COUNT] = {
    "gemm1x1_kernel<128>", "gemm1x1_kernel<64>", "conv3x3p_kernel<32,7,true>", "conv3x3_bf16_kernel<36>",
    "conv3x3_bf16_kernel<32>", "conv_fwd_bf16_kernel<128,true>", "conv_fwd_bf16_kernel<64,true>",
    "conv_fwd_bf16_kernel<128>", "conv_fwd_bf16_kernel<64>", "conv_fwd_kernel<float,128>",
    "conv_fwd_kernel<float,64>", "convs2_bf16_kernel<36,down>", "convs2_bf16_kernel<32,down>",
    "convs2_bf16_kernel<36,up>", "convs2_bf16_kernel<32,up>", "conv3x3ws_kernel<32>", "conv3x3ws_kernel<36>"};

struct ConvFwdPlan {
  ConvFwdVariant v = CFV_INVALID;
  int TH = 0, TW = 0;  // halo tile (conv3x3p / conv3x3ws / halo kernels)
};

static ConvFwdPlan conv_fwd_plan(int dtype, int Nb, int Hi, int Wi, int C1, int C2, int Ho, int Wo, int Cout, int Co1,
                                 int KH, int KW, int S, int P, int U) {
  ConvFwdPlan pl;
  if ((C1 % BK) || (C2 % BK) || (Cout % 64) || (Co1 % 16) || Co1 > Cout || C1 <= 0) return pl;
  if (dtype != CESM_DT_BF16 && dtype != CESM_DT_F32) return pl;
  const int64_t M = (int64_t)Nb * Ho * Wo;
  const int BN = (Cout % 128 == 0) ? 128 : 64;
  const bool halo3 = dtype == CESM_DT_BF16 && KH == 3 && KW == 3 && S == 1 && P == 1 && U == 1 && Ho == Hi &&
                     Wo == Wi && (Co1 % H3_BN) == 0;
  const bool g1x1 = dtype == CESM_DT_BF16 && KH == 1 && KW == 1 && S == 1 && P == 0 && U == 1 && Ho == Hi &&
                    Wo == Wi && (C1 % 64) == 0 && (C2 % 64) == 0 && (Co1 % 8) == 0 && M < (1ll << 31);
  int wth = 0, wtw = 0;
  // warp-specialized conv: by default for the level-0 64 -> 64 shape only (the conv3x3p case: 579 -> 518 us at
  // 96 x 192 x 288, profiles/r4c4_ws_check.txt); at 128 / 256 channels and for concat inputs it measured 0.85 - 1.01x
  // of the halo conv, so there it is opt-in (CESM_CONV_WS=1)
  const bool ws = halo3 && (C1 + C2) >= 64 && (getenv_flag("CESM_CONV_WS") || (C1 == 64 && C2 == 0 && Cout == 64));
  const double wutil = ws ? ws_tile(Ho, Wo, wth, wtw) : 0.0;
  if (g1x1) {
    pl.v = (Cout % 128 == 0) ? CFV_GEMM1X1_128 : CFV_GEMM1X1_64;
  } else if (wutil >= 0.9) {
    // warp-specialized persistent conv (round 4) where its 256-pixel tiles cover the image to >= 90 %
    pl.v = wtw == 36 ? CFV_WS36 : CFV_WS32;
    pl.TH = wth;
    pl.TW = wtw;
  } else if (halo3 && (C1 + C2) == 64 && Cout == 64 && (Wo % 32) == 0) {
    // v4 (persistent, resident weights) for the level-0 64 -> 64 convs the warp-specialized tiles do not cover
    // (the reference's 64 / 128-wide crops): TW = 32 -> TH = 14 (448 px = 4 waves x 7 groups).  (Round 6 removed the
    // env-selected alternatives: the halo conv here, this kernel everywhere, its 3-stage and streamed-weight forms,
    // and the round-1 v2 / v3 kernels -- all measured slower, profiles/r2_*, r3_conv_v4_everywhere_ab.txt.)
    pl.TW = 32;
    pl.TH = CP_TH;
    pl.v = CFV_P32_RW;
  } else if (halo3) {
    pl.TH = H3_TH; pl.TW = H3_TW;
    h3_big_tile(Ho, Wo, pl.TH, pl.TW);
    pl.v = pl.TW == 36 ? CFV_HALO36 : CFV_HALO32;
  } else if (dtype == CESM_DT_BF16 && KH == 4 && KW == 4 && C2 == 0 && Co1 == Cout && (Cout % H3_BN) == 0 &&
             ((S == 2 && P == 1 && U == 1 && Hi == 2 * Ho && Wi == 2 * Wo) ||
              (S == 1 && P == 2 && U == 2 && Ho == 2 * Hi && Wo == 2 * Wi))) {
    // stride-2 4x4 conv / its transpose: halo kernel on the low-resolution grid
    const bool up = U == 2;
    const int Hl = up ? Hi : Ho, Wl = up ? Wi : Wo;
    pl.TH = H3_TH; pl.TW = H3_TW;
    c2_tile(Hl, Wl, pl.TH, pl.TW);
    pl.v = up ? (pl.TW == 36 ? CFV_S2UP36 : CFV_S2UP32) : (pl.TW == 36 ? CFV_S2DOWN36 : CFV_S2DOWN32);
  } else if (dtype == CESM_DT_BF16 && U == 2 && S == 1 && KH % 2 == 0 && KW % 2 == 0 && Ho % 2 == 0 &&
             Wo % 2 == 0) {
    pl.v = BN == 128 ? CFV_TCONV_PAR_128 : CFV_TCONV_PAR_64;
  } else if (dtype == CESM_DT_BF16) {
    pl.v = BN == 128 ? CFV_GEN_BF16_128 : CFV_GEN_BF16_64;
  } else {
    pl.v = BN == 128 ? CFV_GEN_F32_128 : CFV_GEN_F32_64;
  }
  return pl;
}

}  // namespace

// ========================================================================================
// C ABI
// ========================================================================================
extern "C" {

const char* cesm_conv_fwd_variant(int dtype, int Nb, int Hi, int Wi, int C1, int C2, int Ho, int Wo, int Cout,
                                  int Co1, int KH, int KW, int S, int P, int U) {
  const ConvFwdPlan pl = conv_fwd_plan(dtype, Nb, Hi, Wi, C1, C2, Ho, Wo, Cout, Co1, KH, KW, S, P, U);
  return pl.v == CFV_INVALID ? "invalid" : kConvFwdVariantName[pl.v];
}

}  // extern "C"

namespace {
// GroupNorm statistics partial slots per sample that the halo conv of plan pl writes for Nb images in B samples:
// conv3x3p: (frame, tile, wave), conv3x3_bf16: (frame, tile, pixel half); 0 = this plan has no partials
int64_t conv_gn_nslot(const ConvFwdPlan& pl, int Nb, int Ho, int Wo, int B) {
  if (B <= 0 || Nb % B) return 0;
  const int64_t fimg = Nb / B;
  const int64_t tiles = (pl.TW > 0 && pl.TH > 0) ? cdiv(Wo, pl.TW) * cdiv(Ho, pl.TH) : 0;
  switch (pl.v) {
    case CFV_P32_RW: return fimg * tiles * 4;
    case CFV_HALO36: case CFV_HALO32: return fimg * tiles * 4;
    case CFV_WS32: case CFV_WS36: return fimg * tiles * 4;
    default: return 0;
  }
}

int conv_fwd_launch(int dtype, const void* x1, const void* x2, const void* wp, const float* bias, const void* res,
                    const void* res2, void* y1, void* y2, int Nb, int Hi, int Wi, int C1, int C2, int Ho, int Wo,
                    int Cout, int Co1, int KH, int KW, int S, int P, int U, float* gnp, int gn_fimg, int* queue,
                    hipStream_t stream) {
  const ConvFwdPlan pl = conv_fwd_plan(dtype, Nb, Hi, Wi, C1, C2, Ho, Wo, Cout, Co1, KH, KW, S, P, U);
  if (pl.v == CFV_INVALID) return CESM_EINVAL;
  ConvGeom g{Nb, Hi, Wi, Ho, Wo, C1, C2, Cout, Co1, KH, KW, S, P, U};
  g.wch = wpk_chunked(dtype == CESM_DT_BF16, Cout, C1 + C2, KH, KW);
  const int64_t M = (int64_t)Nb * Ho * Wo;
  const int BN = (Cout % 128 == 0) ? 128 : 64;
  dim3 grid(Cout / BN, (unsigned)cdiv(M, BMP));
  const bf16 *bx1 = (const bf16*)x1, *bx2 = (const bf16*)x2, *bwp = (const bf16*)wp, *br = (const bf16*)res,
             *br2 = (const bf16*)res2;
  bf16 *by1 = (bf16*)y1, *by2 = (bf16*)y2;
  // the halo and level-0 kernels (bf16 only) are launched from their own sources
  const ConvLaunchArgs fam{bx1, bx2, bwp, bias, br, br2, by1, by2, Nb, Hi, Wi, Ho, Wo, C1, C2, Cout, Co1, KH, KW, S, P, U,
                           pl.TH, pl.TW, gnp, gn_fimg, queue, stream};
  switch (pl.v) {
    case CFV_GEMM1X1_128:
    case CFV_GEMM1X1_64: {
      const bool one = C1 + C2 == 64;  // single-stage K = 64 variant
#define G1L(BNv, NSv)                                                                                               \
  gemm1x1_kernel<BNv, NSv><<<dim3((unsigned)(Cout / BNv * 8 * cdiv(cdiv(M, G1_BM), 8))), 256, 0, stream>>>(      \
      bx1, bx2, bwp, bias, br, br2, by1, by2, (int)M, C1, C2, Cout, Co1)
      if (pl.v == CFV_GEMM1X1_128) {
        if (one) G1L(128, 1); else G1L(128, 2);
      } else {
        if (one) G1L(64, 1); else G1L(64, 2);
      }
#undef G1L
      break;
    }
    case CFV_P32_RW: conv_p32_launch(fam); break;
    case CFV_WS32:
    case CFV_WS36: conv_ws_launch(fam); break;
    case CFV_HALO36:
    case CFV_HALO32: conv_halo3_launch(fam); break;
    case CFV_S2DOWN36:
    case CFV_S2DOWN32:
    case CFV_S2UP36:
    case CFV_S2UP32: conv_s2_launch(fam); break;
    case CFV_TCONV_PAR_128:
    case CFV_TCONV_PAR_64: {
      const int64_t Mp = (int64_t)Nb * (Ho / 2) * (Wo / 2);
      const int bpp = (int)cdiv(Mp, BMP);
      dim3 gp(Cout / BN, 4 * bpp);
      if (pl.v == CFV_TCONV_PAR_128)
        conv_fwd_bf16_kernel<128, true><<<gp, 256, 0, stream>>>(bx1, bx2, bwp, bias, br, br2, by1, by2, g, Mp, bpp);
      else
        conv_fwd_bf16_kernel<64, true><<<gp, 256, 0, stream>>>(bx1, bx2, bwp, bias, br, br2, by1, by2, g, Mp, bpp);
      break;
    }
    case CFV_GEN_BF16_128:
      conv_fwd_bf16_kernel<128><<<grid, 256, 0, stream>>>(bx1, bx2, bwp, bias, br, br2, by1, by2, g, M);
      break;
    case CFV_GEN_BF16_64:
      conv_fwd_bf16_kernel<64><<<grid, 256, 0, stream>>>(bx1, bx2, bwp, bias, br, br2, by1, by2, g, M);
      break;
    case CFV_GEN_F32_128:
      conv_fwd_kernel<float, 128><<<grid, 256, 0, stream>>>((const float*)x1, (const float*)x2, (const float*)wp,
                                                            bias, (const float*)res, (const float*)res2, (float*)y1,
                                                            (float*)y2, g, M);
      break;
    case CFV_GEN_F32_64:
      conv_fwd_kernel<float, 64><<<grid, 256, 0, stream>>>((const float*)x1, (const float*)x2, (const float*)wp,
                                                           bias, (const float*)res, (const float*)res2, (float*)y1,
                                                           (float*)y2, g, M);
      break;
    default:
      return CESM_EINVAL;
  }
  return cesm_launch_status();
}
}  // namespace

extern "C" {

// Generic implicit-GEMM conv / dgrad.  Shapes: x1 [Nb][Hi][Wi][C1], x2 [Nb][Hi][Wi][C2] (may be
// null if C2 == 0), wp [Cout][KH*KW][C1+C2] packed, y1 [Nb][Ho][Wo][Co1], y2 [..][Cout-Co1].
int cesm_conv_fwd(int dtype, const void* x1, const void* x2, const void* wp, const float* bias, const void* res,
                  const void* res2, void* y1, void* y2, int Nb, int Hi, int Wi, int C1, int C2, int Ho, int Wo, int Cout, int Co1,
                  int KH, int KW, int S, int P, int U, int* queue, hipStream_t stream) {
  if (Nb <= 0 || Ho <= 0 || Wo <= 0) return CESM_OK;
  return conv_fwd_launch(dtype, x1, x2, wp, bias, res, res2, y1, y2, Nb, Hi, Wi, C1, C2, Ho, Wo, Cout, Co1, KH, KW, S, P,
                         U, nullptr, 1, queue, stream);
}

int64_t cesm_conv_gn_nslot(int dtype, int Nb, int Hi, int Wi, int C1, int C2, int Ho, int Wo, int Cout, int KH, int KW,
                           int S, int P, int U, int B) {
  const ConvFwdPlan pl = conv_fwd_plan(dtype, Nb, Hi, Wi, C1, C2, Ho, Wo, Cout, Cout, KH, KW, S, P, U);
  return conv_gn_nslot(pl, Nb, Ho, Wo, B);
}

int cesm_conv_fwd_gn(int dtype, const void* x1, const void* x2, const void* wp, const float* bias, void* y, float* gnpart,
                     int B, int Nb, int Hi, int Wi, int C1, int C2, int Ho, int Wo, int Cout, int KH, int KW, int S,
                     int P, int U, int* queue, hipStream_t stream) {
  if (Nb <= 0 || Ho <= 0 || Wo <= 0) return CESM_OK;
  const ConvFwdPlan pl = conv_fwd_plan(dtype, Nb, Hi, Wi, C1, C2, Ho, Wo, Cout, Cout, KH, KW, S, P, U);
  if (pl.v == CFV_INVALID) return CESM_EINVAL;
  if (!gnpart || conv_gn_nslot(pl, Nb, Ho, Wo, B) == 0) return CESM_EUNSUPPORTED;
  return conv_fwd_launch(dtype, x1, x2, wp, bias, nullptr, nullptr, y, nullptr, Nb, Hi, Wi, C1, C2, Ho, Wo, Cout, Cout,
                         KH, KW, S, P, U, gnpart, Nb / B, queue, stream);
}

}  // extern "C"
