// Multi-variable stem and head: the two ends of the network for V target variables (2 <= V <= 4).
//   stem  Conv3d(2V -> Co, (1,KS,KS), pad KS/2) on cat([x_t, cond]): input channels 0..V-1 are x_t, V..2V-1 are cond
//         xt [B][V][Fx][H][W], cond [B][V][Fc][H][W] fp32 (Fx, Fc = 1 or F; 1 < F is a stride-0 read of frame 0),
//         w [Co][2V][KS][KS] fp32, y / dy [B*F][H][W][Co] in the compute dtype
//   head  Conv3d(C -> V, 1) on frame F/2: out [B][V][HW] fp32, w [V][C], bias [V]
// V = 1 is not handled here: the *_mv entry points hand it to the single-variable entry points (stem_head.hip), which
// launch what they always launched.  Everything is deterministic: no atomics, fixed summation orders.
// Included by stem_head.hip alone, after its sum_partials_kernel, which the weight gradient's launcher here uses.
// The second half of the file is the stem for Cc != V conditioning maps (cesm_stem_*_mc: V + Cc input planes), as
// kernels of their own.
#pragma once
#include <algorithm>

#include "common.h"
#include "cesm_hip.h"

namespace {

constexpr int MV_TS = 16;    // output tile of the stem forward and data gradient
constexpr int MV_TWM = 22;   // halo width at KS = 7 (row stride of the LDS halos for every KS)
constexpr int MV_HP = MV_TWM * MV_TWM;
constexpr int MV_VMAX = 4;

// plane (frame f of input channel ci of sample b) of the concatenated stem input
__device__ __forceinline__ const float* mv_plane(const float* xt, const float* cond, int V, int ci, int b, int f, int Fx,
                                                 int Fc, int64_t HW) {
  return ci < V ? xt + (((int64_t)b * V + ci) * Fx + (Fx == 1 ? 0 : f)) * HW
                : cond + (((int64_t)b * V + (ci - V)) * Fc + (Fc == 1 ? 0 : f)) * HW;
}

// ---------------------------------------------------------------------------------------- stem forward, fp32
// The single-variable VALU kernel with a loop over plane pairs (2cp, 2cp + 1): the static LDS is that kernel's, the
// 64 accumulators stay in registers over the pairs (input channels summed in ascending order).
__global__ __launch_bounds__(256) void mv_stem_fwd_kernel(const float* __restrict__ xt, const float* __restrict__ cond,
                                                          const float* __restrict__ w, const float* __restrict__ bias,
                                                          float* __restrict__ y, int V, int F, int Fx, int Fc, int H,
                                                          int W, int Co, int KS) {
  const int PAD = KS / 2, TW = MV_TS + KS - 1, KK = KS * KS, CIN = 2 * V;
  __shared__ float tin[2][MV_HP];
  __shared__ float tw[64 * 2 * 49];
  const int n = blockIdx.z;
  const int b = n / F, f = n - b * F;
  const int tiles_x = (W + MV_TS - 1) / MV_TS;
  const int ty0 = ((int)blockIdx.x / tiles_x) * MV_TS, tx0 = ((int)blockIdx.x % tiles_x) * MV_TS;
  const int cog = blockIdx.y * 64;
  const int py = threadIdx.x / MV_TS, px = threadIdx.x % MV_TS;
  const int oy = ty0 + py, ox = tx0 + px;
  float acc[64];
#pragma unroll
  for (int c = 0; c < 64; ++c) acc[c] = bias[cog + c];
  for (int cp = 0; cp < V; ++cp) {
    const float* s0 = mv_plane(xt, cond, V, 2 * cp, b, f, Fx, Fc, (int64_t)H * W);
    const float* s1 = mv_plane(xt, cond, V, 2 * cp + 1, b, f, Fx, Fc, (int64_t)H * W);
    __syncthreads();  // the previous pair's readers are done
    for (int e = threadIdx.x; e < TW * TW; e += 256) {
      const int yy = ty0 - PAD + e / TW, xx = tx0 - PAD + e % TW;
      const bool ok = yy >= 0 && yy < H && xx >= 0 && xx < W;
      tin[0][e] = ok ? s0[(int64_t)yy * W + xx] : 0.f;
      tin[1][e] = ok ? s1[(int64_t)yy * W + xx] : 0.f;
    }
    for (int e = threadIdx.x; e < 64 * 2 * KK; e += 256) {
      const int c = e / (2 * KK), r = e - c * 2 * KK;
      tw[e] = w[((int64_t)(cog + c) * CIN + 2 * cp) * KK + r];
    }
    __syncthreads();
    for (int ci = 0; ci < 2; ++ci)
      for (int ky = 0; ky < KS; ++ky)
        for (int kx = 0; kx < KS; ++kx) {
          const float v = tin[ci][(py + ky) * TW + px + kx];
          const int wo = (ci * KS + ky) * KS + kx;
#pragma unroll
          for (int c = 0; c < 64; ++c) acc[c] = fmaf(tw[c * 2 * KK + wo], v, acc[c]);
        }
  }
  if (oy < H && ox < W) {
    float* dst = y + (((int64_t)n * H + oy) * W + ox) * Co + cog;
#pragma unroll
    for (int c = 0; c < 64; c += 4) store4(dst + c, acc + c);
  }
}

// ---------------------------------------------------------------------------------------- stem forward, bf16 (MFMA)
// Implicit GEMM D[co][px] = W[co][k] X[k][px], k = ci*KS*KS + ky*KS + kx padded to a multiple of 32 (KS = 7: 224 at
// V = 2, 320 at V = 3, 416 at V = 4), mfma_f32_16x16x32_bf16, 16x16 output tile, persistent over tiles like the
// single-variable kernel.  That kernel keeps the 64 x 128 weight as A fragments in registers; 64 x 416 does not fit
// a register file, so here the block converts its weight slice ONCE into an LDS image of A fragments
//   wimg  bf16 [ct 4][ks NKS][lane 64][8]   (<= 52 KB; a fragment is one conflict-free 16-B read per lane)
// and re-reads 4 fragments per K-step per tile.  The halo is held as bf16 (the B operand is bf16 anyway, and the
// rounding is the one the gather did): tin bf16 [2V][22*22] (<= 7.6 KB).  The per-k halo offsets (ci*484 + ky*22 + kx)
// live in LDS as u16 (8 per lane per K-step: one 16-B read) instead of NKS x 8 registers.  Padding taps read offset 0
// with a zero weight: always a staged, finite halo element.
template <int CIN>
struct MvFwd {
  static constexpr int KPMAX = (CIN * 49 + 31) / 32 * 32;
  static constexpr int NKSMAX = KPMAX / 32;
};

template <int CIN>
__global__ __launch_bounds__(256) void mv_stem_fwd_mfma_kernel(const float* __restrict__ xt,
                                                               const float* __restrict__ cond,
                                                               const float* __restrict__ w,
                                                               const float* __restrict__ bias, bf16* __restrict__ y,
                                                               int F, int Fx, int Fc, int H, int W, int Co, int KS,
                                                               int ntiles) {
  constexpr int V = CIN / 2, KPMAX = MvFwd<CIN>::KPMAX, NKSMAX = MvFwd<CIN>::NKSMAX;
  __shared__ __attribute__((aligned(16))) bf16 wimg[64 * KPMAX];
  __shared__ __attribute__((aligned(16))) unsigned short koff[KPMAX];
  __shared__ bf16 tin[CIN * MV_HP];
  const int PAD = KS / 2, TW = MV_TS + KS - 1, KK = KS * KS, K = CIN * KK;
  const int nks = (K + 31) / 32;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int lr = lane & 15, lg = lane >> 4;
  const int cog = blockIdx.y * 64;
  const int tiles_x = (W + MV_TS - 1) / MV_TS, tiles_img = tiles_x * ((H + MV_TS - 1) / MV_TS);
  // A-fragment image: lane (lg, lr) of (ct, ks) holds W[ct*16 + lr][ks*32 + lg*8 + 0..7]
  for (int e = tid; e < 64 * nks * 32; e += 256) {
    const int co = e / (nks * 32), k = e - co * (nks * 32);
    const float v = k < K ? w[(int64_t)(cog + co) * K + k] : 0.f;
    const int ct = co >> 4, ks = k >> 5, ln = ((k >> 3) & 3) * 16 + (co & 15);
    wimg[((ct * NKSMAX + ks) * 64 + ln) * 8 + (k & 7)] = (bf16)v;
  }
  for (int k = tid; k < nks * 32; k += 256) {
    const int ci = k / KK, r = k - ci * KK, ky = r / KS, kx = r - ky * KS;
    koff[k] = k < K ? (unsigned short)(ci * MV_HP + ky * MV_TWM + kx) : (unsigned short)0;
  }
  float bv[4][4];
#pragma unroll
  for (int ct = 0; ct < 4; ++ct)
#pragma unroll
    for (int r = 0; r < 4; ++r) bv[ct][r] = bias[cog + ct * 16 + lg * 4 + r];
  // the next tile's halo values (TW*TW <= 484 <= 2 x 256 per plane) are loaded into registers while this tile computes
  float hv[2][CIN];
  auto fetch = [&](int tile_in) {
    // past the last tile: addresses of tile 0 (in bounds), values zeroed below
    const int tile = tile_in < ntiles ? tile_in : 0;
    const int n = tile / tiles_img, tr = tile - n * tiles_img;
    const int b = n / F, f = n - b * F;
    const int ty0 = (tr / tiles_x) * MV_TS, tx0 = (tr - (tr / tiles_x) * tiles_x) * MV_TS;
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int e = tid + q * 256;
      const int yy = ty0 - PAD + e / TW, xx = tx0 - PAD + e % TW;
      const bool ok = tile_in < ntiles && e < TW * TW && yy >= 0 && yy < H && xx >= 0 && xx < W;
      const int64_t o = ok ? (int64_t)yy * W + xx : 0;
#pragma unroll
      for (int ci = 0; ci < CIN; ++ci) {
        const float v = mv_plane(xt, cond, V, ci, b, f, Fx, Fc, (int64_t)H * W)[o];  // unpredicated, selected after
        hv[q][ci] = ok ? v : 0.f;
      }
    }
  };
  if ((int)blockIdx.x < ntiles) fetch(blockIdx.x);
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int n = tile / tiles_img, tr = tile - n * tiles_img;
    const int ty0 = (tr / tiles_x) * MV_TS, tx0 = (tr - (tr / tiles_x) * tiles_x) * MV_TS;
    __syncthreads();  // previous tile's gathers done (first tile: nothing pending)
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int e = tid + q * 256;
      if (e < TW * TW) {
        const int o = (e / TW) * MV_TWM + e % TW;
#pragma unroll
        for (int ci = 0; ci < CIN; ++ci) tin[ci * MV_HP + o] = (bf16)hv[q][ci];
      }
    }
    __syncthreads();  // halo (and, on the first tile, wimg / koff) visible
    fetch(tile + gridDim.x);
    f32x4 acc[4][4];
#pragma unroll
    for (int ct = 0; ct < 4; ++ct)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[ct][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int ks = 0; ks < nks; ++ks) {
      const u32x4 oq = *reinterpret_cast<const u32x4*>(koff + ks * 32 + lg * 8);
      int to[8];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        to[2 * i] = (int)(oq[i] & 0xffffu);
        to[2 * i + 1] = (int)(oq[i] >> 16);
      }
      bf16x8 af[4];
#pragma unroll
      for (int ct = 0; ct < 4; ++ct)
        af[ct] = *reinterpret_cast<const bf16x8*>(wimg + ((ct * NKSMAX + ks) * 64 + lane) * 8);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int pbase = (wid * 4 + j) * MV_TWM + lr;  // group j = tile row wid*4 + j, pixel lr
        bf16x8 bfr;
#pragma unroll
        for (int e = 0; e < 8; ++e) bfr[e] = tin[pbase + to[e]];
#pragma unroll
        for (int ct = 0; ct < 4; ++ct)
          acc[ct][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[ct], bfr, acc[ct][j], 0, 0, 0);
      }
    }
    // lane holds co = cog + ct*16 + lg*4 + r of pixel (wid*4 + j, lr)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int oy = ty0 + wid * 4 + j, ox = tx0 + lr;
      if (oy >= H || ox >= W) continue;
      bf16* dst = y + (((int64_t)n * H + oy) * W + ox) * Co + cog;
#pragma unroll
      for (int ct = 0; ct < 4; ++ct) {
        float v[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = acc[ct][j][r] + bv[ct][r];
        store4(dst + ct * 16 + lg * 4, v);
      }
    }
  }
}

// ---------------------------------------------------------------------------------------- stem weight gradient, fp32
// partials part[blk][co][ci*KS*KS + ky*KS + kx], ci < 2V.  The single-variable VALU kernel, one plane pair per
// blockIdx.z (the dy tile is re-read per pair; the static LDS is that kernel's).
__global__ __launch_bounds__(256) void mv_stem_wgrad_kernel(const float* __restrict__ xt, const float* __restrict__ cond,
                                                            const float* __restrict__ dy, float* __restrict__ part,
                                                            int V, int F, int Fx, int Fc, int H, int W, int Co, int KS,
                                                            int ntiles) {
  const int PAD = KS / 2;
  constexpr int TH = 8, TWD = 32;
  const int IH = TH + KS - 1, IW = TWD + KS - 1;  // <= 14 x 38
  __shared__ float tin[2][14 * 38];
  __shared__ float tdy[TH * TWD * 65];
  const int KK = 2 * KS * KS;  // taps of the pair
  const int cp = blockIdx.z;
  const int co = threadIdx.x & 63, grp = threadIdx.x >> 6;
  const int tpg = (KK + 3) / 4;
  float acc[25];
  int toff[25];  // LDS offset of each of this thread's taps (-1: none)
#pragma unroll
  for (int i = 0; i < 25; ++i) {
    acc[i] = 0.f;
    const int kk = grp * tpg + i;
    if (i < tpg && kk < KK) {
      const int ci = kk / (KS * KS), r = kk - ci * KS * KS;
      const int ky = r / KS, kx = r - ky * KS;
      toff[i] = ci * (14 * 38) + ky * IW + kx;
    } else {
      toff[i] = -1;
    }
  }
  const float* tinf = &tin[0][0];
  const int tx_tiles = (W + TWD - 1) / TWD, ty_tiles = (H + TH - 1) / TH;
  const int per_img = tx_tiles * ty_tiles;
  const int cog = blockIdx.y * 64;
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int n = tile / per_img;
    const int rem = tile - n * per_img;
    const int ty0 = (rem / tx_tiles) * TH, tx0 = (rem % tx_tiles) * TWD;
    const int b = n / F, f = n - b * F;
    const float* s0 = mv_plane(xt, cond, V, 2 * cp, b, f, Fx, Fc, (int64_t)H * W);
    const float* s1 = mv_plane(xt, cond, V, 2 * cp + 1, b, f, Fx, Fc, (int64_t)H * W);
    __syncthreads();
    for (int e = threadIdx.x; e < IH * IW; e += 256) {
      const int yy = ty0 - PAD + e / IW, xx = tx0 - PAD + e % IW;
      const bool ok = yy >= 0 && yy < H && xx >= 0 && xx < W;
      tin[0][e] = ok ? s0[(int64_t)yy * W + xx] : 0.f;
      tin[1][e] = ok ? s1[(int64_t)yy * W + xx] : 0.f;
    }
    for (int e = threadIdx.x; e < TH * TWD * 64; e += 256) {
      const int p = e >> 6, c = e & 63;
      const int yy = ty0 + p / TWD, xx = tx0 + p % TWD;
      tdy[p * 65 + c] = (yy < H && xx < W) ? dy[(((int64_t)n * H + yy) * W + xx) * Co + cog + c] : 0.f;
    }
    __syncthreads();
    for (int py = 0; py < TH; ++py)
      for (int px = 0; px < TWD; ++px) {
        const float g = tdy[(py * TWD + px) * 65 + co];
        const int base = py * IW + px;
#pragma unroll
        for (int i = 0; i < 25; ++i)
          if (toff[i] >= 0) acc[i] = fmaf(g, tinf[toff[i] + base], acc[i]);
      }
  }
  const int KT = 2 * V * KS * KS;
  for (int i = 0; i < tpg; ++i) {
    const int kk = grp * tpg + i;
    if (kk < KK) part[((int64_t)blockIdx.x * Co + cog + co) * KT + cp * KK + kk] = acc[i];
  }
}

// ---------------------------------------------------------------------------------------- stem weight gradient, bf16
// The single-variable MFMA kernel (8x32-pixel tiles, wave = 16 output channels, A = dy^T by transposed LDS reads, B =
// kx-shifted bf16 copies of the halo) with the dy tile staged once per tile and a loop over the V plane pairs inside
// it: a pair's halo and shifted copies reuse one buffer, its 7 tap tiles (98 taps padded to 112) accumulate in their
// own registers (V x 7 f32x4).
constexpr int MW_TH = 8, MW_TW = 32;
__device__ __forceinline__ int mw_dy_off(int px, int co) {  // bf16 index in the [256][64] dy tile
  return px * 64 + ((((co >> 3) ^ (px & 7))) << 3) + (co & 7);
}
template <int V>
__global__ __launch_bounds__(256) void mv_stem_wgrad_mfma_kernel(const float* __restrict__ xt,
                                                                 const float* __restrict__ cond,
                                                                 const bf16* __restrict__ dy, float* __restrict__ part,
                                                                 int F, int Fx, int Fc, int H, int W, int Co, int KS,
                                                                 int ntiles) {
  const int PAD = KS / 2;
  const int IH = MW_TH + KS - 1, IW = MW_TW + KS - 1;  // <= 14 x 38
  const int NT = 2 * KS * KS;                          // taps of a pair (<= 98)
  __shared__ float tin[2 * 14 * 38];
  __shared__ __attribute__((aligned(16))) bf16 tink[7 * 2 * 14 * MW_TW];
  __shared__ __attribute__((aligned(16))) bf16 tdy[MW_TH * MW_TW * 64];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int lr = lane & 15, lg = lane >> 4;
  const int cog = blockIdx.y * 64;
  int toff[7];  // per-lane tap offsets into tink for each of the 7 tap tiles (-1: padded tap)
#pragma unroll
  for (int nt = 0; nt < 7; ++nt) {
    const int t = nt * 16 + lr;
    if (t < NT) {
      const int ci = t / (KS * KS), r = t - ci * KS * KS, ky = r / KS, kx = r - ky * KS;
      toff[nt] = ((kx * 2 + ci) * 14 + ky) * MW_TW + lg * 8;
    } else {
      toff[nt] = -1;
    }
  }
  f32x4 acc[V][7];
#pragma unroll
  for (int cp = 0; cp < V; ++cp)
#pragma unroll
    for (int nt = 0; nt < 7; ++nt) acc[cp][nt] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int tx_tiles = (W + MW_TW - 1) / MW_TW, ty_tiles = (H + MW_TH - 1) / MW_TH;
  const int per_img = tx_tiles * ty_tiles;
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int n = tile / per_img;
    const int rem = tile - n * per_img;
    const int ty0 = (rem / tx_tiles) * MW_TH, tx0 = (rem % tx_tiles) * MW_TW;
    const int b = n / F, f = n - b * F;
    __syncthreads();  // previous tile's readers done
    for (int e = tid; e < MW_TH * MW_TW * 8; e += 256) {  // dy: 256 px x 8 chunks of 8 co
      const int px = e >> 3, ch = e & 7;
      const int yy = ty0 + px / MW_TW, xx = tx0 + px % MW_TW;
      bf16x8 v;
      if (yy < H && xx < W) v = *reinterpret_cast<const bf16x8*>(dy + (((int64_t)n * H + yy) * W + xx) * Co + cog + ch * 8);
      else {
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = (bf16)0.f;
      }
      *reinterpret_cast<bf16x8*>(tdy + mw_dy_off(px, ch * 8)) = v;
    }
#pragma unroll
    for (int cp = 0; cp < V; ++cp) {
      const float* s0 = mv_plane(xt, cond, V, 2 * cp, b, f, Fx, Fc, (int64_t)H * W);
      const float* s1 = mv_plane(xt, cond, V, 2 * cp + 1, b, f, Fx, Fc, (int64_t)H * W);
      // tin's last readers (the previous pair's copy loop) finished before the barrier that followed it
      for (int e = tid; e < IH * IW; e += 256) {
        const int yy = ty0 - PAD + e / IW, xx = tx0 - PAD + e % IW;
        const bool ok = yy >= 0 && yy < H && xx >= 0 && xx < W;
        tin[e] = ok ? s0[(int64_t)yy * W + xx] : 0.f;
        tin[IH * IW + e] = ok ? s1[(int64_t)yy * W + xx] : 0.f;
      }
      __syncthreads();  // tin (and tdy) staged; the previous pair's tink readers are done
      for (int e = tid; e < KS * 2 * IH * MW_TW; e += 256) {  // kx-shifted bf16 copies
        const int x = e % MW_TW, r = e / MW_TW;
        const int row = r % IH, r2 = r / IH, ci = r2 & 1, kx = r2 >> 1;
        tink[((kx * 2 + ci) * 14 + row) * MW_TW + x] = (bf16)tin[ci * IH * IW + row * IW + x + kx];
      }
      __syncthreads();
#pragma unroll 2
      for (int py = 0; py < MW_TH; ++py) {
        // A: dy^T[co = wid*16 + i][px = py*32 + 8g + e]
        bf16x8 a;
        const int q = (lane >> 2) & 3, p4 = (lane & 3) * 4;
#pragma unroll
        for (int hf = 0; hf < 2; ++hf) {
          const int px = py * MW_TW + lg * 8 + hf * 4 + q;
          const s16x4 v = __builtin_amdgcn_ds_read_tr16_b64_v4i16((LDS_PTR(s16x4))(tdy + mw_dy_off(px, wid * 16 + p4)));
#pragma unroll
          for (int e = 0; e < 4; ++e) a[hf * 4 + e] = __builtin_bit_cast(bf16, (short)v[e]);
        }
#pragma unroll
        for (int nt = 0; nt < 7; ++nt) {
          bf16x8 bb;
          if (toff[nt] >= 0) bb = *reinterpret_cast<const bf16x8*>(tink + toff[nt] + py * MW_TW);
          else {
#pragma unroll
            for (int i = 0; i < 8; ++i) bb[i] = (bf16)0.f;
          }
          acc[cp][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, bb, acc[cp][nt], 0, 0, 0);
        }
      }
    }
  }
  // D[co = wid*16 + 4g + r][tap = nt*16 + i] of pair cp
  const int KT = V * NT;
#pragma unroll
  for (int cp = 0; cp < V; ++cp)
#pragma unroll
    for (int nt = 0; nt < 7; ++nt) {
      const int t = nt * 16 + lr;
      if (t >= NT) continue;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int co = cog + wid * 16 + lg * 4 + r;
        part[((int64_t)blockIdx.x * Co + co) * KT + cp * NT + t] = acc[cp][nt][r];
      }
    }
}

// ---------------------------------------------------------------------------------------- stem data gradient
//   dX_ci[b][f'][y][x] = sum_{f -> f'} sum_{co,ky,kx} w[co][ci][ky][kx] * dy[b,f][y - ky + P][x - kx + P][co]
// dxt [B][V][Fx][H][W] (ci < V) and dcond [B][V][Fc][H][W] (ci >= V), each nullable.  The rules of stem_dgrad.h: a
// block = one 16x16 tile of one sample and a run of frames, all 2V accumulators of a pixel in registers; a per-frame
// output is stored and reset after every frame, a broadcast one once after the last frame (the host then gives one
// block every frame), so each output element is written by exactly one thread in a fixed order.  Out-of-image dy
// counts as zero: halo loads read a clamped in-bounds address and select afterwards.
__device__ __forceinline__ float* mv_dst(float* base, int b, int V, int v, int Fi, int f, int F, int H, int W, int y,
                                         int x) {
  return base + ((((int64_t)b * V + v) * Fi + (Fi == F ? f : 0)) * H + y) * W + x;
}

constexpr int MD_CC = 16;  // dy channels staged at a time (fp32)
template <int CIN>
__global__ __launch_bounds__(256) void mv_stem_dgrad_kernel(const float* __restrict__ dy, const float* __restrict__ w,
                                                            float* __restrict__ dxt, float* __restrict__ dcond, int F,
                                                            int Fx, int Fc, int H, int W, int Co, int KS, int fpb) {
  constexpr int V = CIN / 2;
  __shared__ float tdy[MD_CC][MV_HP];
  __shared__ float tw[MD_CC * CIN * 49];
  const int PAD = KS / 2, TW = MV_TS + KS - 1, KK = KS * KS;
  const int tid = threadIdx.x, py = tid / MV_TS, px = tid % MV_TS;
  const int tiles_x = (W + MV_TS - 1) / MV_TS;
  const int ty0 = ((int)blockIdx.x / tiles_x) * MV_TS, tx0 = ((int)blockIdx.x % tiles_x) * MV_TS;
  const int b = blockIdx.y;
  const int f0 = blockIdx.z * fpb, f1 = min(F, f0 + fpb);
  const int oy = ty0 + py, ox = tx0 + px;
  const bool inside = oy < H && ox < W;
  float a[CIN];
#pragma unroll
  for (int ci = 0; ci < CIN; ++ci) a[ci] = 0.f;
  for (int f = f0; f < f1; ++f) {
    const float* src = dy + (int64_t)(b * F + f) * H * W * Co;
    for (int c0 = 0; c0 < Co; c0 += MD_CC) {
      __syncthreads();  // the previous chunk's readers are done
      for (int e = tid; e < TW * TW * (MD_CC / 4); e += 256) {
        const int p = e / (MD_CC / 4), q = e % (MD_CC / 4);
        const int hy = p / TW, hx = p - hy * TW;
        const int yy = ty0 - PAD + hy, xx = tx0 - PAD + hx;
        const bool ok = yy >= 0 && yy < H && xx >= 0 && xx < W;
        const int64_t o = ok ? ((int64_t)yy * W + xx) * Co + c0 + q * 4 : 0;  // clamped: element 0 of the frame
        const f32x4 v = *reinterpret_cast<const f32x4*>(src + o);
#pragma unroll
        for (int i = 0; i < 4; ++i) tdy[q * 4 + i][hy * MV_TWM + hx] = ok ? v[i] : 0.f;
      }
      for (int e = tid; e < MD_CC * CIN * KK; e += 256) tw[e] = w[(int64_t)c0 * CIN * KK + e];
      __syncthreads();
      for (int c = 0; c < MD_CC; ++c) {
        const float* wc = tw + c * CIN * KK;
        for (int ky = 0; ky < KS; ++ky) {
          const float* row = &tdy[c][(py + KS - 1 - ky) * MV_TWM + px + KS - 1];
          for (int kx = 0; kx < KS; ++kx) {
            const float v = row[-kx];
#pragma unroll
            for (int ci = 0; ci < CIN; ++ci) a[ci] = fmaf(wc[ci * KK + ky * KS + kx], v, a[ci]);
          }
        }
      }
    }
    const bool last = f == f1 - 1;
#pragma unroll
    for (int ci = 0; ci < CIN; ++ci) {
      const bool isx = ci < V;
      const int Fi = isx ? Fx : Fc;
      float* base = isx ? dxt : dcond;
      if (Fi == F || last) {
        if (base && inside) *mv_dst(base, b, V, isx ? ci : ci - V, Fi, f, F, H, W, oy, ox) = a[ci];
      }
      if (Fi == F) a[ci] = 0.f;
    }
  }
}

// bf16 mode on MFMA: D[ci][px] = sum_k W'[ci][k] dYhalo[k][px], k = (ky, kx, co), as in stem_dgrad.h with the 2V input
// channels in rows 0..2V-1 of the 16-row A fragment (2V <= 8 rows: the two rows of V = 1 left 14 idle).
//   halo  bf16 [22*22 px][64 co], 62 KB, a pixel's 8 16-B chunks XOR-swizzled with (px index & 7)
//   wimg  bf16 [KS*KS taps][2 halves][2V ci][32 co], <= 49 KB: the weight of the current 64-channel group
// Dynamic LDS (per-call attribute): 62 KB + wimg.  Wave w owns tile rows 4w..4w+3; results: lane (lg, lr), register
// r = channel ci = lg*4 + r of pixel lr.
constexpr int MD_HALO = MV_HP * 64;  // bf16 elements
constexpr int MD_WIMG_MAX = 49 * 2 * (2 * MV_VMAX) * 32;
constexpr int MD_LDS_MAX = (MD_HALO + MD_WIMG_MAX) * 2;  // bytes
__global__ __launch_bounds__(256) void mv_stem_dgrad_mfma_kernel(const bf16* __restrict__ dy,
                                                                 const float* __restrict__ w, float* __restrict__ dxt,
                                                                 float* __restrict__ dcond, int V, int F, int Fx, int Fc,
                                                                 int H, int W, int Co, int KS, int fpb) {
  extern __shared__ __attribute__((aligned(16))) bf16 md_lds[];
  bf16* halo = md_lds;
  bf16* wimg = md_lds + MD_HALO;
  const int CIN = 2 * V;
  const int PAD = KS / 2, TW = MV_TS + KS - 1, KK = KS * KS;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int lr = lane & 15, lg = lane >> 4;
  const int tiles_x = (W + MV_TS - 1) / MV_TS;
  const int ty0 = ((int)blockIdx.x / tiles_x) * MV_TS, tx0 = ((int)blockIdx.x % tiles_x) * MV_TS;
  const int b = blockIdx.y;
  const int f0 = blockIdx.z * fpb, f1 = min(F, f0 + fpb);
  const int ngrp = Co / 64;
  f32x4 acc[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
  bf16x8 zero8;
#pragma unroll
  for (int i = 0; i < 8; ++i) zero8[i] = (bf16)0.f;
  const int arow = lr < CIN ? lr : 0;  // A row of this lane (rows >= 2V are zero)
  // halo pixel of (tile row wid*4, column lr) at tap (ky, kx) = (KS-1, KS-1); other rows / taps are offsets of it
  const int pbase = (wid * 4 + KS - 1) * MV_TWM + lr + KS - 1;
  for (int f = f0; f < f1; ++f) {
    const bf16* src = dy + (int64_t)(b * F + f) * H * W * Co;
    for (int g = 0; g < ngrp; ++g) {
      __syncthreads();  // the previous group's fragment reads are done
      for (int e = tid; e < TW * TW * 8; e += 256) {
        const int p = e >> 3, ch = e & 7;
        const int hy = p / TW, hx = p - hy * TW;
        const int yy = ty0 - PAD + hy, xx = tx0 - PAD + hx;
        const bool ok = yy >= 0 && yy < H && xx >= 0 && xx < W;
        const int64_t o = ok ? ((int64_t)yy * W + xx) * Co + g * 64 + ch * 8 : 0;  // clamped: the frame's first 16 B
        const bf16x8 v = *reinterpret_cast<const bf16x8*>(src + o);
        const int pix = hy * MV_TWM + hx;
        *reinterpret_cast<bf16x8*>(halo + pix * 64 + ((ch ^ (pix & 7)) << 3)) = ok ? v : zero8;
      }
      if (ngrp > 1 || f == f0) {
        for (int e = tid; e < KK * 2 * CIN * 32; e += 256) {
          const int c = e & 31, r1 = e >> 5, ci = r1 % CIN, r2 = r1 / CIN, h = r2 & 1, tap = r2 >> 1;
          wimg[e] = (bf16)w[((int64_t)(g * 64 + h * 32 + c) * CIN + ci) * KK + tap];
        }
      }
      __syncthreads();
      for (int ky = 0; ky < KS; ++ky)
        for (int kx = 0; kx < KS; ++kx) {
          const int tap = ky * KS + kx;
          const int p0 = pbase - ky * MV_TWM - kx;
#pragma unroll
          for (int h = 0; h < 2; ++h) {
            // A: row lr = ci, k = lg*8 + e = channel h*32 + lg*8 + e of this tap
            const bf16x8 av = *reinterpret_cast<const bf16x8*>(wimg + ((tap * 2 + h) * CIN + arow) * 32 + lg * 8);
            const bf16x8 a = lr < CIN ? av : zero8;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              const int pix = p0 + j * MV_TWM;
              const bf16x8 bv = *reinterpret_cast<const bf16x8*>(halo + pix * 64 + (((h * 4 + lg) ^ (pix & 7)) << 3));
              acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, bv, acc[j], 0, 0, 0);
            }
          }
        }
    }
    const bool last = f == f1 - 1;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int oy = ty0 + wid * 4 + j, ox = tx0 + lr;
      const bool inside = oy < H && ox < W;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int ci = lg * 4 + r;
        if (ci < CIN) {
          const bool isx = ci < V;
          const int Fi = isx ? Fx : Fc;
          float* base = isx ? dxt : dcond;
          if ((Fi == F || last) && base && inside)
            *mv_dst(base, b, V, isx ? ci : ci - V, Fi, f, F, H, W, oy, ox) = acc[j][r];
          if (Fi == F) acc[j][r] = 0.f;
        }
      }
    }
  }
}

// ---------------------------------------------------------------------------------------- head
// out[b][v][p] = bias[v] + sum_c w[v][c] * x[b, F/2, p, c]: 8 lanes per pixel, each lane 8 channels per 64; x is read
// once for all V outputs
template <typename T, int V>
__global__ void mv_head_fwd_kernel(const T* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias,
                                   float* __restrict__ out, int B, int F, int HW, int C) {
  const int64_t gw = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) >> 3;
  const int sub = threadIdx.x & 7;
  const int64_t total = (int64_t)B * HW;
  if (gw >= total) return;
  const int b = (int)(gw / HW);
  const int64_t p = gw - (int64_t)b * HW;
  const T* src = x + (((int64_t)b * F + F / 2) * HW + p) * C;
  float s[V];
#pragma unroll
  for (int v = 0; v < V; ++v) s[v] = 0.f;
  for (int c = sub * 8; c < C; c += 64) {
    float xv[8];
    load8(src + c, xv);
#pragma unroll
    for (int v = 0; v < V; ++v)
#pragma unroll
      for (int i = 0; i < 8; ++i) s[v] = fmaf(xv[i], w[v * C + c + i], s[v]);
  }
#pragma unroll
  for (int v = 0; v < V; ++v) {
    const float t = group_sum(s[v], 8);
    if (sub == 0) out[((int64_t)b * V + v) * HW + p] = t + bias[v];
  }
}

// dX = 0 everywhere except frame mid, where dX[c] = sum_v dout[b][v][p] * w[v][c] (v ascending)
template <typename T, int V>
__global__ void mv_head_dgrad_kernel(const float* __restrict__ dout, const float* __restrict__ w, T* __restrict__ dx,
                                     int B, int F, int HW, int C) {
  const int64_t total = (int64_t)B * F * HW * (C / 8);
  for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
    const int cq = (int)(e % (C / 8));
    const int64_t vox = e / (C / 8);
    const int64_t p = vox % HW;
    const int64_t nf = vox / HW;
    const int f = (int)(nf % F), b = (int)(nf / F);
    float o[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (f == F / 2) {
#pragma unroll
      for (int v = 0; v < V; ++v) {
        const float g = dout[((int64_t)b * V + v) * HW + p];
#pragma unroll
        for (int i = 0; i < 8; ++i) o[i] = fmaf(g, w[v * C + cq * 8 + i], o[i]);
      }
    }
    store8(dx + vox * C + cq * 8, o);
  }
}

// head weight / bias gradient partials part[blk][v][c] (c < C) and part[blk][v][C] = bias: thread = (pixel lane pl,
// 8-channel chunk sub), one coalesced pass over the mid frame per 64 channels for all V outputs, per-block sums over
// the 32 pixel lanes in a fixed order
template <typename T, int V>
__global__ __launch_bounds__(256) void mv_head_wgrad_kernel(const float* __restrict__ dout, const T* __restrict__ x,
                                                            float* __restrict__ part, int B, int F, int HW, int C,
                                                            int64_t px_per_blk) {
  __shared__ float red[32][65];
  const int64_t total = (int64_t)B * HW;
  const int64_t p0 = blockIdx.x * px_per_blk, p1 = min(total, p0 + px_per_blk);
  const int sub = threadIdx.x & 7, pl = threadIdx.x >> 3;
  for (int c0 = 0; c0 < C; c0 += 64) {
    const bool live = c0 + sub * 8 < C;
    float acc[V][8], gs[V];
#pragma unroll
    for (int v = 0; v < V; ++v) {
      gs[v] = 0.f;
#pragma unroll
      for (int i = 0; i < 8; ++i) acc[v][i] = 0.f;
    }
    for (int64_t q = p0 + pl; q < p1; q += 32) {
      const int b = (int)(q / HW);
      const int64_t p = q - (int64_t)b * HW;
      float g[V];
#pragma unroll
      for (int v = 0; v < V; ++v) {
        g[v] = dout[((int64_t)b * V + v) * HW + p];
        gs[v] += g[v];
      }
      if (live) {
        float xv[8];
        load8(x + (((int64_t)b * F + F / 2) * HW + p) * C + c0 + sub * 8, xv);
#pragma unroll
        for (int v = 0; v < V; ++v)
#pragma unroll
          for (int i = 0; i < 8; ++i) acc[v][i] = fmaf(g[v], xv[i], acc[v][i]);
      }
    }
#pragma unroll
    for (int v = 0; v < V; ++v) {
#pragma unroll
      for (int i = 0; i < 8; ++i) red[pl][sub * 8 + i] = acc[v][i];
      if (sub == 0) red[pl][64] = gs[v];
      __syncthreads();
      if (threadIdx.x < 65) {
        const int c = threadIdx.x;
        float t = 0.f;
        for (int q = 0; q < 32; ++q) t += red[q][c];
        float* dst = part + ((int64_t)blockIdx.x * V + v) * (C + 1);
        if (c < 64 && c0 + c < C) dst[c0 + c] = t;
        if (c == 64 && c0 == 0) dst[C] = t;
      }
      __syncthreads();
    }
  }
}

// dw[v][c] / db[v] (+)= sum_blk part[blk][v][c], blocks ascending
__global__ void mv_head_reduce_kernel(const float* __restrict__ part, float* __restrict__ dw, float* __restrict__ db,
                                      int nblk, int V, int C, int accumulate) {
  const int n = V * (C + 1);
  for (int e = threadIdx.x; e < n; e += blockDim.x) {
    const int v = e / (C + 1), c = e - v * (C + 1);
    float s = 0.f;
    for (int k = 0; k < nblk; ++k) s += part[(int64_t)k * n + e];
    float* d = (c == C) ? db + v : dw + v * C + c;
    *d = accumulate ? *d + s : s;
  }
}

inline bool mv_stem_shape_ok(int V, int B, int F, int Fx, int Fc, int H, int W, int Co, int KS) {
  return V >= 2 && V <= MV_VMAX && KS >= 1 && KS <= 7 && (KS & 1) && Co > 0 && Co % 64 == 0 && (Fx == 1 || Fx == F) &&
         (Fc == 1 || Fc == F) && B > 0 && F > 0 && H > 0 && W > 0 && (int64_t)B * F <= 65535 && Co / 64 <= 65535;
}

template <int V>
int mv_stem_fwd_bf16(const float* xt, const float* cond, const float* w, const float* bias, bf16* y, int B, int F, int Fx,
                     int Fc, int H, int W, int Co, int KS, hipStream_t stream) {
  const int64_t nt = cdiv(H, 16) * cdiv(W, 16) * B * F;
  if (nt > 0x7fffffff) return CESM_EUNSUPPORTED;
  // 2 blocks of this kernel's LDS fit a CU
  dim3 gp((unsigned)std::min<int64_t>(nt, 2 * (int64_t)cesm_num_cus()), Co / 64);
  mv_stem_fwd_mfma_kernel<2 * V><<<gp, 256, 0, stream>>>(xt, cond, w, bias, y, F, Fx, Fc, H, W, Co, KS, (int)nt);
  return cesm_launch_status();
}

template <typename T, int V>
int mv_head_bwd_t(const float* dout, const T* x, const float* w, T* dx, float* dw, float* part, int nblk, int B, int F,
                  int HW, int C, hipStream_t stream) {
  const int64_t total = (int64_t)B * F * HW * (C / 8);
  const unsigned g1 = (unsigned)std::min<int64_t>(cdiv(total, 256), 8192);
  const int64_t ppb = cdiv((int64_t)B * HW, nblk);
  if (dx) mv_head_dgrad_kernel<T, V><<<g1, 256, 0, stream>>>(dout, w, dx, B, F, HW, C);
  if (dw) mv_head_wgrad_kernel<T, V><<<nblk, 256, 0, stream>>>(dout, x, part, B, F, HW, C, ppb);
  return CESM_OK;
}

}  // namespace

// host launchers of the cesm_*_mv entry points (the ABI entries are in stem_head.hip)
static inline int mv_stem_fwd_launch(int dtype, const float* xt, const float* cond, const float* w, const float* bias, void* y, int B,
                     int V, int F, int Fx, int Fc, int H, int W, int Co, int KS, hipStream_t stream) {
  if (V == 1) return cesm_stem_fwd(dtype, xt, cond, w, bias, y, B, F, Fx, Fc, H, W, Co, KS, stream);
  if (dtype != CESM_DT_F32 && dtype != CESM_DT_BF16) return CESM_EINVAL;
  if (!xt || !cond || !w || !bias || !y) return CESM_EINVAL;
  if (!mv_stem_shape_ok(V, B, F, Fx, Fc, H, W, Co, KS)) return CESM_EUNSUPPORTED;
  if (dtype == CESM_DT_BF16) {
    switch (V) {
      case 2: return mv_stem_fwd_bf16<2>(xt, cond, w, bias, (bf16*)y, B, F, Fx, Fc, H, W, Co, KS, stream);
      case 3: return mv_stem_fwd_bf16<3>(xt, cond, w, bias, (bf16*)y, B, F, Fx, Fc, H, W, Co, KS, stream);
      default: return mv_stem_fwd_bf16<4>(xt, cond, w, bias, (bf16*)y, B, F, Fx, Fc, H, W, Co, KS, stream);
    }
  }
  const int64_t tiles = cdiv(H, 16) * cdiv(W, 16);
  if (tiles > 0x7fffffff) return CESM_EUNSUPPORTED;
  dim3 grid((unsigned)tiles, Co / 64, B * F);
  mv_stem_fwd_kernel<<<grid, 256, 0, stream>>>(xt, cond, w, bias, (float*)y, V, F, Fx, Fc, H, W, Co, KS);
  return cesm_launch_status();
}

static inline int mv_stem_wgrad_launch(int dtype, const float* xt, const float* cond, const void* dy, float* dw, float* part, int nblk,
                       int B, int V, int F, int Fx, int Fc, int H, int W, int Co, int KS, int accumulate,
                       hipStream_t stream) {
  if (V == 1)
    return cesm_stem_wgrad(dtype, xt, cond, dy, dw, part, nblk, B, F, Fx, Fc, H, W, Co, KS, accumulate, stream);
  if (dtype != CESM_DT_F32 && dtype != CESM_DT_BF16) return CESM_EINVAL;
  if (!xt || !cond || !dy || !dw || !part || nblk <= 0) return CESM_EINVAL;
  if (!mv_stem_shape_ok(V, B, F, Fx, Fc, H, W, Co, KS)) return CESM_EUNSUPPORTED;
  const int64_t nt = (int64_t)B * F * cdiv(H, 8) * cdiv(W, 32);
  if (nt > 0x7fffffff) return CESM_EUNSUPPORTED;
  if (dtype == CESM_DT_BF16) {
    dim3 grid(nblk, Co / 64);
    switch (V) {
      case 2:
        mv_stem_wgrad_mfma_kernel<2><<<grid, 256, 0, stream>>>(xt, cond, (const bf16*)dy, part, F, Fx, Fc, H, W, Co, KS,
                                                               (int)nt);
        break;
      case 3:
        mv_stem_wgrad_mfma_kernel<3><<<grid, 256, 0, stream>>>(xt, cond, (const bf16*)dy, part, F, Fx, Fc, H, W, Co, KS,
                                                               (int)nt);
        break;
      default:
        mv_stem_wgrad_mfma_kernel<4><<<grid, 256, 0, stream>>>(xt, cond, (const bf16*)dy, part, F, Fx, Fc, H, W, Co, KS,
                                                               (int)nt);
    }
  } else {
    dim3 grid(nblk, Co / 64, V);
    mv_stem_wgrad_kernel<<<grid, 256, 0, stream>>>(xt, cond, (const float*)dy, part, V, F, Fx, Fc, H, W, Co, KS,
                                                   (int)nt);
  }
  const int64_t n = (int64_t)Co * 2 * V * KS * KS;
  sum_partials_kernel<<<(unsigned)cdiv(n, 64), 1024, 0, stream>>>(part, dw, nblk, n, accumulate);
  return cesm_launch_status();
}

static inline int mv_stem_dgrad_launch(int dtype, const void* dy, const float* w, float* dxt, float* dcond, int B, int V, int F, int Fx,
                       int Fc, int H, int W, int Co, int KS, hipStream_t stream) {
  if (V == 1) return cesm_stem_dgrad(dtype, dy, w, dxt, dcond, B, F, Fx, Fc, H, W, Co, KS, stream);
  if (dtype != CESM_DT_F32 && dtype != CESM_DT_BF16) return CESM_EINVAL;
  if (B <= 0 || F <= 0 || H <= 0 || W <= 0 || !dy || !w) return CESM_EINVAL;
  if (!mv_stem_shape_ok(V, B, F, Fx, Fc, H, W, Co, KS) || B > 65535 || F > 65535) return CESM_EUNSUPPORTED;
  if (!dxt && !dcond) return CESM_OK;
  const int64_t tiles = cdiv(H, MV_TS) * cdiv(W, MV_TS);
  if (tiles > 0x7fffffff) return CESM_EUNSUPPORTED;
  // a broadcast output is a sum over every frame: one block runs them all.  Otherwise frames are independent and
  // are split over gridDim.z until the grid fills the chip (a per-frame output does not depend on the split).
  const bool bcast = (dxt && Fx != F) || (dcond && Fc != F);
  int fpb = F;
  if (!bcast) {
    const int64_t fz = std::min<int64_t>(F, std::max<int64_t>(1, cdiv(4 * (int64_t)cesm_num_cus(), tiles * B)));
    fpb = (int)cdiv(F, fz);
  }
  dim3 grid((unsigned)tiles, (unsigned)B, (unsigned)cdiv(F, fpb));
  if (dtype == CESM_DT_BF16) {
    if (hipFuncSetAttribute((const void*)mv_stem_dgrad_mfma_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                            MD_LDS_MAX) != hipSuccess)
      return CESM_ELAUNCH;
    const int lds = (MD_HALO + KS * KS * 2 * 2 * V * 32) * 2;
    mv_stem_dgrad_mfma_kernel<<<grid, 256, lds, stream>>>((const bf16*)dy, w, dxt, dcond, V, F, Fx, Fc, H, W, Co, KS,
                                                          fpb);
  } else {
    const float* d = (const float*)dy;
    switch (V) {
      case 2: mv_stem_dgrad_kernel<4><<<grid, 256, 0, stream>>>(d, w, dxt, dcond, F, Fx, Fc, H, W, Co, KS, fpb); break;
      case 3: mv_stem_dgrad_kernel<6><<<grid, 256, 0, stream>>>(d, w, dxt, dcond, F, Fx, Fc, H, W, Co, KS, fpb); break;
      default: mv_stem_dgrad_kernel<8><<<grid, 256, 0, stream>>>(d, w, dxt, dcond, F, Fx, Fc, H, W, Co, KS, fpb);
    }
  }
  return cesm_launch_status();
}

static inline int mv_head_fwd_launch(int dtype, const void* x, const float* w, const float* bias, float* out, int B, int V, int F,
                     int HW, int C, hipStream_t stream) {
  if (V == 1) return cesm_head_fwd(dtype, x, w, bias, out, B, F, HW, C, stream);
  if (dtype != CESM_DT_F32 && dtype != CESM_DT_BF16) return CESM_EINVAL;
  if (!x || !w || !bias || !out || B <= 0 || F <= 0 || HW <= 0 || C <= 0 || C % 8) return CESM_EINVAL;
  if (V < 2 || V > MV_VMAX) return CESM_EUNSUPPORTED;
  const unsigned grid = (unsigned)cdiv((int64_t)B * HW * 8, 256);
#define MV_HF(T, VV) mv_head_fwd_kernel<T, VV><<<grid, 256, 0, stream>>>((const T*)x, w, bias, out, B, F, HW, C)
  if (dtype == CESM_DT_BF16) {
    if (V == 2) MV_HF(bf16, 2); else if (V == 3) MV_HF(bf16, 3); else MV_HF(bf16, 4);
  } else {
    if (V == 2) MV_HF(float, 2); else if (V == 3) MV_HF(float, 3); else MV_HF(float, 4);
  }
#undef MV_HF
  return cesm_launch_status();
}

static inline int mv_head_bwd_launch(int dtype, const float* dout, const void* x, const float* w, void* dx, float* dw, float* db,
                     float* part, int nblk, int B, int V, int F, int HW, int C, int accumulate, hipStream_t stream) {
  if (V == 1) return cesm_head_bwd(dtype, dout, x, w, dx, dw, db, part, nblk, B, F, HW, C, accumulate, stream);
  if (dtype != CESM_DT_F32 && dtype != CESM_DT_BF16) return CESM_EINVAL;
  if (!dout || !x || !w || B <= 0 || F <= 0 || HW <= 0 || C <= 0 || C % 8 || nblk <= 0) return CESM_EINVAL;
  if (dw && (!db || !part)) return CESM_EINVAL;
  if (V < 2 || V > MV_VMAX) return CESM_EUNSUPPORTED;
#define MV_HB(T, VV) mv_head_bwd_t<T, VV>(dout, (const T*)x, w, (T*)dx, dw, part, nblk, B, F, HW, C, stream)
  if (dtype == CESM_DT_BF16) {
    if (V == 2) MV_HB(bf16, 2); else if (V == 3) MV_HB(bf16, 3); else MV_HB(bf16, 4);
  } else {
    if (V == 2) MV_HB(float, 2); else if (V == 3) MV_HB(float, 3); else MV_HB(float, 4);
  }
#undef MV_HB
  if (dw) mv_head_reduce_kernel<<<1, 256, 0, stream>>>(part, dw, db, nblk, V, C, accumulate);
  return cesm_launch_status();
}

// ======================================================================================== multi-forcing stem
// The stem with the cond plane count Cc separated from V (1 <= V, Cc <= 4, Cc != V here: Cc == V runs the launchers
// above): Conv3d(P -> Co), P = V + Cc, input channels 0..V-1 = x_t [B][V][Fx][H][W], V..P-1 = cond [B][Cc][Fc][H][W],
// w [Co][P][KS][KS].  Separate kernels, so that the code of the V = Cc instantiations above stays what it was.  Plane
// pairs are consecutive planes (2cp, 2cp + 1) of the concatenated input, so a pair may straddle the x_t / cond
// boundary, and an odd P leaves a last pair whose second plane does not exist (the phantom plane).  The phantom is
// never addressed (its pointer is the pair's first plane, its halo is zero-filled without a load), its weights are
// never read (they would lie in the next output channel's row, or past the tensor) and its taps are never written.
namespace {

__device__ __forceinline__ const float* mc_plane(const float* xt, const float* cond, int V, int Cc, int ci, int b, int f,
                                                 int Fx, int Fc, int64_t HW) {
  return ci < V ? xt + (((int64_t)b * V + ci) * Fx + (Fx == 1 ? 0 : f)) * HW
                : cond + (((int64_t)b * Cc + (ci - V)) * Fc + (Fc == 1 ? 0 : f)) * HW;
}

// ---- forward, fp32: mv_stem_fwd_kernel over ceil(P / 2) pairs
__global__ __launch_bounds__(256) void mc_stem_fwd_kernel(const float* __restrict__ xt, const float* __restrict__ cond,
                                                          const float* __restrict__ w, const float* __restrict__ bias,
                                                          float* __restrict__ y, int V, int Cc, int F, int Fx, int Fc,
                                                          int H, int W, int Co, int KS) {
  const int PAD = KS / 2, TW = MV_TS + KS - 1, KK = KS * KS, CIN = V + Cc, NP = (CIN + 1) / 2;
  __shared__ float tin[2][MV_HP];
  __shared__ float tw[64 * 2 * 49];
  const int n = blockIdx.z;
  const int b = n / F, f = n - b * F;
  const int tiles_x = (W + MV_TS - 1) / MV_TS;
  const int ty0 = ((int)blockIdx.x / tiles_x) * MV_TS, tx0 = ((int)blockIdx.x % tiles_x) * MV_TS;
  const int cog = blockIdx.y * 64;
  const int py = threadIdx.x / MV_TS, px = threadIdx.x % MV_TS;
  const int oy = ty0 + py, ox = tx0 + px;
  float acc[64];
#pragma unroll
  for (int c = 0; c < 64; ++c) acc[c] = bias[cog + c];
  for (int cp = 0; cp < NP; ++cp) {
    const bool two = 2 * cp + 1 < CIN;  // false: the second plane of this pair is the phantom
    const int nw = two ? 2 * KK : KK;   // weights of the pair that exist
    const float* s0 = mc_plane(xt, cond, V, Cc, 2 * cp, b, f, Fx, Fc, (int64_t)H * W);
    const float* s1 = two ? mc_plane(xt, cond, V, Cc, 2 * cp + 1, b, f, Fx, Fc, (int64_t)H * W) : s0;
    __syncthreads();  // the previous pair's readers are done
    for (int e = threadIdx.x; e < TW * TW; e += 256) {
      const int yy = ty0 - PAD + e / TW, xx = tx0 - PAD + e % TW;
      const bool ok = yy >= 0 && yy < H && xx >= 0 && xx < W;
      tin[0][e] = ok ? s0[(int64_t)yy * W + xx] : 0.f;
      tin[1][e] = ok && two ? s1[(int64_t)yy * W + xx] : 0.f;
    }
    for (int e = threadIdx.x; e < 64 * nw; e += 256) {
      const int c = e / nw, r = e - c * nw;
      tw[c * 2 * KK + r] = w[((int64_t)(cog + c) * CIN + 2 * cp) * KK + r];
    }
    __syncthreads();
    const int nci = two ? 2 : 1;
    for (int ci = 0; ci < nci; ++ci)
      for (int ky = 0; ky < KS; ++ky)
        for (int kx = 0; kx < KS; ++kx) {
          const float v = tin[ci][(py + ky) * TW + px + kx];
          const int wo = (ci * KS + ky) * KS + kx;
#pragma unroll
          for (int c = 0; c < 64; ++c) acc[c] = fmaf(tw[c * 2 * KK + wo], v, acc[c]);
        }
  }
  if (oy < H && ox < W) {
    float* dst = y + (((int64_t)n * H + oy) * W + ox) * Co + cog;
#pragma unroll
    for (int c = 0; c < 64; c += 4) store4(dst + c, acc + c);
  }
}

// ---- forward, bf16: mv_stem_fwd_mfma_kernel with CIN = P any of 3..7 and V a run-time split.  K = CIN KS^2 padded to
// a multiple of 32 (KS = 7: 147 -> 160, 196 -> 224, 245 -> 256, 294 -> 320, 343 -> 352); a padding tap reads halo
// offset 0 (staged, finite) against a zero weight.  The LDS weight image is that of the 2 ceil(P/2) kernel or smaller.
template <int CIN>
__global__ __launch_bounds__(256) void mc_stem_fwd_mfma_kernel(const float* __restrict__ xt,
                                                               const float* __restrict__ cond,
                                                               const float* __restrict__ w,
                                                               const float* __restrict__ bias, bf16* __restrict__ y,
                                                               int V, int F, int Fx, int Fc, int H, int W, int Co,
                                                               int KS, int ntiles) {
  constexpr int KPMAX = MvFwd<CIN>::KPMAX, NKSMAX = MvFwd<CIN>::NKSMAX;
  __shared__ __attribute__((aligned(16))) bf16 wimg[64 * KPMAX];
  __shared__ __attribute__((aligned(16))) unsigned short koff[KPMAX];
  __shared__ bf16 tin[CIN * MV_HP];
  const int Cc = CIN - V;
  const int PAD = KS / 2, TW = MV_TS + KS - 1, KK = KS * KS, K = CIN * KK;
  const int nks = (K + 31) / 32;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int lr = lane & 15, lg = lane >> 4;
  const int cog = blockIdx.y * 64;
  const int tiles_x = (W + MV_TS - 1) / MV_TS, tiles_img = tiles_x * ((H + MV_TS - 1) / MV_TS);
  // A-fragment image: lane (lg, lr) of (ct, ks) holds W[ct*16 + lr][ks*32 + lg*8 + 0..7]
  for (int e = tid; e < 64 * nks * 32; e += 256) {
    const int co = e / (nks * 32), k = e - co * (nks * 32);
    const float v = k < K ? w[(int64_t)(cog + co) * K + k] : 0.f;
    const int ct = co >> 4, ks = k >> 5, ln = ((k >> 3) & 3) * 16 + (co & 15);
    wimg[((ct * NKSMAX + ks) * 64 + ln) * 8 + (k & 7)] = (bf16)v;
  }
  for (int k = tid; k < nks * 32; k += 256) {
    const int ci = k / KK, r = k - ci * KK, ky = r / KS, kx = r - ky * KS;
    koff[k] = k < K ? (unsigned short)(ci * MV_HP + ky * MV_TWM + kx) : (unsigned short)0;
  }
  float bv[4][4];
#pragma unroll
  for (int ct = 0; ct < 4; ++ct)
#pragma unroll
    for (int r = 0; r < 4; ++r) bv[ct][r] = bias[cog + ct * 16 + lg * 4 + r];
  float hv[2][CIN];
  auto fetch = [&](int tile_in) {
    // past the last tile: addresses of tile 0 (in bounds), values zeroed below
    const int tile = tile_in < ntiles ? tile_in : 0;
    const int n = tile / tiles_img, tr = tile - n * tiles_img;
    const int b = n / F, f = n - b * F;
    const int ty0 = (tr / tiles_x) * MV_TS, tx0 = (tr - (tr / tiles_x) * tiles_x) * MV_TS;
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int e = tid + q * 256;
      const int yy = ty0 - PAD + e / TW, xx = tx0 - PAD + e % TW;
      const bool ok = tile_in < ntiles && e < TW * TW && yy >= 0 && yy < H && xx >= 0 && xx < W;
      const int64_t o = ok ? (int64_t)yy * W + xx : 0;
#pragma unroll
      for (int ci = 0; ci < CIN; ++ci) {
        const float v = mc_plane(xt, cond, V, Cc, ci, b, f, Fx, Fc, (int64_t)H * W)[o];  // unpredicated, selected after
        hv[q][ci] = ok ? v : 0.f;
      }
    }
  };
  if ((int)blockIdx.x < ntiles) fetch(blockIdx.x);
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int n = tile / tiles_img, tr = tile - n * tiles_img;
    const int ty0 = (tr / tiles_x) * MV_TS, tx0 = (tr - (tr / tiles_x) * tiles_x) * MV_TS;
    __syncthreads();  // previous tile's gathers done (first tile: nothing pending)
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int e = tid + q * 256;
      if (e < TW * TW) {
        const int o = (e / TW) * MV_TWM + e % TW;
#pragma unroll
        for (int ci = 0; ci < CIN; ++ci) tin[ci * MV_HP + o] = (bf16)hv[q][ci];
      }
    }
    __syncthreads();  // halo (and, on the first tile, wimg / koff) visible
    fetch(tile + gridDim.x);
    f32x4 acc[4][4];
#pragma unroll
    for (int ct = 0; ct < 4; ++ct)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[ct][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int ks = 0; ks < nks; ++ks) {
      const u32x4 oq = *reinterpret_cast<const u32x4*>(koff + ks * 32 + lg * 8);
      int to[8];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        to[2 * i] = (int)(oq[i] & 0xffffu);
        to[2 * i + 1] = (int)(oq[i] >> 16);
      }
      bf16x8 af[4];
#pragma unroll
      for (int ct = 0; ct < 4; ++ct)
        af[ct] = *reinterpret_cast<const bf16x8*>(wimg + ((ct * NKSMAX + ks) * 64 + lane) * 8);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int pbase = (wid * 4 + j) * MV_TWM + lr;  // group j = tile row wid*4 + j, pixel lr
        bf16x8 bfr;
#pragma unroll
        for (int e = 0; e < 8; ++e) bfr[e] = tin[pbase + to[e]];
#pragma unroll
        for (int ct = 0; ct < 4; ++ct)
          acc[ct][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[ct], bfr, acc[ct][j], 0, 0, 0);
      }
    }
    // lane holds co = cog + ct*16 + lg*4 + r of pixel (wid*4 + j, lr)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int oy = ty0 + wid * 4 + j, ox = tx0 + lr;
      if (oy >= H || ox >= W) continue;
      bf16* dst = y + (((int64_t)n * H + oy) * W + ox) * Co + cog;
#pragma unroll
      for (int ct = 0; ct < 4; ++ct) {
        float v[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = acc[ct][j][r] + bv[ct][r];
        store4(dst + ct * 16 + lg * 4, v);
      }
    }
  }
}

// ---- weight gradient, fp32: mv_stem_wgrad_kernel, one pair per blockIdx.z < ceil(P / 2); part rows hold P KS^2 taps
__global__ __launch_bounds__(256) void mc_stem_wgrad_kernel(const float* __restrict__ xt, const float* __restrict__ cond,
                                                            const float* __restrict__ dy, float* __restrict__ part,
                                                            int V, int Cc, int F, int Fx, int Fc, int H, int W, int Co,
                                                            int KS, int ntiles) {
  const int PAD = KS / 2, CIN = V + Cc;
  constexpr int TH = 8, TWD = 32;
  const int IH = TH + KS - 1, IW = TWD + KS - 1;  // <= 14 x 38
  __shared__ float tin[2][14 * 38];
  __shared__ float tdy[TH * TWD * 65];
  const int cp = blockIdx.z;
  const bool two = 2 * cp + 1 < CIN;
  const int KP = 2 * KS * KS;              // taps of a full pair (the pair's stride in a part row)
  const int KK = two ? KP : KS * KS;       // taps of this pair that exist
  const int co = threadIdx.x & 63, grp = threadIdx.x >> 6;
  const int tpg = (KK + 3) / 4;
  float acc[25];
  int toff[25];  // LDS offset of each of this thread's taps (-1: none)
#pragma unroll
  for (int i = 0; i < 25; ++i) {
    acc[i] = 0.f;
    const int kk = grp * tpg + i;
    if (i < tpg && kk < KK) {
      const int ci = kk / (KS * KS), r = kk - ci * KS * KS;
      const int ky = r / KS, kx = r - ky * KS;
      toff[i] = ci * (14 * 38) + ky * IW + kx;
    } else {
      toff[i] = -1;
    }
  }
  const float* tinf = &tin[0][0];
  const int tx_tiles = (W + TWD - 1) / TWD, ty_tiles = (H + TH - 1) / TH;
  const int per_img = tx_tiles * ty_tiles;
  const int cog = blockIdx.y * 64;
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int n = tile / per_img;
    const int rem = tile - n * per_img;
    const int ty0 = (rem / tx_tiles) * TH, tx0 = (rem % tx_tiles) * TWD;
    const int b = n / F, f = n - b * F;
    const float* s0 = mc_plane(xt, cond, V, Cc, 2 * cp, b, f, Fx, Fc, (int64_t)H * W);
    const float* s1 = two ? mc_plane(xt, cond, V, Cc, 2 * cp + 1, b, f, Fx, Fc, (int64_t)H * W) : s0;
    __syncthreads();
    for (int e = threadIdx.x; e < IH * IW; e += 256) {
      const int yy = ty0 - PAD + e / IW, xx = tx0 - PAD + e % IW;
      const bool ok = yy >= 0 && yy < H && xx >= 0 && xx < W;
      tin[0][e] = ok ? s0[(int64_t)yy * W + xx] : 0.f;
      tin[1][e] = ok && two ? s1[(int64_t)yy * W + xx] : 0.f;
    }
    for (int e = threadIdx.x; e < TH * TWD * 64; e += 256) {
      const int p = e >> 6, c = e & 63;
      const int yy = ty0 + p / TWD, xx = tx0 + p % TWD;
      tdy[p * 65 + c] = (yy < H && xx < W) ? dy[(((int64_t)n * H + yy) * W + xx) * Co + cog + c] : 0.f;
    }
    __syncthreads();
    for (int py = 0; py < TH; ++py)
      for (int px = 0; px < TWD; ++px) {
        const float g = tdy[(py * TWD + px) * 65 + co];
        const int base = py * IW + px;
#pragma unroll
        for (int i = 0; i < 25; ++i)
          if (toff[i] >= 0) acc[i] = fmaf(g, tinf[toff[i] + base], acc[i]);
      }
  }
  const int KT = CIN * KS * KS;
  for (int i = 0; i < tpg; ++i) {
    const int kk = grp * tpg + i;
    if (kk < KK) part[((int64_t)blockIdx.x * Co + cog + co) * KT + cp * KP + kk] = acc[i];
  }
}

// ---- weight gradient, bf16: mv_stem_wgrad_mfma_kernel with NP = ceil(P / 2) pairs (NP x 7 accumulator tiles).  The
// phantom plane's halo is zero-filled, so its taps accumulate zeros; they are not stored.
template <int NP>
__global__ __launch_bounds__(256) void mc_stem_wgrad_mfma_kernel(const float* __restrict__ xt,
                                                                 const float* __restrict__ cond,
                                                                 const bf16* __restrict__ dy, float* __restrict__ part,
                                                                 int V, int Cc, int F, int Fx, int Fc, int H, int W,
                                                                 int Co, int KS, int ntiles) {
  const int PAD = KS / 2, CIN = V + Cc;
  const int IH = MW_TH + KS - 1, IW = MW_TW + KS - 1;  // <= 14 x 38
  const int NT = 2 * KS * KS;                          // taps of a pair (<= 98)
  __shared__ float tin[2 * 14 * 38];
  __shared__ __attribute__((aligned(16))) bf16 tink[7 * 2 * 14 * MW_TW];
  __shared__ __attribute__((aligned(16))) bf16 tdy[MW_TH * MW_TW * 64];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int lr = lane & 15, lg = lane >> 4;
  const int cog = blockIdx.y * 64;
  int toff[7];  // per-lane tap offsets into tink for each of the 7 tap tiles (-1: padded tap)
#pragma unroll
  for (int nt = 0; nt < 7; ++nt) {
    const int t = nt * 16 + lr;
    if (t < NT) {
      const int ci = t / (KS * KS), r = t - ci * KS * KS, ky = r / KS, kx = r - ky * KS;
      toff[nt] = ((kx * 2 + ci) * 14 + ky) * MW_TW + lg * 8;
    } else {
      toff[nt] = -1;
    }
  }
  f32x4 acc[NP][7];
#pragma unroll
  for (int cp = 0; cp < NP; ++cp)
#pragma unroll
    for (int nt = 0; nt < 7; ++nt) acc[cp][nt] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int tx_tiles = (W + MW_TW - 1) / MW_TW, ty_tiles = (H + MW_TH - 1) / MW_TH;
  const int per_img = tx_tiles * ty_tiles;
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int n = tile / per_img;
    const int rem = tile - n * per_img;
    const int ty0 = (rem / tx_tiles) * MW_TH, tx0 = (rem % tx_tiles) * MW_TW;
    const int b = n / F, f = n - b * F;
    __syncthreads();  // previous tile's readers done
    for (int e = tid; e < MW_TH * MW_TW * 8; e += 256) {  // dy: 256 px x 8 chunks of 8 co
      const int px = e >> 3, ch = e & 7;
      const int yy = ty0 + px / MW_TW, xx = tx0 + px % MW_TW;
      bf16x8 v;
      if (yy < H && xx < W) v = *reinterpret_cast<const bf16x8*>(dy + (((int64_t)n * H + yy) * W + xx) * Co + cog + ch * 8);
      else {
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = (bf16)0.f;
      }
      *reinterpret_cast<bf16x8*>(tdy + mw_dy_off(px, ch * 8)) = v;
    }
#pragma unroll
    for (int cp = 0; cp < NP; ++cp) {
      const bool two = 2 * cp + 1 < CIN;
      const float* s0 = mc_plane(xt, cond, V, Cc, 2 * cp, b, f, Fx, Fc, (int64_t)H * W);
      const float* s1 = two ? mc_plane(xt, cond, V, Cc, 2 * cp + 1, b, f, Fx, Fc, (int64_t)H * W) : s0;
      // tin's last readers (the previous pair's copy loop) finished before the barrier that followed it
      for (int e = tid; e < IH * IW; e += 256) {
        const int yy = ty0 - PAD + e / IW, xx = tx0 - PAD + e % IW;
        const bool ok = yy >= 0 && yy < H && xx >= 0 && xx < W;
        tin[e] = ok ? s0[(int64_t)yy * W + xx] : 0.f;
        tin[IH * IW + e] = ok && two ? s1[(int64_t)yy * W + xx] : 0.f;
      }
      __syncthreads();  // tin (and tdy) staged; the previous pair's tink readers are done
      for (int e = tid; e < KS * 2 * IH * MW_TW; e += 256) {  // kx-shifted bf16 copies
        const int x = e % MW_TW, r = e / MW_TW;
        const int row = r % IH, r2 = r / IH, ci = r2 & 1, kx = r2 >> 1;
        tink[((kx * 2 + ci) * 14 + row) * MW_TW + x] = (bf16)tin[ci * IH * IW + row * IW + x + kx];
      }
      __syncthreads();
#pragma unroll 2
      for (int py = 0; py < MW_TH; ++py) {
        // A: dy^T[co = wid*16 + i][px = py*32 + 8g + e]
        bf16x8 a;
        const int q = (lane >> 2) & 3, p4 = (lane & 3) * 4;
#pragma unroll
        for (int hf = 0; hf < 2; ++hf) {
          const int px = py * MW_TW + lg * 8 + hf * 4 + q;
          const s16x4 v = __builtin_amdgcn_ds_read_tr16_b64_v4i16((LDS_PTR(s16x4))(tdy + mw_dy_off(px, wid * 16 + p4)));
#pragma unroll
          for (int e = 0; e < 4; ++e) a[hf * 4 + e] = __builtin_bit_cast(bf16, (short)v[e]);
        }
#pragma unroll
        for (int nt = 0; nt < 7; ++nt) {
          bf16x8 bb;
          if (toff[nt] >= 0) bb = *reinterpret_cast<const bf16x8*>(tink + toff[nt] + py * MW_TW);
          else {
#pragma unroll
            for (int i = 0; i < 8; ++i) bb[i] = (bf16)0.f;
          }
          acc[cp][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, bb, acc[cp][nt], 0, 0, 0);
        }
      }
    }
  }
  // D[co = wid*16 + 4g + r][tap = nt*16 + i] of pair cp; a part row holds CIN KS^2 taps, so the phantom's would be
  // the next row's first
  const int KT = CIN * KS * KS;
#pragma unroll
  for (int cp = 0; cp < NP; ++cp)
#pragma unroll
    for (int nt = 0; nt < 7; ++nt) {
      const int t = nt * 16 + lr;
      if (t >= NT || cp * NT + t >= KT) continue;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int co = cog + wid * 16 + lg * 4 + r;
        part[((int64_t)blockIdx.x * Co + co) * KT + cp * NT + t] = acc[cp][nt][r];
      }
    }
}

// ---- data gradient, fp32: mv_stem_dgrad_kernel with CIN = P and V a run-time split
template <int CIN>
__global__ __launch_bounds__(256) void mc_stem_dgrad_kernel(const float* __restrict__ dy, const float* __restrict__ w,
                                                            float* __restrict__ dxt, float* __restrict__ dcond, int V,
                                                            int F, int Fx, int Fc, int H, int W, int Co, int KS,
                                                            int fpb) {
  __shared__ float tdy[MD_CC][MV_HP];
  __shared__ float tw[MD_CC * CIN * 49];
  const int Cc = CIN - V;
  const int PAD = KS / 2, TW = MV_TS + KS - 1, KK = KS * KS;
  const int tid = threadIdx.x, py = tid / MV_TS, px = tid % MV_TS;
  const int tiles_x = (W + MV_TS - 1) / MV_TS;
  const int ty0 = ((int)blockIdx.x / tiles_x) * MV_TS, tx0 = ((int)blockIdx.x % tiles_x) * MV_TS;
  const int b = blockIdx.y;
  const int f0 = blockIdx.z * fpb, f1 = min(F, f0 + fpb);
  const int oy = ty0 + py, ox = tx0 + px;
  const bool inside = oy < H && ox < W;
  float a[CIN];
#pragma unroll
  for (int ci = 0; ci < CIN; ++ci) a[ci] = 0.f;
  for (int f = f0; f < f1; ++f) {
    const float* src = dy + (int64_t)(b * F + f) * H * W * Co;
    for (int c0 = 0; c0 < Co; c0 += MD_CC) {
      __syncthreads();  // the previous chunk's readers are done
      for (int e = tid; e < TW * TW * (MD_CC / 4); e += 256) {
        const int p = e / (MD_CC / 4), q = e % (MD_CC / 4);
        const int hy = p / TW, hx = p - hy * TW;
        const int yy = ty0 - PAD + hy, xx = tx0 - PAD + hx;
        const bool ok = yy >= 0 && yy < H && xx >= 0 && xx < W;
        const int64_t o = ok ? ((int64_t)yy * W + xx) * Co + c0 + q * 4 : 0;  // clamped: element 0 of the frame
        const f32x4 v = *reinterpret_cast<const f32x4*>(src + o);
#pragma unroll
        for (int i = 0; i < 4; ++i) tdy[q * 4 + i][hy * MV_TWM + hx] = ok ? v[i] : 0.f;
      }
      for (int e = tid; e < MD_CC * CIN * KK; e += 256) tw[e] = w[(int64_t)c0 * CIN * KK + e];
      __syncthreads();
      for (int c = 0; c < MD_CC; ++c) {
        const float* wc = tw + c * CIN * KK;
        for (int ky = 0; ky < KS; ++ky) {
          const float* row = &tdy[c][(py + KS - 1 - ky) * MV_TWM + px + KS - 1];
          for (int kx = 0; kx < KS; ++kx) {
            const float v = row[-kx];
#pragma unroll
            for (int ci = 0; ci < CIN; ++ci) a[ci] = fmaf(wc[ci * KK + ky * KS + kx], v, a[ci]);
          }
        }
      }
    }
    const bool last = f == f1 - 1;
#pragma unroll
    for (int ci = 0; ci < CIN; ++ci) {
      const bool isx = ci < V;
      const int Fi = isx ? Fx : Fc;
      float* base = isx ? dxt : dcond;
      if (Fi == F || last) {
        if (base && inside) *mv_dst(base, b, isx ? V : Cc, isx ? ci : ci - V, Fi, f, F, H, W, oy, ox) = a[ci];
      }
      if (Fi == F) a[ci] = 0.f;
    }
  }
}

// ---- data gradient, bf16: mv_stem_dgrad_mfma_kernel with the weight image [tap][half][P][32] (P <= 7 of the 16
// A-fragment rows); rows 0..V-1 go to dxt, V..P-1 to dcond
__global__ __launch_bounds__(256) void mc_stem_dgrad_mfma_kernel(const bf16* __restrict__ dy,
                                                                 const float* __restrict__ w, float* __restrict__ dxt,
                                                                 float* __restrict__ dcond, int V, int Cc, int F, int Fx,
                                                                 int Fc, int H, int W, int Co, int KS, int fpb) {
  extern __shared__ __attribute__((aligned(16))) bf16 md_lds[];
  bf16* halo = md_lds;
  bf16* wimg = md_lds + MD_HALO;
  const int CIN = V + Cc;
  const int PAD = KS / 2, TW = MV_TS + KS - 1, KK = KS * KS;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int lr = lane & 15, lg = lane >> 4;
  const int tiles_x = (W + MV_TS - 1) / MV_TS;
  const int ty0 = ((int)blockIdx.x / tiles_x) * MV_TS, tx0 = ((int)blockIdx.x % tiles_x) * MV_TS;
  const int b = blockIdx.y;
  const int f0 = blockIdx.z * fpb, f1 = min(F, f0 + fpb);
  const int ngrp = Co / 64;
  f32x4 acc[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
  bf16x8 zero8;
#pragma unroll
  for (int i = 0; i < 8; ++i) zero8[i] = (bf16)0.f;
  const int arow = lr < CIN ? lr : 0;  // A row of this lane (rows >= P are zero)
  // halo pixel of (tile row wid*4, column lr) at tap (ky, kx) = (KS-1, KS-1); other rows / taps are offsets of it
  const int pbase = (wid * 4 + KS - 1) * MV_TWM + lr + KS - 1;
  for (int f = f0; f < f1; ++f) {
    const bf16* src = dy + (int64_t)(b * F + f) * H * W * Co;
    for (int g = 0; g < ngrp; ++g) {
      __syncthreads();  // the previous group's fragment reads are done
      for (int e = tid; e < TW * TW * 8; e += 256) {
        const int p = e >> 3, ch = e & 7;
        const int hy = p / TW, hx = p - hy * TW;
        const int yy = ty0 - PAD + hy, xx = tx0 - PAD + hx;
        const bool ok = yy >= 0 && yy < H && xx >= 0 && xx < W;
        const int64_t o = ok ? ((int64_t)yy * W + xx) * Co + g * 64 + ch * 8 : 0;  // clamped: the frame's first 16 B
        const bf16x8 v = *reinterpret_cast<const bf16x8*>(src + o);
        const int pix = hy * MV_TWM + hx;
        *reinterpret_cast<bf16x8*>(halo + pix * 64 + ((ch ^ (pix & 7)) << 3)) = ok ? v : zero8;
      }
      if (ngrp > 1 || f == f0) {
        for (int e = tid; e < KK * 2 * CIN * 32; e += 256) {
          const int c = e & 31, r1 = e >> 5, ci = r1 % CIN, r2 = r1 / CIN, h = r2 & 1, tap = r2 >> 1;
          wimg[e] = (bf16)w[((int64_t)(g * 64 + h * 32 + c) * CIN + ci) * KK + tap];
        }
      }
      __syncthreads();
      for (int ky = 0; ky < KS; ++ky)
        for (int kx = 0; kx < KS; ++kx) {
          const int tap = ky * KS + kx;
          const int p0 = pbase - ky * MV_TWM - kx;
#pragma unroll
          for (int h = 0; h < 2; ++h) {
            // A: row lr = ci, k = lg*8 + e = channel h*32 + lg*8 + e of this tap
            const bf16x8 av = *reinterpret_cast<const bf16x8*>(wimg + ((tap * 2 + h) * CIN + arow) * 32 + lg * 8);
            const bf16x8 a = lr < CIN ? av : zero8;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              const int pix = p0 + j * MV_TWM;
              const bf16x8 bv = *reinterpret_cast<const bf16x8*>(halo + pix * 64 + (((h * 4 + lg) ^ (pix & 7)) << 3));
              acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, bv, acc[j], 0, 0, 0);
            }
          }
        }
    }
    const bool last = f == f1 - 1;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int oy = ty0 + wid * 4 + j, ox = tx0 + lr;
      const bool inside = oy < H && ox < W;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int ci = lg * 4 + r;
        if (ci < CIN) {
          const bool isx = ci < V;
          const int Fi = isx ? Fx : Fc;
          float* base = isx ? dxt : dcond;
          if ((Fi == F || last) && base && inside)
            *mv_dst(base, b, isx ? V : Cc, isx ? ci : ci - V, Fi, f, F, H, W, oy, ox) = acc[j][r];
          if (Fi == F) acc[j][r] = 0.f;
        }
      }
    }
  }
}

inline bool mc_stem_shape_ok(int V, int Cc, int B, int F, int Fx, int Fc, int H, int W, int Co, int KS) {
  return V >= 1 && V <= MV_VMAX && Cc >= 1 && Cc <= MV_VMAX && KS >= 1 && KS <= 7 && (KS & 1) && Co > 0 &&
         Co % 64 == 0 && (Fx == 1 || Fx == F) && (Fc == 1 || Fc == F) && B > 0 && F > 0 && H > 0 && W > 0 &&
         (int64_t)B * F <= 65535 && Co / 64 <= 65535;
}

}  // namespace

// host launchers of the cesm_stem_*_mc entry points: Cc == V IS the *_mv launcher (same kernels, same grids)
static inline int mc_stem_fwd_launch(int dtype, const float* xt, const float* cond, const float* w, const float* bias,
                                     void* y, int B, int V, int Cc, int F, int Fx, int Fc, int H, int W, int Co, int KS,
                                     hipStream_t stream) {
  if (Cc == V) return mv_stem_fwd_launch(dtype, xt, cond, w, bias, y, B, V, F, Fx, Fc, H, W, Co, KS, stream);
  if (dtype != CESM_DT_F32 && dtype != CESM_DT_BF16) return CESM_EINVAL;
  if (!xt || !cond || !w || !bias || !y) return CESM_EINVAL;
  if (!mc_stem_shape_ok(V, Cc, B, F, Fx, Fc, H, W, Co, KS)) return CESM_EUNSUPPORTED;
  const int64_t tiles = cdiv(H, 16) * cdiv(W, 16);
  if (tiles * B * F > 0x7fffffff) return CESM_EUNSUPPORTED;
  if (dtype == CESM_DT_BF16) {
    const int64_t nt = tiles * B * F;
    dim3 gp((unsigned)std::min<int64_t>(nt, 2 * (int64_t)cesm_num_cus()), Co / 64);
#define MC_FWD(P)                                                                                                  \
  mc_stem_fwd_mfma_kernel<P><<<gp, 256, 0, stream>>>(xt, cond, w, bias, (bf16*)y, V, F, Fx, Fc, H, W, Co, KS, (int)nt)
    switch (V + Cc) {
      case 3: MC_FWD(3); break;
      case 4: MC_FWD(4); break;
      case 5: MC_FWD(5); break;
      case 6: MC_FWD(6); break;
      default: MC_FWD(7);
    }
#undef MC_FWD
    return cesm_launch_status();
  }
  dim3 grid((unsigned)tiles, Co / 64, B * F);
  mc_stem_fwd_kernel<<<grid, 256, 0, stream>>>(xt, cond, w, bias, (float*)y, V, Cc, F, Fx, Fc, H, W, Co, KS);
  return cesm_launch_status();
}

static inline int mc_stem_wgrad_launch(int dtype, const float* xt, const float* cond, const void* dy, float* dw,
                                       float* part, int nblk, int B, int V, int Cc, int F, int Fx, int Fc, int H, int W,
                                       int Co, int KS, int accumulate, hipStream_t stream) {
  if (Cc == V)
    return mv_stem_wgrad_launch(dtype, xt, cond, dy, dw, part, nblk, B, V, F, Fx, Fc, H, W, Co, KS, accumulate, stream);
  if (dtype != CESM_DT_F32 && dtype != CESM_DT_BF16) return CESM_EINVAL;
  if (!xt || !cond || !dy || !dw || !part || nblk <= 0) return CESM_EINVAL;
  if (!mc_stem_shape_ok(V, Cc, B, F, Fx, Fc, H, W, Co, KS)) return CESM_EUNSUPPORTED;
  const int64_t nt = (int64_t)B * F * cdiv(H, 8) * cdiv(W, 32);
  if (nt > 0x7fffffff) return CESM_EUNSUPPORTED;
  const int P = V + Cc, NP = (P + 1) / 2;
  if (dtype == CESM_DT_BF16) {
    dim3 grid(nblk, Co / 64);
#define MC_WG(N)                                                                                                     \
  mc_stem_wgrad_mfma_kernel<N><<<grid, 256, 0, stream>>>(xt, cond, (const bf16*)dy, part, V, Cc, F, Fx, Fc, H, W, Co, \
                                                         KS, (int)nt)
    switch (NP) {
      case 2: MC_WG(2); break;
      case 3: MC_WG(3); break;
      default: MC_WG(4);
    }
#undef MC_WG
  } else {
    dim3 grid(nblk, Co / 64, NP);
    mc_stem_wgrad_kernel<<<grid, 256, 0, stream>>>(xt, cond, (const float*)dy, part, V, Cc, F, Fx, Fc, H, W, Co, KS,
                                                   (int)nt);
  }
  const int64_t n = (int64_t)Co * P * KS * KS;
  sum_partials_kernel<<<(unsigned)cdiv(n, 64), 1024, 0, stream>>>(part, dw, nblk, n, accumulate);
  return cesm_launch_status();
}

static inline int mc_stem_dgrad_launch(int dtype, const void* dy, const float* w, float* dxt, float* dcond, int B, int V,
                                       int Cc, int F, int Fx, int Fc, int H, int W, int Co, int KS, hipStream_t stream) {
  if (Cc == V) return mv_stem_dgrad_launch(dtype, dy, w, dxt, dcond, B, V, F, Fx, Fc, H, W, Co, KS, stream);
  if (dtype != CESM_DT_F32 && dtype != CESM_DT_BF16) return CESM_EINVAL;
  if (B <= 0 || F <= 0 || H <= 0 || W <= 0 || !dy || !w) return CESM_EINVAL;
  if (!mc_stem_shape_ok(V, Cc, B, F, Fx, Fc, H, W, Co, KS) || B > 65535 || F > 65535) return CESM_EUNSUPPORTED;
  if (!dxt && !dcond) return CESM_OK;
  const int64_t tiles = cdiv(H, MV_TS) * cdiv(W, MV_TS);
  if (tiles > 0x7fffffff) return CESM_EUNSUPPORTED;
  // the frame split of mv_stem_dgrad_launch
  const bool bcast = (dxt && Fx != F) || (dcond && Fc != F);
  int fpb = F;
  if (!bcast) {
    const int64_t fz = std::min<int64_t>(F, std::max<int64_t>(1, cdiv(4 * (int64_t)cesm_num_cus(), tiles * B)));
    fpb = (int)cdiv(F, fz);
  }
  dim3 grid((unsigned)tiles, (unsigned)B, (unsigned)cdiv(F, fpb));
  const int P = V + Cc;
  if (dtype == CESM_DT_BF16) {
    if (hipFuncSetAttribute((const void*)mc_stem_dgrad_mfma_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                            MD_LDS_MAX) != hipSuccess)
      return CESM_ELAUNCH;
    const int lds = (MD_HALO + KS * KS * 2 * P * 32) * 2;
    mc_stem_dgrad_mfma_kernel<<<grid, 256, lds, stream>>>((const bf16*)dy, w, dxt, dcond, V, Cc, F, Fx, Fc, H, W, Co,
                                                          KS, fpb);
  } else {
    const float* d = (const float*)dy;
#define MC_DG(N) mc_stem_dgrad_kernel<N><<<grid, 256, 0, stream>>>(d, w, dxt, dcond, V, F, Fx, Fc, H, W, Co, KS, fpb)
    switch (P) {
      case 3: MC_DG(3); break;
      case 4: MC_DG(4); break;
      case 5: MC_DG(5); break;
      case 6: MC_DG(6); break;
      default: MC_DG(7);
    }
#undef MC_DG
  }
  return cesm_launch_status();
}
