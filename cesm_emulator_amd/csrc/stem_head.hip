// The two ends of the network, which read and write the reference's NCDHW fp32 tensors: the stem, Conv3d(2V -> Co,
// (1,7,7)) on cat([x_t, cond]), and the head, Conv3d(C -> V, 1) on the middle frame; forward, weight gradients and data
// gradients.  Here: the single-variable (V = 1) stem forward and weight gradient and the head; stem_dgrad.h: the V = 1
// stem data gradient; multivar.h: all of them for V = 2 .. 4.  Every ABI entry of the three is at the end of this file.
#include "common.h"
#include "cesm_hip.h"

namespace {

// (ahead of the two headers: the stem weight gradients of this file and of multivar.h both end with it)
// dst[e] (+)= sum_k part[k][e]: block = 64 elements x 16 split groups (each thread sums every 16th split, the
// 16 group sums are added in a fixed order), so a few thousand elements over hundreds of splits still fill the
// chip (one thread per element ran 512 dependent loads: 120 us for the stem's 6272 x 512 partials)
__global__ __launch_bounds__(1024) void sum_partials_kernel(const float* __restrict__ part, float* __restrict__ dst,
                                                            int nsplit, int64_t n, int accumulate) {
  __shared__ float red[16][65];
  const int el = threadIdx.x & 63, kg = threadIdx.x >> 6;
  const int64_t e = blockIdx.x * (int64_t)64 + el;
  float s = 0.f;
  if (e < n)
    for (int k = kg; k < nsplit; k += 16) s += part[(int64_t)k * n + e];
  red[kg][el] = s;
  __syncthreads();
  if (kg == 0 && e < n) {
    float t = 0.f;
#pragma unroll
    for (int q = 0; q < 16; ++q) t += red[q][el];
    dst[e] = accumulate ? dst[e] + t : t;
  }
}

}  // namespace

#include "stem_dgrad.h"
#include "multivar.h"

namespace {

// ----------------------------------------------------------------------------------------
// stem: Conv3d(2 -> Co, (1,7,7), pad 3) on cat([x_t broadcast over F, cond]) (video_net.py:595-600,
// :808-815).  Inputs are the boundary NCDHW fp32 tensors: xt [B][Fx][H][W] (Fx = 1 or F),
// cond [B][Fc][H][W].  Direct VALU conv (0.3 % of the MACs): block = 16x16 output pixels of
// one frame, 64 output channels (Co == 64 at the default base_ch; Co % 64 == 0 handled by grid.y).
// ----------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void stem_fwd_kernel(const float* __restrict__ xt, const float* __restrict__ cond,
                                                       const float* __restrict__ w, const float* __restrict__ bias,
                                                       T* __restrict__ y, int B, int F, int Fx, int Fc, int H, int W,
                                                       int Co, int KS) {
  const int PAD = KS / 2;
  const int TS = 16;
  const int TW = TS + KS - 1;
  __shared__ float tin[2][22 * 22];
  __shared__ float tw[64 * 2 * 49];
  const int n = blockIdx.z;  // b*F + f
  const int b = n / F, f = n - b * F;
  const int ty0 = (blockIdx.x / ((W + TS - 1) / TS)) * TS;
  const int tx0 = (blockIdx.x % ((W + TS - 1) / TS)) * TS;
  const int cog = blockIdx.y * 64;
  const float* s0 = xt + ((int64_t)b * Fx + (Fx == 1 ? 0 : f)) * H * W;
  const float* s1 = cond + ((int64_t)b * Fc + (Fc == 1 ? 0 : f)) * H * W;
  for (int e = threadIdx.x; e < TW * TW; e += 256) {
    const int yy = ty0 - PAD + e / TW, xx = tx0 - PAD + e % TW;
    const bool ok = yy >= 0 && yy < H && xx >= 0 && xx < W;
    tin[0][e] = ok ? s0[(int64_t)yy * W + xx] : 0.f;
    tin[1][e] = ok ? s1[(int64_t)yy * W + xx] : 0.f;
  }
  for (int e = threadIdx.x; e < 64 * 2 * KS * KS; e += 256) tw[e] = w[(int64_t)cog * 2 * KS * KS + e];
  __syncthreads();
  const int py = threadIdx.x / TS, px = threadIdx.x % TS;
  const int oy = ty0 + py, ox = tx0 + px;
  float acc[64];
#pragma unroll
  for (int c = 0; c < 64; ++c) acc[c] = bias[cog + c];
  for (int ci = 0; ci < 2; ++ci)
    for (int ky = 0; ky < KS; ++ky)
      for (int kx = 0; kx < KS; ++kx) {
        const float v = tin[ci][(py + ky) * TW + px + kx];
        const int wo = (ci * KS + ky) * KS + kx;
#pragma unroll
        for (int c = 0; c < 64; ++c) acc[c] = fmaf(tw[c * 2 * KS * KS + wo], v, acc[c]);
      }
  if (oy < H && ox < W) {
    T* dst = y + (((int64_t)n * H + oy) * W + ox) * Co + cog;
#pragma unroll
    for (int c = 0; c < 64; c += 4) store4(dst + c, acc + c);
  }
}

// bf16 stem on MFMA: the same 16x16 output tile / 22x22x2 fp32 input halo in LDS, as an implicit
// GEMM D[co][px] = W[co][k] X[k][px] with k = ci*KS*KS + ky*KS + kx padded to 128 (4 K-steps of 32).
// Wave w owns tile rows 4w..4w+3 (4 fragment groups of 16 px) x 64 co; B fragments are gathered
// straight from the LDS halo (8 taps per lane, converted to bf16), A fragments from the LDS weights.
// Replaces one LDS read per FMA of the VALU kernel (6272 per pixel) with ~100 per pixel.
// Persistent over tiles (round 2): the 64 x 98 weight is staged and converted to A fragments once per block
// (it was once per 256-pixel tile, which dominated: 1.13 ms per level-0 launch), then the block loops over its
// tiles (tile = blockIdx.x + k * gridDim.x) with the fragments in registers.
__global__ __launch_bounds__(256) void stem_fwd_mfma_kernel(const float* __restrict__ xt, const float* __restrict__ cond,
                                                            const float* __restrict__ w, const float* __restrict__ bias,
                                                            bf16* __restrict__ y, int B, int F, int Fx, int Fc, int H,
                                                            int W, int Co, int KS, int ntiles) {
  constexpr int TS = 16, TWM = 22;  // tile and max halo width (KS <= 7)
  __shared__ float tin[2][TWM * TWM];
  __shared__ float tw[64 * 128];    // W[co][k], k padded to 128 with zeros
  const int PAD = KS / 2, TW = TS + KS - 1, KK = KS * KS;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int lr = lane & 15, lg = lane >> 4;
  const int cog = blockIdx.y * 64;
  const int tiles_x = (W + TS - 1) / TS, tiles_img = tiles_x * ((H + TS - 1) / TS);
  for (int e = tid; e < 64 * 128; e += 256) {
    const int co = e >> 7, k = e & 127;
    tw[e] = k < 2 * KK ? w[(int64_t)(cog + co) * 2 * KK + k] : 0.f;
  }
  __syncthreads();
  // A fragments: W[ct*16 + lr][ks*32 + lg*8 + e]
  bf16x8 af[4][4];
#pragma unroll
  for (int ct = 0; ct < 4; ++ct)
#pragma unroll
    for (int ks = 0; ks < 4; ++ks)
#pragma unroll
      for (int e = 0; e < 8; ++e) af[ct][ks][e] = (bf16)tw[(ct * 16 + lr) * 128 + ks * 32 + lg * 8 + e];
  // per-lane LDS offset of tap k (relative to the pixel's (0,0) tap), -1 for padding taps
  int toff[4][8];
#pragma unroll
  for (int ks = 0; ks < 4; ++ks)
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int k = ks * 32 + lg * 8 + e;
      const int ci = k / KK, r = k - ci * KK, ky = r / KS, kx = r - ky * KS;
      // padding taps (k >= 2 KK) read tap 0: their weights are zero and the halo holds finite values
      toff[ks][e] = k < 2 * KK ? ci * TWM * TWM + ky * TWM + kx : 0;
    }
  float bv[4][4];
#pragma unroll
  for (int ct = 0; ct < 4; ++ct)
#pragma unroll
    for (int r = 0; r < 4; ++r) bv[ct][r] = bias[cog + ct * 16 + lg * 4 + r];
  const float* tbase = &tin[0][0];
  // the next tile's halo values (TW*TW <= 484 <= 2 x 256) are loaded into registers while this tile computes
  float hv[2][2];
  auto fetch = [&](int tile_in) {
    // past the last tile: addresses of tile 0 (in bounds), values zeroed below
    const int tile = tile_in < ntiles ? tile_in : 0;
    const int n = tile / tiles_img, tr = tile - n * tiles_img;
    const int b = n / F, f = n - b * F;
    const int ty0 = (tr / tiles_x) * TS, tx0 = (tr - (tr / tiles_x) * tiles_x) * TS;
    const float* s0 = xt + ((int64_t)b * Fx + (Fx == 1 ? 0 : f)) * H * W;
    const float* s1 = cond + ((int64_t)b * Fc + (Fc == 1 ? 0 : f)) * H * W;
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int e = tid + q * 256;
      const int yy = ty0 - PAD + e / TW, xx = tx0 - PAD + e % TW;
      const bool ok = tile_in < ntiles && e < TW * TW && yy >= 0 && yy < H && xx >= 0 && xx < W;
      const int64_t o = ok ? (int64_t)yy * W + xx : 0;
      const float v0 = s0[o], v1 = s1[o];  // unpredicated loads, selected after
      hv[q][0] = ok ? v0 : 0.f;
      hv[q][1] = ok ? v1 : 0.f;
    }
  };
  if ((int)blockIdx.x < ntiles) fetch(blockIdx.x);
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int n = tile / tiles_img, tr = tile - n * tiles_img;
    const int ty0 = (tr / tiles_x) * TS, tx0 = (tr - (tr / tiles_x) * tiles_x) * TS;
    __syncthreads();  // previous tile's gathers done
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int e = tid + q * 256;
      if (e < TW * TW) {
        tin[0][(e / TW) * TWM + e % TW] = hv[q][0];
        tin[1][(e / TW) * TWM + e % TW] = hv[q][1];
      }
    }
    __syncthreads();
    fetch(tile + gridDim.x);
    f32x4 acc[4][4];
#pragma unroll
    for (int ct = 0; ct < 4; ++ct)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[ct][j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int py = wid * 4 + j, px = lr;  // group j = tile row py, pixel lr
      const int pbase = py * TWM + px;
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        bf16x8 bfr;
#pragma unroll
        for (int e = 0; e < 8; ++e) bfr[e] = (bf16)tbase[pbase + toff[ks][e]];
#pragma unroll
        for (int ct = 0; ct < 4; ++ct) acc[ct][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[ct][ks], bfr, acc[ct][j], 0, 0, 0);
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
        const int co = ct * 16 + lg * 4;
        float v[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = acc[ct][j][r] + bv[ct][r];
        store4(dst + co, v);
      }
    }
  }
}

// stem weight gradient partials: part[blk][co][ci*KS*KS + ky*KS + kx]
template <typename T>
__global__ __launch_bounds__(256) void stem_wgrad_kernel(const float* __restrict__ xt, const float* __restrict__ cond,
                                                         const T* __restrict__ dy, float* __restrict__ part, int B,
                                                         int F, int Fx, int Fc, int H, int W, int Co, int KS,
                                                         int ntiles) {
  const int PAD = KS / 2;
  const int TH = 8, TWD = 32;
  const int IH = TH + KS - 1, IW = TWD + KS - 1;  // 14 x 38
  __shared__ float tin[2][14 * 38];
  __shared__ float tdy[TH * TWD * 65];
  const int KK = 2 * KS * KS;  // 98
  // thread -> (co, tap-group): 64 co x 4 groups
  const int co = threadIdx.x & 63, grp = threadIdx.x >> 6;
  const int tpg = (KK + 3) / 4;
  float acc[25];
  int toff[25];  // LDS offset of each of this thread's taps (-1: none), hoisted out of the pixel loop
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
    const float* s0 = xt + ((int64_t)b * Fx + (Fx == 1 ? 0 : f)) * H * W;
    const float* s1 = cond + ((int64_t)b * Fc + (Fc == 1 ? 0 : f)) * H * W;
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
      tdy[p * 65 + c] = (yy < H && xx < W) ? to_f(dy[(((int64_t)n * H + yy) * W + xx) * Co + cog + c]) : 0.f;
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
  for (int i = 0; i < tpg; ++i) {
    const int kk = grp * tpg + i;
    if (kk < KK) part[((int64_t)blockIdx.x * Co + cog + co) * KK + kk] = acc[i];
  }
}

// bf16 stem dW on MFMA: dW[co][tap] = sum_px dy[px][co] * X[ci][y+ky-P][x+kx-P]  (tap = (ci,ky,kx)).
// Block = 8x32-pixel tiles (grid-stride), 4 waves = 4 output-channel tiles of 16 (Co slice of 64);
// each wave accumulates all <=7 tap tiles (98 taps padded to 112).  k-step = 32 pixels of one row.
//   A = dy^T fragment via ds_read_b64_tr_b16 from the [256 px][64 co] bf16 tile (XOR-swizzled chunks)
//   B = im2col fragment: 8 consecutive x of tap (ci,ky,kx) — read 16-B aligned from kx-shifted bf16
//       copies tin_k[kx][ci][row][32] of the input halo (so every tap's 8-pixel run is aligned)
constexpr int SW_TH = 8, SW_TW = 32;
__device__ __forceinline__ int sw_dy_off(int px, int co) {  // bf16 index in the [256][64] dy tile
  return px * 64 + ((((co >> 3) ^ (px & 7))) << 3) + (co & 7);
}
__global__ __launch_bounds__(256) void stem_wgrad_mfma_kernel(const float* __restrict__ xt, const float* __restrict__ cond,
                                                              const bf16* __restrict__ dy, float* __restrict__ part,
                                                              int F, int Fx, int Fc, int H, int W, int Co, int KS,
                                                              int ntiles) {
  const int PAD = KS / 2;
  const int IH = SW_TH + KS - 1, IW = SW_TW + KS - 1;  // <= 14 x 38
  const int NT = 2 * KS * KS;                          // taps (<= 98)
  __shared__ float tin[2 * 14 * 38];
  __shared__ __attribute__((aligned(16))) bf16 tink[7 * 2 * 14 * SW_TW];
  __shared__ __attribute__((aligned(16))) bf16 tdy[SW_TH * SW_TW * 64];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int lr = lane & 15, lg = lane >> 4;
  const int cog = blockIdx.y * 64;
  // per-lane tap offsets into tink for each of the 7 tap tiles (-1: padded tap)
  int toff[7];
#pragma unroll
  for (int nt = 0; nt < 7; ++nt) {
    const int t = nt * 16 + lr;
    if (t < NT) {
      const int ci = t / (KS * KS), r = t - ci * KS * KS, ky = r / KS, kx = r - ky * KS;
      toff[nt] = ((kx * 2 + ci) * 14 + ky) * SW_TW + lg * 8;
    } else {
      toff[nt] = -1;
    }
  }
  f32x4 acc[7];
#pragma unroll
  for (int nt = 0; nt < 7; ++nt) acc[nt] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int tx_tiles = (W + SW_TW - 1) / SW_TW, ty_tiles = (H + SW_TH - 1) / SW_TH;
  const int per_img = tx_tiles * ty_tiles;
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int n = tile / per_img;
    const int rem = tile - n * per_img;
    const int ty0 = (rem / tx_tiles) * SW_TH, tx0 = (rem % tx_tiles) * SW_TW;
    const int b = n / F, f = n - b * F;
    const float* s0 = xt + ((int64_t)b * Fx + (Fx == 1 ? 0 : f)) * H * W;
    const float* s1 = cond + ((int64_t)b * Fc + (Fc == 1 ? 0 : f)) * H * W;
    __syncthreads();  // previous tile's readers done
    for (int e = tid; e < IH * IW; e += 256) {
      const int yy = ty0 - PAD + e / IW, xx = tx0 - PAD + e % IW;
      const bool ok = yy >= 0 && yy < H && xx >= 0 && xx < W;
      tin[e] = ok ? s0[(int64_t)yy * W + xx] : 0.f;
      tin[IH * IW + e] = ok ? s1[(int64_t)yy * W + xx] : 0.f;
    }
    for (int e = tid; e < SW_TH * SW_TW * 8; e += 256) {  // dy: 256 px x 8 chunks of 8 co
      const int px = e >> 3, ch = e & 7;
      const int yy = ty0 + px / SW_TW, xx = tx0 + px % SW_TW;
      bf16x8 v;
      if (yy < H && xx < W) v = *reinterpret_cast<const bf16x8*>(dy + (((int64_t)n * H + yy) * W + xx) * Co + cog + ch * 8);
      else {
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = (bf16)0.f;
      }
      *reinterpret_cast<bf16x8*>(tdy + sw_dy_off(px, ch * 8)) = v;
    }
    __syncthreads();
    for (int e = tid; e < KS * 2 * IH * SW_TW; e += 256) {  // kx-shifted bf16 copies
      const int x = e % SW_TW, r = e / SW_TW;
      const int row = r % IH, r2 = r / IH, ci = r2 & 1, kx = r2 >> 1;
      tink[((kx * 2 + ci) * 14 + row) * SW_TW + x] = (bf16)tin[ci * IH * IW + row * IW + x + kx];
    }
    __syncthreads();
#pragma unroll 2
    for (int py = 0; py < SW_TH; ++py) {
      // A: dy^T[co = wid*16 + i][px = py*32 + 8g + e]
      bf16x8 a;
      const int q = (lane >> 2) & 3, p4 = (lane & 3) * 4;
#pragma unroll
      for (int hf = 0; hf < 2; ++hf) {
        const int px = py * SW_TW + lg * 8 + hf * 4 + q;
        const s16x4 v = __builtin_amdgcn_ds_read_tr16_b64_v4i16((LDS_PTR(s16x4))(tdy + sw_dy_off(px, wid * 16 + p4)));
#pragma unroll
        for (int e = 0; e < 4; ++e) a[hf * 4 + e] = __builtin_bit_cast(bf16, (short)v[e]);
      }
#pragma unroll
      for (int nt = 0; nt < 7; ++nt) {
        bf16x8 bb;
        if (toff[nt] >= 0) bb = *reinterpret_cast<const bf16x8*>(tink + toff[nt] + py * SW_TW);
        else {
#pragma unroll
          for (int i = 0; i < 8; ++i) bb[i] = (bf16)0.f;
        }
        acc[nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, bb, acc[nt], 0, 0, 0);
      }
    }
  }
  // D[co = wid*16 + 4g + r][tap = nt*16 + i]
#pragma unroll
  for (int nt = 0; nt < 7; ++nt) {
    const int t = nt * 16 + lr;
    if (t >= NT) continue;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int co = cog + wid * 16 + lg * 4 + r;
      part[((int64_t)blockIdx.x * Co + co) * NT + t] = acc[nt][r];
    }
  }
}

// ----------------------------------------------------------------------------------------
// head: Conv3d(C -> 1, 1) evaluated only on frame F//2 (the frame model.py:124-130 keeps).
// out[b][y][x] (fp32 [B,1,H,W]) = bias + sum_c w[c] * x[(b*F+mid)][y][x][c]
// ----------------------------------------------------------------------------------------
template <typename T>
__global__ void head_fwd_kernel(const T* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias,
                                float* __restrict__ out, int B, int F, int HW, int C) {
  // one 64-lane wave per 8 pixels: 8 lanes per pixel, each lane 8 channels (C <= 64*... looped)
  const int64_t gw = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) >> 3;
  const int sub = threadIdx.x & 7;
  const int64_t total = (int64_t)B * HW;
  if (gw >= total) return;
  const int b = (int)(gw / HW);
  const int64_t p = gw - (int64_t)b * HW;
  const T* src = x + (((int64_t)b * F + F / 2) * HW + p) * C;
  float s = 0.f;
  for (int c = sub * 8; c < C; c += 64) {
    float v[8];
    load8(src + c, v);
#pragma unroll
    for (int i = 0; i < 8; ++i) s = fmaf(v[i], w[c + i], s);
  }
  s = group_sum(s, 8);
  if (sub == 0) out[gw] = s + bias[0];
}

// dX = 0 everywhere except frame mid where dX[c] = dout * w[c]
template <typename T>
__global__ void head_dgrad_kernel(const float* __restrict__ dout, const float* __restrict__ w, T* __restrict__ dx,
                                  int B, int F, int HW, int C) {
  const int64_t total = (int64_t)B * F * HW * (C / 8);
  for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
    const int cq = (int)(e % (C / 8));
    const int64_t vox = e / (C / 8);
    const int64_t p = vox % HW;
    const int64_t nf = vox / HW;
    const int f = (int)(nf % F), b = (int)(nf / F);
    float v[8];
    const float g = (f == F / 2) ? dout[(int64_t)b * HW + p] : 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = g * w[cq * 8 + i];
    store8(dx + vox * C + cq * 8, v);
  }
}

// head weight/bias grads: part[blk][c] (c < C) and part[blk][C] = bias.  Thread = (pixel lane pl, 8-channel chunk
// sub): one coalesced pass over the mid frame (the per-channel strided loop it replaces read it C + 1 times:
// 0.5 ms per step); per-block sums over the 32 pixel lanes in a fixed order
template <typename T>
__global__ __launch_bounds__(256) void head_wgrad_kernel(const float* __restrict__ dout, const T* __restrict__ x,
                                                         float* __restrict__ part, int B, int F, int HW, int C,
                                                         int64_t px_per_blk) {
  __shared__ float red[32][65];
  const int64_t total = (int64_t)B * HW;
  const int64_t p0 = blockIdx.x * px_per_blk, p1 = min(total, p0 + px_per_blk);
  const int sub = threadIdx.x & 7, pl = threadIdx.x >> 3;
  for (int c0 = 0; c0 < C; c0 += 64) {
    const bool live = c0 + sub * 8 < C;
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, gs = 0.f;
    for (int64_t q = p0 + pl; q < p1; q += 32) {
      const int b = (int)(q / HW);
      const int64_t p = q - (int64_t)b * HW;
      const float g = dout[q];
      gs += g;
      if (live) {
        float v[8];
        load8(x + (((int64_t)b * F + F / 2) * HW + p) * C + c0 + sub * 8, v);
#pragma unroll
        for (int i = 0; i < 8; ++i) acc[i] = fmaf(g, v[i], acc[i]);
      }
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) red[pl][sub * 8 + i] = acc[i];
    if (sub == 0) red[pl][64] = gs;
    __syncthreads();
    if (threadIdx.x < 65) {
      const int c = threadIdx.x;
      float t = 0.f;
      for (int q = 0; q < 32; ++q) t += red[q][c];
      if (c < 64 && c0 + c < C) part[(int64_t)blockIdx.x * (C + 1) + c0 + c] = t;
      if (c == 64 && c0 == 0) part[(int64_t)blockIdx.x * (C + 1) + C] = t;
    }
    __syncthreads();
  }
}

__global__ void head_reduce_kernel(const float* __restrict__ part, float* __restrict__ dw, float* __restrict__ db,
                                   int nblk, int C, int accumulate) {
  for (int c = threadIdx.x; c <= C; c += blockDim.x) {
    float s = 0.f;
    for (int k = 0; k < nblk; ++k) s += part[(int64_t)k * (C + 1) + c];
    float* d = (c == C) ? db : dw + c;
    *d = accumulate ? *d + s : s;
  }
}

}  // namespace

extern "C" {

int cesm_stem_fwd(int dtype, const float* xt, const float* cond, const float* w, const float* bias, void* y, int B,
                  int F, int Fx, int Fc, int H, int W, int Co, int KS, hipStream_t stream) {
  if (KS > 7 || Co % 64) return CESM_EINVAL;
  dim3 grid((unsigned)(cdiv(H, 16) * cdiv(W, 16)), Co / 64, B * F);
  if (dtype == CESM_DT_BF16 && 2 * KS * KS <= 128) {
    const int ntiles = (int)(cdiv(H, 16) * cdiv(W, 16)) * B * F;
    dim3 gp((unsigned)std::min(ntiles, 4 * cesm_num_cus()), Co / 64);
    stem_fwd_mfma_kernel<<<gp, 256, 0, stream>>>(xt, cond, w, bias, (bf16*)y, B, F, Fx, Fc, H, W, Co, KS, ntiles);
  } else if (dtype == CESM_DT_BF16)
    stem_fwd_kernel<bf16><<<grid, 256, 0, stream>>>(xt, cond, w, bias, (bf16*)y, B, F, Fx, Fc, H, W, Co, KS);
  else if (dtype == CESM_DT_F32)
    stem_fwd_kernel<float><<<grid, 256, 0, stream>>>(xt, cond, w, bias, (float*)y, B, F, Fx, Fc, H, W, Co, KS);
  else
    return CESM_EINVAL;
  return cesm_launch_status();
}

// stem dW (+ bias via cesm_colsum on dy); part: nblk*Co*2*KS*KS floats
int cesm_stem_wgrad(int dtype, const float* xt, const float* cond, const void* dy, float* dw, float* part, int nblk,
                    int B, int F, int Fx, int Fc, int H, int W, int Co, int KS, int accumulate, hipStream_t stream) {
  if (KS > 7 || Co % 64 || nblk <= 0) return CESM_EINVAL;
  const int ntiles = B * F * (int)cdiv(H, 8) * (int)cdiv(W, 32);
  dim3 grid(nblk, Co / 64);
  if (dtype == CESM_DT_BF16)
    stem_wgrad_mfma_kernel<<<grid, 256, 0, stream>>>(xt, cond, (const bf16*)dy, part, F, Fx, Fc, H, W, Co, KS, ntiles);
  else if (dtype == CESM_DT_F32)
    stem_wgrad_kernel<float><<<grid, 256, 0, stream>>>(xt, cond, (const float*)dy, part, B, F, Fx, Fc, H, W, Co, KS,
                                                       ntiles);
  else
    return CESM_EINVAL;
  const int64_t n = (int64_t)Co * 2 * KS * KS;
  sum_partials_kernel<<<(unsigned)cdiv(n, 64), 1024, 0, stream>>>(part, dw, nblk, n, accumulate);
  return cesm_launch_status();
}

int cesm_head_fwd(int dtype, const void* x, const float* w, const float* bias, float* out, int B, int F, int HW, int C,
                  hipStream_t stream) {
  if (C % 8) return CESM_EINVAL;
  const int64_t threads = (int64_t)B * HW * 8;
  const unsigned grid = (unsigned)cdiv(threads, 256);
  if (dtype == CESM_DT_BF16)
    head_fwd_kernel<bf16><<<grid, 256, 0, stream>>>((const bf16*)x, w, bias, out, B, F, HW, C);
  else if (dtype == CESM_DT_F32)
    head_fwd_kernel<float><<<grid, 256, 0, stream>>>((const float*)x, w, bias, out, B, F, HW, C);
  else
    return CESM_EINVAL;
  return cesm_launch_status();
}

// head backward: dx (full [B*F][HW][C]), dw[C], db[1] (via part: nblk*(C+1) floats)
int cesm_head_bwd(int dtype, const float* dout, const void* x, const float* w, void* dx, float* dw, float* db,
                  float* part, int nblk, int B, int F, int HW, int C, int accumulate, hipStream_t stream) {
  if (C % 8 || nblk <= 0) return CESM_EINVAL;
  const int64_t total = (int64_t)B * F * HW * (C / 8);
  const unsigned g1 = (unsigned)std::min<int64_t>(cdiv(total, 256), 8192);
  const int64_t ppb = cdiv((int64_t)B * HW, nblk);
  if (dtype == CESM_DT_BF16) {
    if (dx) head_dgrad_kernel<bf16><<<g1, 256, 0, stream>>>(dout, w, (bf16*)dx, B, F, HW, C);
    if (dw) head_wgrad_kernel<bf16><<<nblk, 256, 0, stream>>>(dout, (const bf16*)x, part, B, F, HW, C, ppb);
  } else if (dtype == CESM_DT_F32) {
    if (dx) head_dgrad_kernel<float><<<g1, 256, 0, stream>>>(dout, w, (float*)dx, B, F, HW, C);
    if (dw) head_wgrad_kernel<float><<<nblk, 256, 0, stream>>>(dout, (const float*)x, part, B, F, HW, C, ppb);
  } else {
    return CESM_EINVAL;
  }
  if (dw) head_reduce_kernel<<<1, 256, 0, stream>>>(part, dw, db, nblk, C, accumulate);
  return cesm_launch_status();
}

// stem data gradient (input gradients; kernels: stem_dgrad.h)
int cesm_stem_dgrad(int dtype, const void* dy, const float* w, float* dxt, float* dcond, int B, int F, int Fx, int Fc,
                    int H, int W, int Co, int KS, hipStream_t stream) {
  return stem_dgrad_launch(dtype, dy, w, dxt, dcond, B, F, Fx, Fc, H, W, Co, KS, stream);
}

// stem and head for V target variables (kernels and launchers: multivar.h; V == 1 runs the entry points above)
int cesm_stem_fwd_mv(int dtype, const float* xt, const float* cond, const float* w, const float* bias, void* y, int B,
                     int V, int F, int Fx, int Fc, int H, int W, int Co, int KS, hipStream_t stream) {
  return mv_stem_fwd_launch(dtype, xt, cond, w, bias, y, B, V, F, Fx, Fc, H, W, Co, KS, stream);
}
int cesm_stem_wgrad_mv(int dtype, const float* xt, const float* cond, const void* dy, float* dw, float* part, int nblk,
                       int B, int V, int F, int Fx, int Fc, int H, int W, int Co, int KS, int accumulate,
                       hipStream_t stream) {
  return mv_stem_wgrad_launch(dtype, xt, cond, dy, dw, part, nblk, B, V, F, Fx, Fc, H, W, Co, KS, accumulate, stream);
}
int cesm_stem_dgrad_mv(int dtype, const void* dy, const float* w, float* dxt, float* dcond, int B, int V, int F, int Fx,
                       int Fc, int H, int W, int Co, int KS, hipStream_t stream) {
  return mv_stem_dgrad_launch(dtype, dy, w, dxt, dcond, B, V, F, Fx, Fc, H, W, Co, KS, stream);
}
int cesm_head_fwd_mv(int dtype, const void* x, const float* w, const float* bias, float* out, int B, int V, int F,
                     int HW, int C, hipStream_t stream) {
  return mv_head_fwd_launch(dtype, x, w, bias, out, B, V, F, HW, C, stream);
}
int cesm_head_bwd_mv(int dtype, const float* dout, const void* x, const float* w, void* dx, float* dw, float* db,
                     float* part, int nblk, int B, int V, int F, int HW, int C, int accumulate, hipStream_t stream) {
  return mv_head_bwd_launch(dtype, dout, x, w, dx, dw, db, part, nblk, B, V, F, HW, C, accumulate, stream);
}

// stem for V target variables and Cc conditioning maps (multivar.h; Cc == V runs the *_mv entry points above)
int cesm_stem_fwd_mc(int dtype, const float* xt, const float* cond, const float* w, const float* bias, void* y, int B,
                     int V, int Cc, int F, int Fx, int Fc, int H, int W, int Co, int KS, hipStream_t stream) {
  return mc_stem_fwd_launch(dtype, xt, cond, w, bias, y, B, V, Cc, F, Fx, Fc, H, W, Co, KS, stream);
}
int cesm_stem_wgrad_mc(int dtype, const float* xt, const float* cond, const void* dy, float* dw, float* part, int nblk,
                       int B, int V, int Cc, int F, int Fx, int Fc, int H, int W, int Co, int KS, int accumulate,
                       hipStream_t stream) {
  return mc_stem_wgrad_launch(dtype, xt, cond, dy, dw, part, nblk, B, V, Cc, F, Fx, Fc, H, W, Co, KS, accumulate,
                              stream);
}
int cesm_stem_dgrad_mc(int dtype, const void* dy, const float* w, float* dxt, float* dcond, int B, int V, int Cc, int F,
                       int Fx, int Fc, int H, int W, int Co, int KS, hipStream_t stream) {
  return mc_stem_dgrad_launch(dtype, dy, w, dxt, dcond, B, V, Cc, F, Fx, Fc, H, W, Co, KS, stream);
}

}  // extern "C"
