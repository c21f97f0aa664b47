// Data gradient of the stem: the adjoint of Conv3d(2 -> Co, (1,KS,KS), pad KS/2) on cat([x_t, cond]) (the forward:
// stem_fwd_kernel, stem_head.hip, which includes this header), for input gradients (saliency, guidance).  Off the
// training path.
//
//   dX_ci[b][f'][y][x] = sum_{f -> f'} sum_{co,ky,kx} w[co][ci][ky][kx] * dy[b,f][y - ky + P][x - kx + P][co]
//
// dy [B*F][H][W][Co] in the compute dtype, w the fp32 master weight [Co][2][KS][KS]; dxt [B][Fx][H][W] and dcond
// [B][Fc][H][W] fp32, overwritten, each nullable.  An input the forward broadcast over frames (Fx or Fc == 1 with
// F > 1: frame 0 read with stride 0) gets the sum over all F frames.
//
// Both kernels: block = one 16x16 output tile of one sample and a run of frames [f0, f1).  The block loops over its
// frames with the two accumulators (ci = 0, 1) of every pixel in registers; an input with F frames is stored and reset
// after every frame, a broadcast input is stored once after the last frame.  The host gives a block every frame
// (gridDim.z = 1) whenever a requested output is a broadcast one, so every output element is written by exactly one
// thread, summed in a fixed order (frames ascending, 64-channel groups ascending): no atomics, bit-reproducible.
// All Co channels are reduced inside the block for the same reason (the forward splits Co over gridDim.y instead).
//
// Out-of-image dy counts as zero: halo loads read a clamped in-bounds address and select afterwards.
#pragma once
#include <algorithm>

#include "common.h"

namespace {

constexpr int SD_TS = 16;   // output tile
constexpr int SD_TWM = 22;  // halo width at KS = 7 (row stride of the LDS halos for every KS)

// where frame f of an input with Fi frames lands (Fi == F: frame f; broadcast: frame 0)
__device__ __forceinline__ float* sd_dst(float* base, int b, int Fi, int f, int F, int H, int W, int y, int x) {
  return base + (((int64_t)b * Fi + (Fi == F ? f : 0)) * H + y) * W + x;
}

// fp32 mode: plain VALU, one output pixel per thread.  dy is staged 16 channels at a time ([c][22][22] fp32, 30 KB)
// with those channels' 2*KS*KS weights; a lane's halo reads are consecutive addresses, the weight reads broadcasts.
constexpr int SD_CC = 16;
__global__ __launch_bounds__(256) void stem_dgrad_kernel(const float* __restrict__ dy, const float* __restrict__ w,
                                                         float* __restrict__ dxt, float* __restrict__ dcond, int F,
                                                         int Fx, int Fc, int H, int W, int Co, int KS, int fpb) {
  __shared__ float tdy[SD_CC][SD_TWM * SD_TWM];
  __shared__ float tw[SD_CC * 2 * 49];
  const int PAD = KS / 2, TW = SD_TS + KS - 1, KK = KS * KS;
  const int tid = threadIdx.x, py = tid / SD_TS, px = tid % SD_TS;
  const int tiles_x = (W + SD_TS - 1) / SD_TS;
  const int ty0 = ((int)blockIdx.x / tiles_x) * SD_TS, tx0 = ((int)blockIdx.x % tiles_x) * SD_TS;
  const int b = blockIdx.y;
  const int f0 = blockIdx.z * fpb, f1 = min(F, f0 + fpb);
  const int oy = ty0 + py, ox = tx0 + px;
  const bool inside = oy < H && ox < W;
  float a0 = 0.f, a1 = 0.f;
  for (int f = f0; f < f1; ++f) {
    const float* src = dy + (int64_t)(b * F + f) * H * W * Co;
    for (int c0 = 0; c0 < Co; c0 += SD_CC) {
      __syncthreads();  // the previous chunk's readers are done
      for (int e = tid; e < TW * TW * (SD_CC / 4); e += 256) {
        const int p = e / (SD_CC / 4), q = e % (SD_CC / 4);
        const int hy = p / TW, hx = p - hy * TW;
        const int yy = ty0 - PAD + hy, xx = tx0 - PAD + hx;
        const bool ok = yy >= 0 && yy < H && xx >= 0 && xx < W;
        const int64_t o = ok ? ((int64_t)yy * W + xx) * Co + c0 + q * 4 : 0;  // clamped: element 0 of the frame
        const f32x4 v = *reinterpret_cast<const f32x4*>(src + o);
#pragma unroll
        for (int i = 0; i < 4; ++i) tdy[q * 4 + i][hy * SD_TWM + hx] = ok ? v[i] : 0.f;
      }
      for (int e = tid; e < SD_CC * 2 * KK; e += 256) tw[e] = w[(int64_t)c0 * 2 * KK + e];
      __syncthreads();
      for (int c = 0; c < SD_CC; ++c) {
        const float* w0 = tw + (c * 2) * KK;
        const float* w1 = w0 + KK;
        for (int ky = 0; ky < KS; ++ky) {
          const float* row = &tdy[c][(py + KS - 1 - ky) * SD_TWM + px + KS - 1];
          for (int kx = 0; kx < KS; ++kx) {
            const float v = row[-kx];
            a0 = fmaf(w0[ky * KS + kx], v, a0);
            a1 = fmaf(w1[ky * KS + kx], v, a1);
          }
        }
      }
    }
    if (Fx == F) {
      if (dxt && inside) *sd_dst(dxt, b, Fx, f, F, H, W, oy, ox) = a0;
      a0 = 0.f;
    }
    if (Fc == F) {
      if (dcond && inside) *sd_dst(dcond, b, Fc, f, F, H, W, oy, ox) = a1;
      a1 = 0.f;
    }
  }
  if (Fx != F && dxt && inside) *sd_dst(dxt, b, Fx, 0, F, H, W, oy, ox) = a0;
  if (Fc != F && dcond && inside) *sd_dst(dcond, b, Fc, 0, F, H, W, oy, ox) = a1;
}

// bf16 mode on MFMA: implicit GEMM D[ci][px] = sum_k W'[ci][k] dYhalo[k][px], k = (ky, kx, co): per 64-channel
// group KS*KS*2 K-steps of 32 channels (98 at KS = 7).  The two ci rows sit in rows 0 / 1 of the 16-row A fragment
// (rows 2-15 are zero: 7/8 of the MFMA rows are idle; the leaner form puts (ci, kx) on that axis).
//   halo  bf16 [22*22 px][64 co], 62 KB: a pixel's 8 16-B chunks XOR-swizzled with (px index & 7), so the B
//         fragments (16 B per lane, 16 consecutive pixels x 4 chunks) are conflict-free ds_read_b128
//   wimg  bf16 [KS*KS taps][2 halves][2 ci][32 co], 12.25 KB: the weight of the current 64-channel group, converted
//         once per block when Co == 64, else once per (frame, group)
// Wave w owns tile rows 4w..4w+3 (4 groups of 16 px).  Results: lanes 0-15 (lg = 0), registers 0 / 1 = ci.
constexpr int SD_HALO = SD_TWM * SD_TWM * 64;  // bf16 elements
constexpr int SD_WIMG = 49 * 2 * 2 * 32;
constexpr int SD_MFMA_LDS = (SD_HALO + SD_WIMG) * 2;  // bytes
__global__ __launch_bounds__(256) void stem_dgrad_mfma_kernel(const bf16* __restrict__ dy, const float* __restrict__ w,
                                                              float* __restrict__ dxt, float* __restrict__ dcond, int F,
                                                              int Fx, int Fc, int H, int W, int Co, int KS, int fpb) {
  extern __shared__ __attribute__((aligned(16))) bf16 sd_lds[];
  bf16* halo = sd_lds;
  bf16* wimg = sd_lds + SD_HALO;
  const int PAD = KS / 2, TW = SD_TS + KS - 1, KK = KS * KS;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int lr = lane & 15, lg = lane >> 4;
  const int tiles_x = (W + SD_TS - 1) / SD_TS;
  const int ty0 = ((int)blockIdx.x / tiles_x) * SD_TS, tx0 = ((int)blockIdx.x % tiles_x) * SD_TS;
  const int b = blockIdx.y;
  const int f0 = blockIdx.z * fpb, f1 = min(F, f0 + fpb);
  const int ngrp = Co / 64;
  f32x4 acc[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
  bf16x8 zero8;
#pragma unroll
  for (int i = 0; i < 8; ++i) zero8[i] = (bf16)0.f;
  // halo pixel of (tile row wid*4, column lr) at tap (ky, kx) = (KS-1, KS-1); other rows / taps are offsets of it
  const int pbase = (wid * 4 + KS - 1) * SD_TWM + lr + KS - 1;
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
        const int pix = hy * SD_TWM + hx;
        *reinterpret_cast<bf16x8*>(halo + pix * 64 + ((ch ^ (pix & 7)) << 3)) = ok ? v : zero8;
      }
      if (ngrp > 1 || f == f0) {
        for (int e = tid; e < KK * 128; e += 256) {
          const int c = e & 31, ci = (e >> 5) & 1, h = (e >> 6) & 1, tap = e >> 7;
          wimg[e] = (bf16)w[((int64_t)(g * 64 + h * 32 + c) * 2 + ci) * KK + tap];
        }
      }
      __syncthreads();
      for (int ky = 0; ky < KS; ++ky)
        for (int kx = 0; kx < KS; ++kx) {
          const int tap = ky * KS + kx;
          const int p0 = pbase - ky * SD_TWM - kx;
#pragma unroll
          for (int h = 0; h < 2; ++h) {
            // A: row lr = ci (rows >= 2 zero), k = lg*8 + e = channel h*32 + lg*8 + e of this tap
            const bf16x8 av = *reinterpret_cast<const bf16x8*>(wimg + ((tap * 2 + h) * 2 + (lr & 1)) * 32 + lg * 8);
            const bf16x8 a = lr < 2 ? av : zero8;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              const int pix = p0 + j * SD_TWM;
              const bf16x8 bv = *reinterpret_cast<const bf16x8*>(halo + pix * 64 + (((h * 4 + lg) ^ (pix & 7)) << 3));
              acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, bv, acc[j], 0, 0, 0);
            }
          }
        }
    }
    // lane (lg = 0, lr): D[ci = r][px = lr] of tile row wid*4 + j
    const bool last = f == f1 - 1;
    const bool st0 = dxt && (Fx == F || last), st1 = dcond && (Fc == F || last);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int oy = ty0 + wid * 4 + j, ox = tx0 + lr;
      if (lg == 0 && oy < H && ox < W) {
        if (st0) *sd_dst(dxt, b, Fx, f, F, H, W, oy, ox) = acc[j][0];
        if (st1) *sd_dst(dcond, b, Fc, f, F, H, W, oy, ox) = acc[j][1];
      }
      if (Fx == F) acc[j][0] = 0.f;
      if (Fc == F) acc[j][1] = 0.f;
    }
  }
}

}  // namespace

// host launcher of cesm_stem_dgrad (the ABI entry is in stem_head.hip)
static inline int stem_dgrad_launch(int dtype, const void* dy, const float* w, float* dxt, float* dcond, int B, int F,
                                    int Fx, int Fc, int H, int W, int Co, int KS, hipStream_t stream) {
  if (dtype != CESM_DT_F32 && dtype != CESM_DT_BF16) return CESM_EINVAL;
  if (B <= 0 || F <= 0 || H <= 0 || W <= 0 || !dy || !w) return CESM_EINVAL;
  if (KS < 1 || KS > 7 || !(KS & 1) || Co <= 0 || Co % 64 || (Fx != 1 && Fx != F) || (Fc != 1 && Fc != F) ||
      B > 65535 || F > 65535)
    return CESM_EUNSUPPORTED;
  if (!dxt && !dcond) return CESM_OK;
  const int64_t tiles = cdiv(H, SD_TS) * cdiv(W, SD_TS);
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
    if (hipFuncSetAttribute((const void*)stem_dgrad_mfma_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                            SD_MFMA_LDS) != hipSuccess)
      return CESM_ELAUNCH;
    stem_dgrad_mfma_kernel<<<grid, 256, SD_MFMA_LDS, stream>>>((const bf16*)dy, w, dxt, dcond, F, Fx, Fc, H, W, Co, KS,
                                                               fpb);
  } else {
    stem_dgrad_kernel<<<grid, 256, 0, stream>>>((const float*)dy, w, dxt, dcond, F, Fx, Fc, H, W, Co, KS, fpb);
  }
  return cesm_launch_status();
}
