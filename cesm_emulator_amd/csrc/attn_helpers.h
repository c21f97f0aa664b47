// Host-launched helper kernels of the fused attention blocks (tblock.hip, sla_fused.hip): the MFMA A-fragment images
// of their weights and the reduction of their weight-gradient slabs.  Only those two sources include this header, so
// no other code object carries a copy of the kernels.
#pragma once
#include "common.h"

namespace {
// A-operand fragment image of a row-major bf16 matrix A[M][K] (M % 16 == 0, K % 32 == 0) for
// v_mfma_f32_16x16x32_bf16: img[((mt * K/32 + kt) * 64 + lane) * 8 + e] = A[mt*16 + lane%16][kt*32 + (lane/16)*8 + e].
// A wave's fragment load from the image is one contiguous 1-KiB line (vs 16 rows x 64 B from A itself):
// half the vector-memory address work for the per-head weight reloads of slab_dx.
__global__ void frag_image_kernel(const bf16* __restrict__ A, bf16* __restrict__ img, int M, int K) {
  const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;  // 16-B vector of the image
  if (v >= (int64_t)M * K / 8) return;
  const int lane = (int)(v & 63);
  const int64_t tile = v >> 6;
  const int KT = K / 32;
  const int kt = (int)(tile % KT), mt = (int)(tile / KT);
  *reinterpret_cast<bf16x8*>(img + v * 8) =
      *reinterpret_cast<const bf16x8*>(A + (int64_t)(mt * 16 + (lane & 15)) * K + kt * 32 + (lane >> 4) * 8);
}

static inline void frag_image(const void* A, void* img, int M, int K, hipStream_t stream) {
  frag_image_kernel<<<(unsigned)cdiv((int64_t)M * K / 8, 256), 256, 0, stream>>>((const bf16*)A, (bf16*)img, M, K);
}

// fp32 weight -> A-fragment image (frag_image layout) of A = W diag(gamma) (trans = 0: A[m][k] = W[m][k] g[k],
// W row-major [M][K]) or of A = (W diag(gamma))^T (trans = 1: A[m][k] = W[k][m] g[m], W [K][M]).  The first nq rows
// of W (the to_qkv query rows) are multiplied by qscale too: the attention scale folded into the weights, so the
// kernels' q epilogue has no multiply (its gradient is restored in twh_dw_reduce_kernel).
__global__ void frag_image_f32_kernel(const float* __restrict__ W, const float* __restrict__ gamma,
                                      bf16* __restrict__ img, int M, int K, int trans, int nq = 0,
                                      float qscale = 1.f) {
  const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (v >= (int64_t)M * K / 8) return;
  const int lane = (int)(v & 63);
  const int64_t tile = v >> 6;
  const int KT = K / 32;
  const int kt = (int)(tile % KT), mt = (int)(tile / KT);
  const int m = mt * 16 + (lane & 15), k0 = kt * 32 + (lane >> 4) * 8;
  bf16x8 o;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const int k = k0 + e;
    const float w = trans ? W[(int64_t)k * M + m] : W[(int64_t)m * K + k];
    const float gm = gamma ? gamma[trans ? m : k] : 1.f;
    const float qs = (trans ? k : m) < nq ? qscale : 1.f;
    o[e] = (bf16)(w * gm * qs);
  }
  *reinterpret_cast<bf16x8*>(img + v * 8) = o;
}

// slab [nblk][J][C] (dW' partials) -> dW (+)= (sum_blk slab) diag(gamma); tmp[j][c] = W[j][c] * sum_blk slab.
// Rows j < nq were computed against weights carrying qscale (frag_image_f32_kernel): their sums are scaled back.
// Block = 64 elements x 4 slab groups (k = grp mod 4, 8 loads in flight per lane), combined in a fixed order (round 6:
// one element per thread kept too few loads in flight, 64 us for the 50 MB of a level-0 call)
constexpr int TWH_RED_G = 4;
__global__ __launch_bounds__(256) void twh_dw_reduce_kernel(const float* __restrict__ slab, int nblk,
                                                            const float* __restrict__ w, const float* __restrict__ gamma,
                                                            float* __restrict__ dw, float* __restrict__ tmp, int J,
                                                            int C, int accumulate, int nq = 0, float qscale = 1.f) {
  const int64_t JC = (int64_t)J * C;
  const int64_t e = (int64_t)blockIdx.x * 64 + (threadIdx.x & 63);
  const int grp = threadIdx.x >> 6;
  float s = 0.f;
  if (e < JC) {
    int k = grp;
    for (; k + 7 * TWH_RED_G < nblk; k += 8 * TWH_RED_G) {
      float v[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) v[i] = slab[(int64_t)(k + i * TWH_RED_G) * JC + e];
#pragma unroll
      for (int i = 0; i < 8; ++i) s += v[i];
    }
    for (; k < nblk; k += TWH_RED_G) s += slab[(int64_t)k * JC + e];
  }
  __shared__ float red[TWH_RED_G][64];
  red[grp][threadIdx.x & 63] = s;
  __syncthreads();
  if (grp != 0 || e >= JC) return;
  s = ((red[0][threadIdx.x] + red[1][threadIdx.x]) + red[2][threadIdx.x]) + red[3][threadIdx.x];
  if (e / C < nq) s *= qscale;
  const int c = (int)(e % C);
  if (dw) dw[e] = (accumulate ? dw[e] : 0.f) + s * gamma[c];
  tmp[e] = s * w[e];
}
static inline unsigned twh_dw_reduce_grid(int64_t nel) { return (unsigned)((nel + 63) / 64); }
// dgamma[c] (+)= sum_j tmp[j][c]
__global__ void twh_dgamma_kernel(const float* __restrict__ tmp, float* __restrict__ dgamma, int J, int C,
                                  int accumulate) {
  const int c = blockIdx.x;
  float s = 0.f;
  for (int j = threadIdx.x; j < J; j += 256) s += tmp[(int64_t)j * C + c];
  s = wave_sum(s);
  __shared__ float red[4];
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    const float t = red[0] + red[1] + red[2] + red[3];
    dgamma[c] = accumulate ? dgamma[c] + t : t;
  }
}
}  // namespace
