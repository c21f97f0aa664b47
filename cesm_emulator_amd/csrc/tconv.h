// Temporal-convolution blocks (UNet(use_temp_attn=False)): Residual(PreNorm(TemporalCNN)) over the frame axis,
// forward and backward.  Included from norm.hip (after its LayerNorm kernels, which the fp32 parity path reuses); the
// ABI entries are at the end of that file.
//
//   n = LN_C(x) * gamma                                    (per voxel, biased variance)
//   y[b,f,p,:]  = x[b,f,p,:] + bias + sum_k W[:,:,k] n[b,f+k-1,p,:]      (n = 0 outside 0 <= f < F)
//   dn[b,f,p,:] = sum_k W[:,:,k]^T dy[b,f-k+1,p,:]
//   dW[:,:,k]   = sum_{b,f,p} dy[b,f,p,:] (x) n[b,f+k-1,p,:]             db = sum dy
//   dx = LN^T(dn) + dy                                                   dgamma = sum dn * xhat
//
// x, y, dy, dx: [B*F][HW][C] channels-last.  The weight comes packed by cesm_conv_pack as a 1 x 3 conv: Wp[m][tap][k]
// (m = the GEMM's output channel), forward image (swap = flip = 0): Wp[co][t][ci] = W[co][ci][t]; backward image
// (swap = flip = 1): Wp[ci][t][co] = W[co][ci][2 - t], so dn is the same three-tap frame GEMM over dy.
//
// bf16 (tconv_mfma_kernel, forward and dx): a block owns TC_PT pixels of one sample over a run of TC_FR frames.  Every
// frame's rows go through a four-slot LDS ring once (forward: normalised, fp32 statistics, rounded to bf16; backward:
// dy as read), frame f + 2 is fetched while frame f is computed, and the ring's +-1-frame halo is the only data a run
// reads twice.  A wave holds the A fragments (weights) of its output-channel tiles in registers for the whole block
// (C <= 128; at C = 256 they are re-read from L2 per frame) and multiplies them with the B fragments (16 pixels x 32
// channels, one ds_read_b128) of up to three ring slots into one fp32 accumulator: D[channel row 4 lg + r][pixel lr].
// Taps
// whose frame lies outside the sample are skipped (uniform branch); pixels past HW are zero rows and are never stored.
// Forward epilogue: + bias + x (an 8-byte re-read of rows this block just fetched: L2) -> y.  Backward epilogue: dn
// (fp32) through LDS to the row-per-lane-group layout of the LayerNorm backward, which adds dy (from the ring), writes
// dx with 16-byte stores and keeps per-thread dgamma / db partial sums (db in double), written as one row of `part` per
// block and summed over blocks in a fixed order.
//
// dW (tconv_wgrad_kernel, bf16): a second launch.  Persistent blocks, each a (64 x 64) slice pair of (co, ci), walk
// (sample, 32-pixel tile) items over all frames, re-derive n from x and the saved (mean, rstd), and accumulate
// dW[:, :, t] += dy[f]^T n[f + t - 1] with K = the tile's 32 pixels (both operands by the hardware transpose read);
// the 3 x 64 x 64 accumulators stay in registers and leave as one fp32 slab per block, summed in a fixed order.
//
// fp32 (parity path): LayerNorm kernels of norm.hip + plain FMA kernels; correct, not fast.

namespace {

constexpr int TC_FR = 16;  // frames per run of the bf16 forward / dx kernels
__host__ __device__ constexpr int tc_pt(int C) { return C == 64 ? 64 : 32; }  // pixels per tile

// 16-byte chunk swizzle of a ring row (conflict-free ds_read_b128 of 16 rows x one chunk and row-contiguous writes)
template <int C>
__device__ __forceinline__ int tc_sw(int row) { return C == 64 ? (row >> 1) & 7 : row & 15; }
template <int C>
__device__ __forceinline__ int tc_off(int row, int chunk) { return row * C + ((chunk ^ tc_sw<C>(row)) << 3); }

template <int C, bool BWD>
struct TcLds {
  static constexpr int PT = tc_pt(C);
  static constexpr int RING = 4 * PT * C * 2;                      // bytes
  static constexpr int DNLD = C + 4;                               // fp32 dn row stride
  static constexpr int DN = BWD ? PT * DNLD * 4 : 0;
  static constexpr int RED = BWD ? 256 * 8 * 8 : 0;                // block reduction of the dgamma / db partial sums
  static constexpr int TAIL = DN > RED ? DN : RED;
  static constexpr int BYTES = RING + TAIL;
};

// forward (BWD = false): src = x, out = y, mr written when non-null.  backward: src = dy, out = dx, x / mr read.
template <int C, bool BWD>
__global__ __launch_bounds__(256) void tconv_mfma_kernel(const bf16* __restrict__ x, const bf16* __restrict__ dy,
                                                         const float* __restrict__ gamma, const bf16* __restrict__ wp,
                                                         const float* __restrict__ bias, bf16* __restrict__ out,
                                                         float* __restrict__ mr, float* __restrict__ part, int F, int HW,
                                                         float eps) {
  using Lds = TcLds<C, BWD>;
  constexpr int PT = Lds::PT, L = C / 8, KT = C / 32, TPW = C / 64, NSUB = PT / 16, NCH = PT * L / 256;
  constexpr bool WREG = C <= 128;
  static_assert(NCH >= 1 && 256 % L == 0, "tconv tile");
  __shared__ __attribute__((aligned(16))) char lds[Lds::BYTES];
  static_assert(Lds::RING % 16 == 0, "tail alignment");
  bf16* ring = reinterpret_cast<bf16*>(lds);
  float* tail = reinterpret_cast<float*>(lds + Lds::RING);

  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, lr = lane & 15, lg = lane >> 4;
  const int sub = tid % L, vl = tid / L;  // LN role: chunk `sub` of tile rows vl, vl + 256 / L, ...
  const int p0 = blockIdx.x * PT;
  const int f0 = blockIdx.y * TC_FR, f1 = min(F, f0 + TC_FR);
  const int64_t vb = (int64_t)blockIdx.z * F * HW;  // first voxel of the sample
  const bf16* src = BWD ? dy : x;

  float ga[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) ga[i] = gamma[sub * 8 + i];

  // wave w owns the channel tiles w, w + 4, .. and every 16-pixel sub-tile.  (Measured against the other split at
  // C = 64 -- a wave owning 16 pixels and all four channel tiles, each B fragment read by one wave instead of four,
  // 16-byte epilogue accesses: 96 more weight registers, 2 instead of 4 waves per SIMD, forward 584 vs 509 us at the
  // bench shape, profiles/tconv_wave_split_ab.txt.)
  // weight row of this lane in its tile tw, first of the lane's four output channels there, tile row of sub-tile s
  auto arow = [&](int tw) { return (wid + 4 * tw) * 16 + lr; };
  auto dch = [&](int tw) { return (wid + 4 * tw) * 16 + lg * 4; };
  auto prow = [&](int sidx) { return sidx * 16 + lr; };
  // A fragments, lane (lr, lg): weight row arow(tw), k = 32 ks + 8 lg .. + 7
  bf16x8 afr[WREG ? TPW * 3 * KT : 1];
  if constexpr (WREG) {
#pragma unroll
    for (int tw = 0; tw < TPW; ++tw)
#pragma unroll
      for (int t = 0; t < 3; ++t)
#pragma unroll
        for (int ks = 0; ks < KT; ++ks)
          afr[(tw * 3 + t) * KT + ks] = *reinterpret_cast<const bf16x8*>(
              wp + ((int64_t)arow(tw) * 3 + t) * C + ks * 32 + lg * 8);
  }

  bf16x8 raw[NCH];
  const bf16x8 zero8 = {0, 0, 0, 0, 0, 0, 0, 0};
  // fetch frame g's rows of the tile (zeros for frames outside the sample and pixels past HW)
  auto fetch = [&](int g) {
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
      const int p = p0 + vl + i * (256 / L);
      raw[i] = (g >= 0 && g < F && p < HW) ? *reinterpret_cast<const bf16x8*>(src + ((vb + (int64_t)g * HW + p) * C + sub * 8))
                                           : zero8;
    }
  };
  // fetched rows -> ring slot g & 3 (forward: normalised; the frames of this run also write their statistics)
  auto stage = [&](int g) {
    bf16* slot = ring + (g & 3) * (PT * C);
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
      const int row = vl + i * (256 / L);
      bf16x8 v = raw[i];
      if constexpr (!BWD) {
        float a[8];
        float s = 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) { a[j] = (float)v[j]; s += a[j]; }
        s = group_sum(s, L);
        const float mean = s / C;
        float q = 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) { const float d = a[j] - mean; q = fmaf(d, d, q); }
        q = group_sum(q, L);
        const float rstd = 1.f / sqrtf(q / C + eps);
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = (bf16)((a[j] - mean) * rstd * ga[j]);
        const int p = p0 + row;
        if (mr && sub == 0 && g >= f0 && g < f1 && p < HW) {
          const int64_t vi = vb + (int64_t)g * HW + p;
          mr[vi * 2] = mean;
          mr[vi * 2 + 1] = rstd;
        }
      }
      *reinterpret_cast<bf16x8*>(slot + tc_off<C>(row, sub)) = v;
    }
  };

  for (int g = f0 - 1; g <= f0 + 1; ++g) {
    fetch(g);
    stage(g);
  }
  __syncthreads();

  // per-thread partial sums of dgamma (dn * xhat) and db (dy).  db in double: it is a plain sum of the inputs, so its
  // only error is the accumulation's, and the double chain (thread, block, blocks) makes the result correctly rounded
  float pg[8];
  double pb[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) { pg[i] = 0.f; pb[i] = 0.0; }
  const f32x4 z4 = {0.f, 0.f, 0.f, 0.f};

  for (int f = f0; f < f1; ++f) {
    const bool more = f + 1 < f1;  // frame f + 2 is needed by the next iteration only
    if (more) fetch(f + 2);
    const int64_t vf = vb + (int64_t)f * HW;
    // loads of the epilogues, issued ahead of the MFMAs
    bf16x4 xres[TPW][NSUB];
    float bv[TPW][4];
    bf16x8 xr[NCH];
    float mean[NCH], rstd[NCH];
    if constexpr (!BWD) {
#pragma unroll
      for (int tw = 0; tw < TPW; ++tw) {
        const int co = dch(tw);
        load4(bias + co, bv[tw]);
#pragma unroll
        for (int s = 0; s < NSUB; ++s) {
          const int p = p0 + prow(s);
          const bf16x4 z = {0, 0, 0, 0};
          xres[tw][s] = p < HW ? *reinterpret_cast<const bf16x4*>(x + (vf + p) * C + co) : z;
        }
      }
    } else {
#pragma unroll
      for (int i = 0; i < NCH; ++i) {
        const int p = p0 + vl + i * (256 / L);
        const bool ok = p < HW;
        xr[i] = ok ? *reinterpret_cast<const bf16x8*>(x + (vf + p) * C + sub * 8) : zero8;
        mean[i] = ok ? mr[(vf + p) * 2] : 0.f;
        rstd[i] = ok ? mr[(vf + p) * 2 + 1] : 0.f;
      }
    }

    f32x4 acc[TPW][NSUB];
#pragma unroll
    for (int tw = 0; tw < TPW; ++tw)
#pragma unroll
      for (int s = 0; s < NSUB; ++s) acc[tw][s] = z4;
    const int wz = WREG ? 0 : opaque_zero();  // C = 256: keeps the weight loads inside the frame loop
#pragma unroll
    for (int t = 0; t < 3; ++t) {
      const int g = f + t - 1;
      if (g < 0 || g >= F) continue;  // uniform: the pad is on n (on dy in the backward)
      const bf16* slot = ring + (g & 3) * (PT * C);
#pragma unroll
      for (int ks = 0; ks < KT; ++ks) {
        bf16x8 bfr[NSUB];
#pragma unroll
        for (int s = 0; s < NSUB; ++s)
          bfr[s] = *reinterpret_cast<const bf16x8*>(slot + tc_off<C>(prow(s), ks * 4 + lg));
#pragma unroll
        for (int tw = 0; tw < TPW; ++tw) {
          bf16x8 a;
          if constexpr (WREG) a = afr[(tw * 3 + t) * KT + ks];
          else a = *reinterpret_cast<const bf16x8*>(wp + wz + ((int64_t)arow(tw) * 3 + t) * C + ks * 32 + lg * 8);
#pragma unroll
          for (int s = 0; s < NSUB; ++s) acc[tw][s] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, bfr[s], acc[tw][s], 0, 0, 0);
        }
      }
    }

    if constexpr (!BWD) {
      // lane: channels dch(tw) .. + 3 of pixel prow(s)
#pragma unroll
      for (int tw = 0; tw < TPW; ++tw)
#pragma unroll
        for (int s = 0; s < NSUB; ++s) {
          const int p = p0 + prow(s);
          if (p < HW) {
            float o[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) o[r] = acc[tw][s][r] + bv[tw][r] + (float)xres[tw][s][r];
            store4(out + (vf + p) * C + dch(tw), o);
          }
        }
    } else {
#pragma unroll
      for (int tw = 0; tw < TPW; ++tw)
#pragma unroll
        for (int s = 0; s < NSUB; ++s)
          *reinterpret_cast<f32x4*>(tail + prow(s) * Lds::DNLD + dch(tw)) = acc[tw][s];
      __syncthreads();
      const bf16* dslot = ring + (f & 3) * (PT * C);
#pragma unroll
      for (int i = 0; i < NCH; ++i) {
        const int row = vl + i * (256 / L);
        const int p = p0 + row;
        float dn[8], d[8], xh[8];
        load8(tail + row * Lds::DNLD + sub * 8, dn);
        const bf16x8 dv = *reinterpret_cast<const bf16x8*>(dslot + tc_off<C>(row, sub));
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          xh[j] = ((float)xr[i][j] - mean[i]) * rstd[i];
          d[j] = (float)dv[j];
          const float g = dn[j] * ga[j];
          s1 += g;
          s2 = fmaf(g, xh[j], s2);
          pg[j] = fmaf(dn[j], xh[j], pg[j]);
          pb[j] += (double)d[j];
        }
        s1 = group_sum(s1, L) / C;
        s2 = group_sum(s2, L) / C;
        if (p < HW) {
#pragma unroll
          for (int j = 0; j < 8; ++j) d[j] += rstd[i] * (dn[j] * ga[j] - s1 - xh[j] * s2);
          store8(out + (vf + p) * C + sub * 8, d);
        }
      }
    }
    if (more) stage(f + 2);
    __syncthreads();
  }

  if constexpr (BWD) {
    if (part) {  // uniform
      // block sums per channel, the threads of one chunk column added in a fixed order; a row of part: C floats
      // (dgamma) then C doubles (db)
      const int64_t blk = ((int64_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
      float* prow = part + blk * (3 * C);
      double* taild = reinterpret_cast<double*>(tail);
#pragma unroll
      for (int j = 0; j < 8; ++j) tail[tid * 9 + j] = pg[j];
      __syncthreads();
      for (int c = tid; c < C; c += 256) {
        float s = 0.f;
        for (int k = 0; k < 256 / L; ++k) s += tail[(k * L + (c >> 3)) * 9 + (c & 7)];
        prow[c] = s;
      }
      __syncthreads();
#pragma unroll
      for (int j = 0; j < 8; ++j) taild[tid * 8 + j] = pb[j];
      __syncthreads();
      for (int c = tid; c < C; c += 256) {
        double s = 0.0;
        for (int k = 0; k < 256 / L; ++k) s += taild[(k * L + (c >> 3)) * 8 + (c & 7)];
        reinterpret_cast<double*>(prow + C)[c] = s;
      }
    }
  }
}

// ---------------------------------------------------------------- dW, bf16
constexpr int TW_PT = 32;   // pixels per tile = K of one MFMA
constexpr int TW_LD = 72;   // bf16 row stride of the 64-channel tiles (144 B)

// grid (streams, (C / 64)^2); slab [streams][C][C][3] fp32 (every element written by exactly one pair's block)
__global__ __launch_bounds__(256) void tconv_wgrad_kernel(const bf16* __restrict__ x, const bf16* __restrict__ dy,
                                                          const float* __restrict__ mr, const float* __restrict__ gamma,
                                                          float* __restrict__ slab, int B, int F, int HW, int C) {
  __shared__ __attribute__((aligned(16))) bf16 nring[4][TW_PT * TW_LD];
  __shared__ __attribute__((aligned(16))) bf16 dring[4][TW_PT * TW_LD];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, lr = lane & 15, lg = lane >> 4;
  const int sub = tid & 7, row = tid >> 3;  // staging role: chunk sub of tile row `row`
  const int nsl = C / 64;
  const int co0 = ((int)blockIdx.y / nsl) * 64, ci0 = ((int)blockIdx.y % nsl) * 64;
  const int ntiles = (HW + TW_PT - 1) / TW_PT;
  const int nitems = B * ntiles;
  float ga[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) ga[i] = gamma[ci0 + sub * 8 + i];
  const bf16x8 zero8 = {0, 0, 0, 0, 0, 0, 0, 0};
  const f32x4 z4 = {0.f, 0.f, 0.f, 0.f};
  f32x4 acc[3][4];
#pragma unroll
  for (int t = 0; t < 3; ++t)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[t][j] = z4;
  // transposed fragment read: lane (lg, lr) <- tile[8 lg + 4 half + e][c0 + lr], e = 0..3
  const int tr_row = lg * 8 + (lr >> 2), tr_col = 4 * (lr & 3);
  auto frag = [&](const bf16* tile, int c0) {
    bf16x8 v;
#pragma unroll
    for (int half = 0; half < 2; ++half) {
      const s16x4 h = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
          (LDS_PTR(s16x4))(tile + (tr_row + half * 4) * TW_LD + c0 + tr_col));
#pragma unroll
      for (int e = 0; e < 4; ++e) v[half * 4 + e] = __builtin_bit_cast(bf16, (short)h[e]);
    }
    return v;
  };

  for (int item = blockIdx.x; item < nitems; item += gridDim.x) {
    const int b = item / ntiles, p = (item - b * ntiles) * TW_PT + row;
    const bool pok = p < HW;
    const int64_t vb = (int64_t)b * F * HW + p;
    bf16x8 rx, rd;
    float mean, rstd;
    auto fetch = [&](int g) {
      const bool ok = pok && g < F;
      const int64_t v = vb + (int64_t)g * HW;
      rx = ok ? *reinterpret_cast<const bf16x8*>(x + v * C + ci0 + sub * 8) : zero8;
      rd = ok ? *reinterpret_cast<const bf16x8*>(dy + v * C + co0 + sub * 8) : zero8;
      mean = ok ? mr[v * 2] : 0.f;
      rstd = ok ? mr[v * 2 + 1] : 0.f;
    };
    auto stage = [&](int g) {
      bf16x8 n;
#pragma unroll
      for (int j = 0; j < 8; ++j) n[j] = (bf16)(((float)rx[j] - mean) * rstd * ga[j]);
      *reinterpret_cast<bf16x8*>(&nring[g & 3][row * TW_LD + sub * 8]) = n;
      *reinterpret_cast<bf16x8*>(&dring[g & 3][row * TW_LD + sub * 8]) = rd;
    };
    fetch(0);
    stage(0);
    fetch(1);
    stage(1);
    __syncthreads();
    for (int f = 0; f < F; ++f) {
      if (f + 2 < F) fetch(f + 2);
      const bf16x8 a = frag(dring[f & 3], wid * 16);  // A[co 16 wid + lr][pixel]
#pragma unroll
      for (int t = 0; t < 3; ++t) {
        const int g = f + t - 1;
        if (g < 0 || g >= F) continue;  // uniform
#pragma unroll
        for (int j = 0; j < 4; ++j)
          acc[t][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, frag(nring[g & 3], j * 16), acc[t][j], 0, 0, 0);
      }
      if (f + 2 < F) stage(f + 2);
      __syncthreads();
    }
  }
  // D[co 16 wid + 4 lg + r][ci 16 j + lr] -> slab[stream][co][ci][t]
  float* o = slab + (int64_t)blockIdx.x * C * C * 3;
#pragma unroll
  for (int t = 0; t < 3; ++t)
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        o[((int64_t)(co0 + wid * 16 + lg * 4 + r) * C + ci0 + j * 16 + lr) * 3 + t] = acc[t][j][r];
}

// dst[e] (+)= sum_s src[s * stride + e], s in order (one thread per element: coalesced over e)
__global__ void tconv_reduce_kernel(const float* __restrict__ src, int64_t stride, int ns, float* __restrict__ dst,
                                    int count, int accumulate) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= count) return;
  float s = 0.f;
  for (int k = 0; k < ns; ++k) s += src[(int64_t)k * stride + e];
  dst[e] = accumulate ? dst[e] + s : s;
}
// the same with one wave per element (many rows, few elements): lanes take rows k, k + 64, ..; fixed order
__global__ void tconv_reduce_wave_kernel(const float* __restrict__ src, int64_t stride, int ns, float* __restrict__ dst,
                                         int accumulate) {
  const int e = blockIdx.x;
  float s = 0.f;
  for (int k = threadIdx.x; k < ns; k += 64) s += src[(int64_t)k * stride + e];
  s = wave_sum(s);
  if (threadIdx.x == 0) dst[e] = accumulate ? dst[e] + s : s;
}
// double partial sums (db): row k holds its doubles at float offset `off` of a row of `stride` floats
__global__ void tconv_reduce_wave_d_kernel(const float* __restrict__ src, int64_t stride, int off, int ns,
                                           float* __restrict__ dst, int accumulate) {
  const int e = blockIdx.x;
  double s = 0.0;
  for (int k = threadIdx.x; k < ns; k += 64) s += reinterpret_cast<const double*>(src + (int64_t)k * stride + off)[e];
  s = wave_sum_d(s);
  if (threadIdx.x == 0) dst[e] = accumulate ? dst[e] + (float)s : (float)s;
}

// ---------------------------------------------------------------- fp32 parity kernels
// out[v][m] = (res ? res[v][m] : 0) + (bias ? bias[m] : 0) + sum_t sum_k wp[m][t][k] in[v + (t - 1) HW][k], frames in range
__global__ __launch_bounds__(256) void tconv_gemm_f32_kernel(const float* __restrict__ in, const float* __restrict__ wp,
                                                             const float* __restrict__ bias, const float* __restrict__ res,
                                                             float* __restrict__ out, int64_t V, int F, int HW, int C) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= V * C) return;
  const int64_t v = e / C;
  const int m = (int)(e - v * C);
  const int f = (int)((v / HW) % F);
  float s = 0.f;
  for (int t = 0; t < 3; ++t) {
    const int g = f + t - 1;
    if (g < 0 || g >= F) continue;
    const float* row = in + (v + (int64_t)(t - 1) * HW) * C;
    const float* w = wp + ((int64_t)m * 3 + t) * C;
    for (int k = 0; k < C; ++k) s = fmaf(w[k], row[k], s);
  }
  if (bias) s += bias[m];
  if (res) s += res[e];
  out[e] = s;
}

// grid (ceil(3 C C / 256), ns): slab[s][co][ci][t] = sum over the slab's voxels of dy[v][co] n[v + (t - 1) HW][ci];
// bslab[s][co] = sum dy[v][co] (threads ci = 0, t = 1)
__global__ __launch_bounds__(256) void tconv_wgrad_f32_kernel(const float* __restrict__ dy, const float* __restrict__ n,
                                                              float* __restrict__ slab, float* __restrict__ bslab,
                                                              int64_t V, int F, int HW, int C) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= 3 * C * C) return;
  const int t = e % 3, ci = (e / 3) % C, co = e / (3 * C);
  const int ns = gridDim.y, s = blockIdx.y;
  const int64_t per = (V + ns - 1) / ns;
  const int64_t v0 = s * per, v1 = v0 + per < V ? v0 + per : V;
  float a = 0.f, bsum = 0.f;
  for (int64_t v = v0; v < v1; ++v) {
    const float d = dy[v * C + co];
    bsum += d;
    const int g = (int)((v / HW) % F) + t - 1;
    if (g >= 0 && g < F) a = fmaf(d, n[(v + (int64_t)(t - 1) * HW) * C + ci], a);
  }
  if (slab) slab[(int64_t)s * 3 * C * C + e] = a;  // null: only the bias gradient was asked for
  if (bslab && ci == 0 && t == 1) bslab[(int64_t)s * C + co] = bsum;
}

constexpr int TC_F32_NS = 64;     // voxel slabs of the fp32 weight gradient
constexpr int TC_F32_NBLK = 256;  // blocks (partial rows) of the fp32 LayerNorm backward

bool tconv_ok(int B, int F, int HW, int C) {
  return (C == 64 || C == 128 || C == 256) && B >= 1 && F >= 1 && HW >= 1 && B <= 65535 &&
         (int64_t)B * F * HW < (1ll << 31);
}
int tconv_streams(int B, int HW, int C) {
  const int64_t items = (int64_t)B * cdiv(HW, TW_PT);
  const int64_t cap = 2 * cesm_num_cus();
  return (int)(items < cap ? items : cap);
}
int64_t tconv_blocks(int B, int F, int HW, int C) { return cdiv(HW, tc_pt(C)) * cdiv(F, TC_FR) * B; }

template <int C>
void tconv_fwd_bf16(const void* x, const float* gamma, const void* wp, const float* bias, void* y, float* mr, int B, int F,
                    int HW, float eps, hipStream_t st) {
  const dim3 grid((unsigned)cdiv(HW, tc_pt(C)), (unsigned)cdiv(F, TC_FR), (unsigned)B);
  tconv_mfma_kernel<C, false><<<grid, 256, 0, st>>>((const bf16*)x, nullptr, gamma, (const bf16*)wp, bias, (bf16*)y, mr,
                                                    nullptr, F, HW, eps);
}
template <int C>
void tconv_dx_bf16(const void* x, const void* dy, const float* mr, const float* gamma, const void* wpt, void* dx,
                   float* part, int B, int F, int HW, hipStream_t st) {
  const dim3 grid((unsigned)cdiv(HW, tc_pt(C)), (unsigned)cdiv(F, TC_FR), (unsigned)B);
  tconv_mfma_kernel<C, true><<<grid, 256, 0, st>>>((const bf16*)x, (const bf16*)dy, gamma, (const bf16*)wpt, nullptr,
                                                   (bf16*)dx, const_cast<float*>(mr), part, F, HW, 0.f);
}

int tconv_fwd_launch(int dtype, const void* x, const float* gamma, const void* wp, const float* bias, void* y, float* mr,
                     void* ws, int B, int F, int HW, int C, float eps, hipStream_t st) {
  if (!tconv_ok(B, F, HW, C)) return CESM_EUNSUPPORTED;
  if (!x || !gamma || !wp || !bias || !y) return CESM_EINVAL;
  const int64_t V = (int64_t)B * F * HW;
  if (dtype == CESM_DT_BF16) {
    if (C == 64) tconv_fwd_bf16<64>(x, gamma, wp, bias, y, mr, B, F, HW, eps, st);
    else if (C == 128) tconv_fwd_bf16<128>(x, gamma, wp, bias, y, mr, B, F, HW, eps, st);
    else tconv_fwd_bf16<256>(x, gamma, wp, bias, y, mr, B, F, HW, eps, st);
  } else if (dtype == CESM_DT_F32) {
    if (!ws) return CESM_EINVAL;
    ln_fwd_kernel<float><<<(unsigned)cdiv(V * (C / 8), 256), 256, 0, st>>>((const float*)x, gamma, (float*)ws, mr, V, C,
                                                                           eps, 0, 0);
    tconv_gemm_f32_kernel<<<(unsigned)cdiv(V * C, 256), 256, 0, st>>>((const float*)ws, (const float*)wp, bias,
                                                                      (const float*)x, (float*)y, V, F, HW, C);
  } else {
    return CESM_EINVAL;
  }
  return cesm_launch_status();
}

// floats of `part` / `slab` cesm_tconv_bwd needs
int64_t tconv_part_floats(int dtype, int B, int F, int HW, int C) {
  if (!tconv_ok(B, F, HW, C)) return 0;
  return dtype == CESM_DT_BF16 ? tconv_blocks(B, F, HW, C) * 3 * C : (int64_t)TC_F32_NBLK * C + (int64_t)TC_F32_NS * C;
}
int64_t tconv_slab_floats(int dtype, int B, int F, int HW, int C) {
  if (!tconv_ok(B, F, HW, C)) return 0;
  return (int64_t)(dtype == CESM_DT_BF16 ? tconv_streams(B, HW, C) : TC_F32_NS) * 3 * C * C;
}

int tconv_bwd_launch(int dtype, const void* x, const void* dy, const float* mr, const float* gamma, const void* wpt,
                     void* dx, float* dgamma, float* dw, float* db, float* part, float* slab, void* ws_n, void* ws_dn,
                     int B, int F, int HW, int C, float eps, int accumulate, hipStream_t st) {
  if (!tconv_ok(B, F, HW, C)) return CESM_EUNSUPPORTED;
  if (!x || !dy || !mr || !gamma || !wpt || !dx) return CESM_EINVAL;
  if ((dgamma || db) && !part) return CESM_EINVAL;
  if (dw && !slab) return CESM_EINVAL;
  const int64_t V = (int64_t)B * F * HW;
  if (dtype == CESM_DT_BF16) {
    float* pp = (dgamma || db) ? part : nullptr;
    if (C == 64) tconv_dx_bf16<64>(x, dy, mr, gamma, wpt, dx, pp, B, F, HW, st);
    else if (C == 128) tconv_dx_bf16<128>(x, dy, mr, gamma, wpt, dx, pp, B, F, HW, st);
    else tconv_dx_bf16<256>(x, dy, mr, gamma, wpt, dx, pp, B, F, HW, st);
    const int nblk = (int)tconv_blocks(B, F, HW, C);
    if (dgamma) tconv_reduce_wave_kernel<<<C, 64, 0, st>>>(part, 3 * C, nblk, dgamma, accumulate);
    if (db) tconv_reduce_wave_d_kernel<<<C, 64, 0, st>>>(part, 3 * C, C, nblk, db, accumulate);
    if (dw) {
      const int ns = tconv_streams(B, HW, C);
      const int nsl = C / 64;
      tconv_wgrad_kernel<<<dim3((unsigned)ns, (unsigned)(nsl * nsl)), 256, 0, st>>>((const bf16*)x, (const bf16*)dy, mr,
                                                                                   gamma, slab, B, F, HW, C);
      tconv_reduce_kernel<<<(unsigned)cdiv(3 * C * C, 256), 256, 0, st>>>(slab, (int64_t)3 * C * C, ns, dw, 3 * C * C,
                                                                         accumulate);
    }
  } else if (dtype == CESM_DT_F32) {
    // part: [TC_F32_NBLK][C] rows of the LayerNorm backward (always written), then the bias slabs [TC_F32_NS][C]
    if (!ws_dn || !part || ((dw || db) && !ws_n)) return CESM_EINVAL;
    tconv_gemm_f32_kernel<<<(unsigned)cdiv(V * C, 256), 256, 0, st>>>((const float*)dy, (const float*)wpt, nullptr, nullptr,
                                                                      (float*)ws_dn, V, F, HW, C);
    ln_bwd_kernel<float><<<TC_F32_NBLK, 256, 0, st>>>((const float*)ws_dn, (const float*)x, mr, gamma, (const float*)dy,
                                                      (float*)dx, part, V, C, 0, 0);
    if (dgamma) sum_rows_kernel<<<C, 64, 0, st>>>(part, dgamma, TC_F32_NBLK, C, accumulate);
    if (dw || db) {
      float* bslab = part + (int64_t)TC_F32_NBLK * C;
      ln_fwd_kernel<float><<<(unsigned)cdiv(V * (C / 8), 256), 256, 0, st>>>((const float*)x, gamma, (float*)ws_n, nullptr,
                                                                             V, C, eps, 0, 0);
      tconv_wgrad_f32_kernel<<<dim3((unsigned)cdiv(3 * C * C, 256), TC_F32_NS), 256, 0, st>>>(
          (const float*)dy, (const float*)ws_n, slab, db ? bslab : nullptr, V, F, HW, C);
      if (dw)
        tconv_reduce_kernel<<<(unsigned)cdiv(3 * C * C, 256), 256, 0, st>>>(slab, (int64_t)3 * C * C, TC_F32_NS, dw,
                                                                           3 * C * C, accumulate);
      if (db) tconv_reduce_kernel<<<(unsigned)cdiv(C, 256), 256, 0, st>>>(bslab, C, TC_F32_NS, db, C, accumulate);
    }
  } else {
    return CESM_EINVAL;
  }
  return cesm_launch_status();
}

}  // namespace
