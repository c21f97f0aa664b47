// Weight gradients of the implicit-GEMM convolutions of conv_fwd.hip (geometry: ConvGeom, conv_common.h), the column sums
// that give bias gradients, wgrad_plan and the cesm_conv_wgrad* / cesm_colsum ABI.
//
// Weight gradients use a second MFMA kernel (pixel axis = MFMA K) that writes fp32 split-K
// slabs, reduced deterministically by conv_wgrad_reduce into the PyTorch weight layout.
#include "conv_common.h"

namespace {

// ----------------------------------------------------------------------------------------
// weight-gradient kernel: slab[split][co][tap*Cin + ci] = sum over the split's pixels of
//   dY[m][co] * X(m, tap, ci)
// Pixel axis is the MFMA K.  Output tile 64 co x 64 K-columns (one tap, 64 channels).
// ----------------------------------------------------------------------------------------
constexpr int WG_BP = 32;   // pixels per step

template <typename T>
__global__ __launch_bounds__(256) void conv_wgrad_kernel(const T* __restrict__ x1, const T* __restrict__ x2,
                                                         const T* __restrict__ dy1, const T* __restrict__ dy2,
                                                         float* __restrict__ slab, ConvGeom g, int64_t M,
                                                         int64_t px_per_split) {
  // LDS tiles are [pixel][64] row-major; bf16 rows are XOR-swizzled in 8-byte chunks so the
  // transposed reads (ds_read_b64_tr_b16) are conflict free.
  constexpr int VEC = sizeof(T) == 2 ? 8 : 4;
  constexpr int ROW = 64;                    // elements per row
  constexpr int LDR = sizeof(T) == 2 ? 64 : 65;
  __shared__ __attribute__((aligned(16))) T tY[2][WG_BP * LDR];
  __shared__ __attribute__((aligned(16))) T tX[2][WG_BP * LDR];

  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int wr = wid >> 1, wc = wid & 1;       // wave owns co [wr*32,+32) x kcol [wc*32,+32)
  const int Cin = g.C1 + g.C2;
  const int co0 = blockIdx.x * 64;
  const int kcol0 = blockIdx.y * 64;           // global K column (tap*Cin + ci)
  const int tap = kcol0 / Cin;
  const int ci0 = kcol0 - tap * Cin;
  const int ky = tap / g.KW, kx = tap - ky * g.KW;
  const int64_t pbeg = (int64_t)blockIdx.z * px_per_split;
  const int64_t pend = min(M, pbeg + px_per_split);

  const T* xs; int xcs, xcc;
  if (ci0 < g.C1) { xs = x1; xcs = g.C1; xcc = ci0; } else { xs = x2; xcs = g.C2; xcc = ci0 - g.C1; }
  const T* ys; int ycs, ycc;
  const int Co2 = g.Cout - g.Co1;
  if (co0 < g.Co1) { ys = dy1; ycs = g.Co1; ycc = co0; } else { ys = dy2; ycs = Co2; ycc = co0 - g.Co1; }

  constexpr int VPR = ROW / VEC;             // 8 (bf16) / 16 (f32) vectors per row
  constexpr int RPP = 256 / VPR;             // rows per pass: 32 / 16
  constexpr int NP = WG_BP / RPP;            // passes: 1 / 2
  const int vrow = tid / VPR, vcol = (tid % VPR) * VEC;

  float xr[NP][VEC], yr[NP][VEC];
  auto gload = [&](int64_t p0) {
#pragma unroll
    for (int p = 0; p < NP; ++p) {
      const int64_t m = p0 + vrow + p * RPP;
      bool ok = m < pend;
      if (ok) {
        if constexpr (VEC == 8) load8(ys + m * ycs + ycc + vcol, yr[p]); else load4(ys + m * ycs + ycc + vcol, yr[p]);
        const int ox = (int)(m % g.Wo);
        const int64_t t = m / g.Wo;
        const int oy = (int)(t % g.Ho);
        const int n = (int)(t / g.Ho);
        int iy, ix;
        if (tap_src(g, oy, ox, ky, kx, iy, ix)) {
          const T* ptr = xs + ((((int64_t)n * g.Hi + iy) * g.Wi + ix) * xcs + xcc + vcol);
          if constexpr (VEC == 8) load8(ptr, xr[p]); else load4(ptr, xr[p]);
        } else {
#pragma unroll
          for (int i = 0; i < VEC; ++i) xr[p][i] = 0.f;
        }
      } else {
#pragma unroll
        for (int i = 0; i < VEC; ++i) { xr[p][i] = 0.f; yr[p][i] = 0.f; }
      }
    }
  };
  auto swz = [](int r) { return (((r >> 1) & 1) << 2) | (((r >> 3) & 1) << 3); };  // in 4-element chunks
  auto sstore = [&](int buf) {
#pragma unroll
    for (int p = 0; p < NP; ++p) {
      const int r = vrow + p * RPP;
      if constexpr (sizeof(T) == 2) {
        const int ch = (vcol >> 2) ^ swz(r);
        store8(tY[buf] + r * LDR + ch * 4, yr[p]);
        store8(tX[buf] + r * LDR + ch * 4, xr[p]);
      } else {
#pragma unroll
        for (int i = 0; i < VEC; ++i) {
          tY[buf][r * LDR + vcol + i] = yr[p][i];
          tX[buf][r * LDR + vcol + i] = xr[p][i];
        }
      }
    }
  };

  f32x4 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int nsteps = (int)((pend - pbeg + WG_BP - 1) / WG_BP);
  if (nsteps > 0) {
    gload(pbeg);
    sstore(0);
  }
  __syncthreads();
  const int lr = lane & 15, lg = lane >> 4;
  for (int s = 0; s < nsteps; ++s) {
    const int buf = s & 1;
    if (s + 1 < nsteps) gload(pbeg + (int64_t)(s + 1) * WG_BP);
    if constexpr (sizeof(T) == 2) {
      // fragment (rows 0..15 of a 16-wide column block c0): lane group lg needs pixel rows
      // 8lg..8lg+7; tr read: lane 4q+p addresses row (8lg + q [+4]), columns c0 + 4p.
      const int q = lr >> 2, pp = lr & 3;
      bf16x8 af[2], bfr[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int c0 = wr * 32 + i * 16;
#pragma unroll
        for (int half = 0; half < 2; ++half) {
          const int r = lg * 8 + half * 4 + q;
          const int ch = ((c0 >> 2) + pp) ^ swz(r);
          s16x4 v = __builtin_amdgcn_ds_read_tr16_b64_v4i16((LDS_PTR(s16x4))(tY[buf] + r * LDR + ch * 4));
#pragma unroll
          for (int e = 0; e < 4; ++e) af[i][half * 4 + e] = __builtin_bit_cast(bf16, (short)v[e]);
        }
      }
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int c0 = wc * 32 + j * 16;
#pragma unroll
        for (int half = 0; half < 2; ++half) {
          const int r = lg * 8 + half * 4 + q;
          const int ch = ((c0 >> 2) + pp) ^ swz(r);
          s16x4 v = __builtin_amdgcn_ds_read_tr16_b64_v4i16((LDS_PTR(s16x4))(tX[buf] + r * LDR + ch * 4));
#pragma unroll
          for (int e = 0; e < 4; ++e) bfr[j][half * 4 + e] = __builtin_bit_cast(bf16, (short)v[e]);
        }
      }
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[i], bfr[j], acc[i][j], 0, 0, 0);
    } else {
      // fp32 16x16x4: lane holds A[row lr][k = lg] and B[k = lg][col lr]; 8 k-steps of 4 pixels
#pragma unroll
      for (int kk = 0; kk < WG_BP / 4; ++kk) {
        const int r = kk * 4 + lg;
        float a0 = tY[buf][r * LDR + wr * 32 + lr];
        float a1 = tY[buf][r * LDR + wr * 32 + 16 + lr];
        float b0 = tX[buf][r * LDR + wc * 32 + lr];
        float b1 = tX[buf][r * LDR + wc * 32 + 16 + lr];
        acc[0][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b0, acc[0][0], 0, 0, 0);
        acc[0][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b1, acc[0][1], 0, 0, 0);
        acc[1][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b0, acc[1][0], 0, 0, 0);
        acc[1][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b1, acc[1][1], 0, 0, 0);
      }
    }
    if (s + 1 < nsteps) sstore(buf ^ 1);
    __syncthreads();
  }
  // D[row = co][col = kcol]: lane holds col lr, rows 4lg + r
  const int K = g.KH * g.KW * Cin;
  float* out = slab + (int64_t)blockIdx.z * g.Cout * K;
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int kc = kcol0 + wc * 32 + j * 16 + lr;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int co = co0 + wr * 32 + i * 16 + lg * 4 + r;
        out[(int64_t)co * K + kc] = acc[i][j][r];
      }
    }
}

// ----------------------------------------------------------------------------------------
// bf16 weight gradient with wide output tiles: BM output channels x 64 K-columns (one tap, 64 input
// channels) per block, pixels split over grid.z.  Same MFMA scheme as conv_wgrad_kernel (pixels are
// the MFMA K axis, both operands read with ds_read_b64_tr_b16), but
//   * BM = 128/256 rows amortise each input tile over 2-4x more output channels (fewer x re-reads);
//   * the input pixel coordinates are advanced incrementally (no 64-bit div/mod per load);
//   * wave w owns rows [w*BM/4, +BM/4) x all 64 columns.
// ----------------------------------------------------------------------------------------
template <int BM>
__device__ __forceinline__ int wgb_swz(int r) {  // XOR on 4-element chunk index of a BM-wide row
  if constexpr (BM == 64) return (((r >> 1) & 1) << 2) | (((r >> 3) & 1) << 3);
  else return 4 * ((r & 3) | (((r >> 3) & 1) << 2));
}

// bslab (nullable): the conv bias gradient sum_px dY[px][co] comes out of the same K loop — the blocks
// of the first K tile multiply their dY fragments by a ones operand (MT extra MFMAs per step, no extra
// memory traffic) and write per-split partials bslab[z][co] (replaces a separate column-sum pass
// over dY, which re-read the whole tensor).
// (BIAS: compile-time, so the plain instantiation keeps its register count — the bias accumulators
// pushed the BM = 256 kernel past 128 VGPRs, a wave per SIMD fewer and 43 % slower.)
// (Round 3 measured an XCD-grouped 1-D grid for a pixel split's tiles: whole step 130.4 -> 131.5 ms; removed.)
// wgrad_wide: register allocation for >= 2 waves per SIMD (256 registers).  With the unconstrained 512-register
// budget the compiler kept the accumulators in VGPRs and copied each one into a[0:3] before its MFMA and back after
// (AGPR-form MFMAs: 64 v_accvgpr_write + 64 v_accvgpr_read + s_nop per 16 MFMAs in the BM = 256 loop, 244 + 40
// registers); capped: VGPR-form MFMAs, no copies, 178 / 122 / 68 registers at BM = 256 / 128 / 64.
template <int BM, bool BIAS = false>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2))) void wgrad_wide_kernel(const bf16* __restrict__ x1, const bf16* __restrict__ x2,
                                                         const bf16* __restrict__ dy1, const bf16* __restrict__ dy2,
                                                         float* __restrict__ slab, float* __restrict__ bslab, ConvGeom g,
                                                         int M, int px_per_split) {
  constexpr int VPRY = BM / 8, RPPY = 256 / VPRY, NPY = WG_BP / RPPY;
  constexpr int MT = BM / 64;  // 16-row co tiles per wave
  __shared__ __attribute__((aligned(16))) bf16 tY[2][WG_BP * BM];
  __shared__ __attribute__((aligned(16))) bf16 tX[2][WG_BP * 64];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int lr = lane & 15, lg = lane >> 4;
  const int Cin = g.C1 + g.C2;
  const int bx = blockIdx.x, by = blockIdx.y, bz = blockIdx.z;
  const int co0 = bx * BM;
  const int kcol0 = by * 64;
  const int tap = kcol0 / Cin;
  const int ci0 = kcol0 - tap * Cin;
  const int ky = tap / g.KW, kx = tap - ky * g.KW;
  const int pbeg = bz * px_per_split;
  const int pend = min(M, pbeg + px_per_split);
  const bf16* xs; int xcs, xcc;
  if (ci0 < g.C1) { xs = x1; xcs = g.C1; xcc = ci0; } else { xs = x2; xcs = g.C2; xcc = ci0 - g.C1; }
  const bf16* ys; int ycs, ycc;
  const int Co2 = g.Cout - g.Co1;
  if (co0 < g.Co1) { ys = dy1; ycs = g.Co1; ycc = co0; } else { ys = dy2; ycs = Co2; ycc = co0 - g.Co1; }

  // x-tile role: one 8-channel vector of one pixel row per thread; its output coordinates advance by
  // WG_BP pixels per step
  const int xrow = tid >> 3, xcol = (tid & 7) * 8;
  int m = pbeg + xrow;
  int ox, oy, on;
  {
    const int hw = g.Ho * g.Wo;
    on = m / hw;
    const int rem = m - on * hw;
    oy = rem / g.Wo;
    ox = rem - oy * g.Wo;
  }
  const int yrow0 = tid / VPRY, ycol = (tid % VPRY) * 8;

  bf16x8 xr2[2], yr2[2][NPY];  // two steps in flight (register slot = step parity)
  auto gload = [&](int p0, auto slotc) {
    constexpr int slot = decltype(slotc)::value;
    bf16x8& xr = xr2[slot];
    bf16x8 (&yr)[NPY] = yr2[slot];
#pragma unroll
    for (int p = 0; p < NPY; ++p) {
      const int mm = p0 + yrow0 + p * RPPY;
      if (mm < pend) yr[p] = *reinterpret_cast<const bf16x8*>(ys + (int64_t)mm * ycs + ycc + ycol);
      else {
#pragma unroll
        for (int i = 0; i < 8; ++i) yr[p][i] = (bf16)0.f;
      }
    }
    int iy, ix;
    if (m < pend && tap_src(g, oy, ox, ky, kx, iy, ix))
      xr = *reinterpret_cast<const bf16x8*>(xs + (((int64_t)on * g.Hi + iy) * g.Wi + ix) * xcs + xcc + xcol);
    else {
#pragma unroll
      for (int i = 0; i < 8; ++i) xr[i] = (bf16)0.f;
    }
    // advance this thread's pixel by one step
    m += WG_BP;
    ox += WG_BP;
    while (ox >= g.Wo) {
      ox -= g.Wo;
      if (++oy >= g.Ho) { oy = 0; ++on; }
    }
  };
  auto sstore = [&](auto bufc) {
    constexpr int buf = decltype(bufc)::value;
    const bf16x8& xr = xr2[buf];
    const bf16x8 (&yr)[NPY] = yr2[buf];
#pragma unroll
    for (int p = 0; p < NPY; ++p) {
      const int r = yrow0 + p * RPPY;
      const int ch = (ycol >> 2) ^ wgb_swz<BM>(r);
      *reinterpret_cast<bf16x8*>(tY[buf] + r * BM + ch * 4) = yr[p];
    }
    const int ch = (xcol >> 2) ^ wgb_swz<64>(xrow);
    *reinterpret_cast<bf16x8*>(tX[buf] + xrow * 64 + ch * 4) = xr;
  };

  f32x4 acc[MT][4];
#pragma unroll
  for (int i = 0; i < MT; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  const bool bias_blk = BIAS && by == 0;  // uniform
  f32x4 bacc[BIAS ? MT : 1];
#pragma unroll
  for (int i = 0; i < (BIAS ? MT : 1); ++i) bacc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
  bf16x8 ones;
#pragma unroll
  for (int e = 0; e < 8; ++e) ones[e] = (bf16)1.f;
  const int nsteps = (pend - pbeg + WG_BP - 1) / WG_BP;
  using I0 = std::integral_constant<int, 0>;
  using I1 = std::integral_constant<int, 1>;
  if (nsteps > 0) {
    gload(pbeg, I0{});
    if (nsteps > 1) gload(pbeg + WG_BP, I1{});
    sstore(I0{});
  }
  __syncthreads();
  const int q = lr >> 2, pp = lr & 3;
  // steps in pairs: LDS buffer and register slot are compile-time; step s+2 is loaded while step s runs
  auto step = [&](int s, auto bufc) {
    constexpr int buf = decltype(bufc)::value;
    if (s + 2 < nsteps) gload(pbeg + (s + 2) * WG_BP, bufc);
    bf16x8 af[MT], bfr[4];
#pragma unroll
    for (int i = 0; i < MT; ++i) {
      const int c0 = wid * (BM / 4) + i * 16;
#pragma unroll
      for (int half = 0; half < 2; ++half) {
        const int r = lg * 8 + half * 4 + q;
        const int ch = ((c0 >> 2) + pp) ^ wgb_swz<BM>(r);
        const s16x4 v = __builtin_amdgcn_ds_read_tr16_b64_v4i16((LDS_PTR(s16x4))(tY[buf] + r * BM + ch * 4));
#pragma unroll
        for (int e = 0; e < 4; ++e) af[i][half * 4 + e] = __builtin_bit_cast(bf16, (short)v[e]);
      }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
#pragma unroll
      for (int half = 0; half < 2; ++half) {
        const int r = lg * 8 + half * 4 + q;
        const int ch = ((j * 16 >> 2) + pp) ^ wgb_swz<64>(r);
        const s16x4 v = __builtin_amdgcn_ds_read_tr16_b64_v4i16((LDS_PTR(s16x4))(tX[buf] + r * 64 + ch * 4));
#pragma unroll
        for (int e = 0; e < 4; ++e) bfr[j][half * 4 + e] = __builtin_bit_cast(bf16, (short)v[e]);
      }
    }
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[i], bfr[j], acc[i][j], 0, 0, 0);
    if constexpr (BIAS) {
      if (bias_blk) {
#pragma unroll
        for (int i = 0; i < MT; ++i) bacc[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[i], ones, bacc[i], 0, 0, 0);
      }
    }
    if (s + 1 < nsteps) sstore(std::integral_constant<int, buf ^ 1>{});
    __syncthreads();
  };
  for (int s = 0; s < nsteps; s += 2) {
    step(s, I0{});
    if (s + 1 < nsteps) step(s + 1, I1{});
  }
  if (BIAS && bias_blk && lr == 0) {  // every output column holds the row sum: column 0 writes it
#pragma unroll
    for (int i = 0; i < (BIAS ? MT : 1); ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r) bslab[(int64_t)bz * g.Cout + co0 + wid * (BM / 4) + i * 16 + lg * 4 + r] = bacc[i][r];
  }
  const int K = g.KH * g.KW * Cin;
  float* out = slab + (int64_t)bz * g.Cout * K;
#pragma unroll
  for (int i = 0; i < MT; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int kc = kcol0 + j * 16 + lr;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int co = co0 + wid * (BM / 4) + i * 16 + lg * 4 + r;
        out[(int64_t)co * K + kc] = acc[i][j][r];
      }
    }
}

// ----------------------------------------------------------------------------------------
// 1x1 weight gradient with square tiles (round 6): BM = 256 (or 64) output rows x BN = 256 (or 128) input channels per
// block, 8 waves (BM/64 row quarters x 8/(BM/64) column slices, 64 rows per wave).  wgrad_wide<256> reads the same 256-row dY slice
// once per 64 input channels: at the 768-channel qkv projections of the C = 256 / 512 levels that is 4-8 reads of the
// largest tensor, and the kernel is bound by those bytes (≈ 2 TB/s of loads at 0.15 of the MFMA peak).  Here dY is read
// once per (row tile, pixel split) and x once per row tile.  Loads through registers as wgrad_wide (two steps in
// flight), fragments by ds_read_b64_tr_b16 from the same XOR-swizzled rows.
// ----------------------------------------------------------------------------------------
template <int BM, int BN, bool BIAS = false>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(2))) void wgrad_sq_kernel(
    const bf16* __restrict__ x, const bf16* __restrict__ dy, float* __restrict__ slab, float* __restrict__ bslab, int M,
    int Cout, int Cin, int px_per_split) {
  // waves: WR row quarters of 64 rows x WC column slices of BN / WC columns
  constexpr int WR = BM / 64, WC = 8 / WR, MT = 4, NT = BN / (16 * WC);
  static_assert((BM == 256 || BM == 64) && NT >= 1, "wgrad_sq tiles");
  constexpr int TY = WG_BP * BM / 8, TX = WG_BP * BN / 8;  // 16-B vectors per step
  constexpr int NY = (TY + 511) / 512, NX = (TX + 511) / 512;
  __shared__ __attribute__((aligned(16))) bf16 tY[2][WG_BP * BM];
  __shared__ __attribute__((aligned(16))) bf16 tX[2][WG_BP * BN];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int lr = lane & 15, lg = lane >> 4;
  const int wr = wid % WR, wc = wid / WR;
  const int co0 = blockIdx.x * BM, k0 = blockIdx.y * BN;
  const int pbeg = blockIdx.z * px_per_split;
  const int pend = min(M, pbeg + px_per_split);
  bf16x8 yr2[2][NY], xr2[2][NX];
  auto gload = [&](int p0, auto slotc) {
    constexpr int slot = decltype(slotc)::value;
#pragma unroll
    for (int u = 0; u < NY; ++u) {
      const int v = tid + 512 * u, r = v / (BM / 8), c = (v % (BM / 8)) * 8;
      const int m = p0 + r;
      yr2[slot][u] = m < pend && v < TY ? *reinterpret_cast<const bf16x8*>(dy + (int64_t)m * Cout + co0 + c) : bf16x8{};
    }
#pragma unroll
    for (int u = 0; u < NX; ++u) {
      const int v = tid + 512 * u, r = v / (BN / 8), c = (v % (BN / 8)) * 8;
      const int m = p0 + r;
      xr2[slot][u] = m < pend && v < TX ? *reinterpret_cast<const bf16x8*>(x + (int64_t)m * Cin + k0 + c) : bf16x8{};
    }
  };
  auto sstore = [&](auto bufc) {
    constexpr int buf = decltype(bufc)::value;
#pragma unroll
    for (int u = 0; u < NY; ++u) {
      const int v = tid + 512 * u, r = v / (BM / 8), c = (v % (BM / 8)) * 8;
      if (v < TY) *reinterpret_cast<bf16x8*>(tY[buf] + r * BM + (((c >> 2) ^ wgb_swz<BM>(r)) * 4)) = yr2[buf][u];
    }
#pragma unroll
    for (int u = 0; u < NX; ++u) {
      const int v = tid + 512 * u, r = v / (BN / 8), c = (v % (BN / 8)) * 8;
      if (v < TX) *reinterpret_cast<bf16x8*>(tX[buf] + r * BN + (((c >> 2) ^ wgb_swz<BN>(r)) * 4)) = xr2[buf][u];
    }
  };
  f32x4 acc[MT][NT];
#pragma unroll
  for (int i = 0; i < MT; ++i)
#pragma unroll
    for (int j = 0; j < NT; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  // BIAS: the conv bias gradient sum_px dY[px][co] from the same dY fragments times a ones operand, by the waves of the
  // first column slice of the first column block (as wgrad_wide<BM, true>); per-split partials bslab[z][co]
  const bool bias_w = BIAS && blockIdx.y == 0 && wc == 0;  // wave-uniform
  f32x4 bacc[BIAS ? MT : 1];
#pragma unroll
  for (int i = 0; i < (BIAS ? MT : 1); ++i) bacc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
  bf16x8 ones;
#pragma unroll
  for (int e = 0; e < 8; ++e) ones[e] = (bf16)1.f;
  const int nsteps = (pend - pbeg + WG_BP - 1) / WG_BP;
  using I0 = std::integral_constant<int, 0>;
  using I1 = std::integral_constant<int, 1>;
  if (nsteps > 0) {
    gload(pbeg, I0{});
    if (nsteps > 1) gload(pbeg + WG_BP, I1{});
    sstore(I0{});
  }
  __syncthreads();
  const int q = lr >> 2, pp = lr & 3;
  auto step = [&](int s, auto bufc) {
    constexpr int buf = decltype(bufc)::value;
    if (s + 2 < nsteps) gload(pbeg + (s + 2) * WG_BP, bufc);
    bf16x8 af[MT], bfr[NT];
#pragma unroll
    for (int i = 0; i < MT; ++i) {
      const int c0 = wr * 64 + i * 16;
#pragma unroll
      for (int half = 0; half < 2; ++half) {
        const int r = lg * 8 + half * 4 + q;
        const int ch = ((c0 >> 2) + pp) ^ wgb_swz<BM>(r);
        const s16x4 v = __builtin_amdgcn_ds_read_tr16_b64_v4i16((LDS_PTR(s16x4))(tY[buf] + r * BM + ch * 4));
#pragma unroll
        for (int e = 0; e < 4; ++e) af[i][half * 4 + e] = __builtin_bit_cast(bf16, (short)v[e]);
      }
    }
#pragma unroll
    for (int j = 0; j < NT; ++j) {
      const int c0 = wc * (BN / WC) + j * 16;
#pragma unroll
      for (int half = 0; half < 2; ++half) {
        const int r = lg * 8 + half * 4 + q;
        const int ch = ((c0 >> 2) + pp) ^ wgb_swz<BN>(r);
        const s16x4 v = __builtin_amdgcn_ds_read_tr16_b64_v4i16((LDS_PTR(s16x4))(tX[buf] + r * BN + ch * 4));
#pragma unroll
        for (int e = 0; e < 4; ++e) bfr[j][half * 4 + e] = __builtin_bit_cast(bf16, (short)v[e]);
      }
    }
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
      for (int j = 0; j < NT; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[i], bfr[j], acc[i][j], 0, 0, 0);
    if constexpr (BIAS) {
      if (bias_w) {
#pragma unroll
        for (int i = 0; i < MT; ++i) bacc[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[i], ones, bacc[i], 0, 0, 0);
      }
    }
    if (s + 1 < nsteps) sstore(std::integral_constant<int, buf ^ 1>{});
    __syncthreads();
  };
  for (int s = 0; s < nsteps; s += 2) {
    step(s, I0{});
    if (s + 1 < nsteps) step(s + 1, I1{});
  }
  if (BIAS && bias_w && lr == 0) {  // every output column holds the row sum: column 0 writes it
#pragma unroll
    for (int i = 0; i < (BIAS ? MT : 1); ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r) bslab[(int64_t)blockIdx.z * Cout + co0 + wr * 64 + i * 16 + lg * 4 + r] = bacc[i][r];
  }
  float* out = slab + (int64_t)blockIdx.z * Cout * Cin;
#pragma unroll
  for (int i = 0; i < MT; ++i)
#pragma unroll
    for (int j = 0; j < NT; ++j) {
      const int kc = k0 + wc * (BN / WC) + j * 16 + lr;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int co = co0 + wr * 64 + i * 16 + lg * 4 + r;
        out[(int64_t)co * Cin + kc] = acc[i][j][r];
      }
    }
}

// ----------------------------------------------------------------------------------------
// 3x3 / stride 1 / pad 1 weight gradient (bf16), halo-tiled.  Block = (64 co) x (32 ci chunk) x
// all 9 taps, looping over 8x32-pixel tiles (its share of the split-K over pixels).  Per tile the
// dY tile [256 px][64 co] and the input halo [10x34 px][32 ci] are staged in LDS; pixels are the
// MFMA K axis, so both operands are read transposed with ds_read_b64_tr_b16 from XOR-swizzled
// rows (conflict-free).  Wave w: co tiles {2*(w>>1), 2*(w>>1)+1} x ci tile (w&1) x 9 taps.
// ----------------------------------------------------------------------------------------
constexpr int W3_TH = 8, W3_TW = 32;
constexpr int W3_HW = W3_TW + 2, W3_NPIX = (W3_TH + 2) * (W3_TW + 2);
// LDS pitch (pixels) of the input-halo rows of both 3x3 weight-gradient kernels: a multiple of 16, so
// a step of whole halo rows keeps bit 3 of the LDS row and with it the chunk swizzle (w3_swz_x) —
// the transposed fragment reads of all nine taps then share six per-lane offsets plus immediates
// instead of recomputing a swizzled address per read (the kernels were VALU-issue bound: 6-10 VALU
// per MFMA, mostly that address arithmetic).
constexpr int W3_P = 48;

__device__ __forceinline__ int w3_swz_dy(int r) { return (((r >> 1) & 1) << 2) | (((r >> 3) & 1) << 3); }
__device__ __forceinline__ int w3_swz_x(int r) { return ((r >> 3) & 1) << 2; }

// Same weight gradient with blocks of 64 co x 64 ci and 8 waves (one block per CU, two waves per SIMD; wave w:
// co tiles {2*(w>>2), 2*(w>>2)+1} x ci tile w&3).  The wgrad is bound by the per-CU load rate (~7.6 B/cycle
// with plain 16-B loads: 54 KB per 8 x 32 tile of a 64 x 32 block, the dY tile re-read by every ci block):
// 64 ci per block loads each dY tile once per 64 input channels (75 KB per tile for twice the MACs).  The
// input halo is kept as two 32-channel planes so the fragment reads are the 64-ci kernel's.
constexpr int W3_PLANE = (W3_TH + 2) * W3_P * 32;  // halo plane (bf16 elements)

// (Round 3 measured a 4-wave form -- one wave per SIMD, 144 accumulators, all four co tiles per wave -- as neutral,
// 63.69 vs 63.58 ms conv total per step: fewer LDS reads per MFMA, less latency hiding.  Removed.)
// 3x3 wgrad kernels: L2 touch of the tile after next (wgrad3x3c64 415 -> 389 us per launch in the step,
// profiles/r4c7b_bench_ab.txt)
constexpr int WG_NT = 512;  // threads per block
constexpr int WG_NI = 2;    // co tiles per wave
__global__ __launch_bounds__(WG_NT, 1) void wgrad3x3c64_kernel(const bf16* __restrict__ x1, const bf16* __restrict__ x2,
                                                             const bf16* __restrict__ dy1, const bf16* __restrict__ dy2,
                                                             float* __restrict__ slab, ConvGeom g, int tiles_x,
                                                             int ntiles) {
  __shared__ __attribute__((aligned(16))) bf16 sdy[W3_TH * W3_TW * 64];  // 32 KB, 128-B rows
  __shared__ __attribute__((aligned(16))) bf16 shx[2 * W3_PLANE];        // 2 x 30 KB, 64-B rows
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int cot0 = (wid >> 2) * 2, cit = wid & 3;
  const int co0 = blockIdx.x * 64, ci0 = blockIdx.y * 64;
  const int Cin = g.C1 + g.C2;
  const bf16* xs; int xcs, xcc;
  if (ci0 < g.C1) { xs = x1; xcs = g.C1; xcc = ci0; } else { xs = x2; xcs = g.C2; xcc = ci0 - g.C1; }
  const bf16* ys; int ycs, ycc;
  const int Co2 = g.Cout - g.Co1;
  if (co0 < g.Co1) { ys = dy1; ycs = g.Co1; ycc = co0; } else { ys = dy2; ycs = Co2; ycc = co0 - g.Co1; }
  const int tiles_per_img = tiles_x * ((g.Ho + W3_TH - 1) / W3_TH);

  f32x4 acc[WG_NI][9];
#pragma unroll
  for (int i = 0; i < WG_NI; ++i)
#pragma unroll
    for (int t = 0; t < 9; ++t) acc[i][t] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int lr = lane & 15, lg = lane >> 4, q = lr >> 2, pp = lr & 3;
  const bf16* shp = shx + (cit >> 1) * W3_PLANE;
  int aoff[WG_NI][2], boff[2][3];
#pragma unroll
  for (int half = 0; half < 2; ++half) {
    const int r = lg * 8 + half * 4 + q;
#pragma unroll
    for (int i = 0; i < WG_NI; ++i) aoff[i][half] = r * 64 + ((((cot0 + i) * 4 + pp) ^ w3_swz_dy(r)) * 4);
#pragma unroll
    for (int kx = 0; kx < 3; ++kx) boff[half][kx] = (r + kx) * 32 + ((((cit & 1) * 4 + pp) ^ w3_swz_x(r + kx)) * 4);
  }
  // next tile's vectors in registers (unpredicated loads: clamped address + select), written to LDS after
  // the barrier that ends the current tile's reads
  constexpr int YV = 2048 / WG_NT, HV = (W3_NPIX * 8 + WG_NT - 1) / WG_NT;
  bf16x8 yv[YV], hv[HV];
  auto gload = [&](int tile) {
    const int n = tile / tiles_per_img;
    const int rem = tile - n * tiles_per_img;
    const int ty = rem / tiles_x, tx = rem - ty * tiles_x;
    const int y0 = ty * W3_TH, x0 = tx * W3_TW;
#pragma unroll
    for (int k = 0; k < YV; ++k) {      // dY: 256 px x 8 vectors
      const int e = tid + k * WG_NT;
      const int p = e >> 3, part = e & 7;
      const int oy = y0 + (p >> 5), ox = x0 + (p & 31);
      const bool ok = oy < g.Ho && ox < g.Wo;
      const bf16x8 v = *reinterpret_cast<const bf16x8*>(
          ys + (ok ? (((int64_t)n * g.Ho + oy) * g.Wo + ox) * ycs : 0) + ycc + part * 8);
      yv[k] = ok ? v : bf16x8{};
    }
#pragma unroll
    for (int k = 0; k < HV; ++k) {      // halo: 340 px x 8 vectors (64 ci)
      const int e = tid + k * WG_NT;
      const int hp = e >> 3, part = e & 7;
      const int r = hp / W3_HW, c = hp - r * W3_HW;
      const int iy = y0 - 1 + r, ix = x0 - 1 + c;
      const bool ok = e < W3_NPIX * 8 && (unsigned)iy < (unsigned)g.Hi && (unsigned)ix < (unsigned)g.Wi;
      const bf16x8 v = *reinterpret_cast<const bf16x8*>(
          xs + (ok ? (((int64_t)n * g.Hi + iy) * g.Wi + ix) * xcs : 0) + xcc + part * 8);
      hv[k] = ok ? v : bf16x8{};
    }
  };
  // L2 touch: the dY and input-halo lines of the tile after next, LDS-direct into a never-read row per wave
  // (4 B per 128-B pixel line), so the register prefetch of that tile a step later finds them in L2
  __shared__ __attribute__((aligned(16))) int tdump[WG_NT];
  auto touch = [&](int tile) {
    const int n = tile / tiles_per_img;
    const int rem = tile - n * tiles_per_img;
    const int ty = rem / tiles_x, tx = rem - ty * tiles_x;
    const int y0 = ty * W3_TH, x0 = tx * W3_TW;
    const int64_t yimg = (int64_t)g.Ho * g.Wo * ycs, ximg = (int64_t)g.Hi * g.Wi * xcs;
    const __amdgpu_buffer_rsrc_t yrs =
        __builtin_amdgcn_make_buffer_rsrc((void*)(ys + n * yimg + ycc), (short)0, (int)(yimg * 2 - ycc * 2), 0x00020000);
    const __amdgpu_buffer_rsrc_t xrs =
        __builtin_amdgcn_make_buffer_rsrc((void*)(xs + n * ximg + xcc), (short)0, (int)(ximg * 2 - xcc * 2), 0x00020000);
    auto* dst = (__attribute__((address_space(3))) void*)(tdump + wid * 64);
    {  // dY: 256 pixels
      const int p = tid & 255;
      const int oy = y0 + (p >> 5), ox = x0 + (p & 31);
      const bool ok = tid < 256 && oy < g.Ho && ox < g.Wo;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(yrs, dst, 4, ok ? (oy * g.Wo + ox) * ycs * 2 : 0x7ffffff0, 0, 0, 0);
    }
    {  // halo: 340 pixels (threads 256..511 and 0..83)
      const int hp = tid < 256 ? 256 + tid : tid - 256;
      const int r = hp / W3_HW, c = hp - r * W3_HW;
      const int iy = y0 - 1 + r, ix = x0 - 1 + c;
      const bool ok = hp < W3_NPIX && (unsigned)iy < (unsigned)g.Hi && (unsigned)ix < (unsigned)g.Wi;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(xrs, dst, 4, ok ? (iy * g.Wi + ix) * xcs * 2 : 0x7ffffff0, 0, 0, 0);
    }
  };
  if ((int)blockIdx.z < ntiles) gload(blockIdx.z);
  for (int tile = blockIdx.z; tile < ntiles; tile += gridDim.z) {
    __syncthreads();
#pragma unroll
    for (int k = 0; k < YV; ++k) {
      const int e = tid + k * WG_NT;
      const int p = e >> 3, part = e & 7;  // chunk pair (2part, 2part+1) of 8-B chunks
      const int ch = (part * 2) ^ w3_swz_dy(p);
      *reinterpret_cast<bf16x8*>(sdy + p * 64 + ch * 4) = yv[k];
    }
#pragma unroll
    for (int k = 0; k < HV; ++k) {
      const int e = tid + k * WG_NT;
      if (e < W3_NPIX * 8) {
        const int hp = e >> 3, part = e & 7;
        const int r = hp / W3_HW, row = r * W3_P + (hp - r * W3_HW);
        const int ch = ((part & 3) * 2) ^ w3_swz_x(row);
        *reinterpret_cast<bf16x8*>(shx + (part >> 2) * W3_PLANE + row * 32 + ch * 4) = hv[k];
      }
    }
    __syncthreads();
    if (tile + (int)gridDim.z < ntiles) gload(tile + gridDim.z);
    if (tile + 2 * (int)gridDim.z < ntiles) touch(tile + 2 * gridDim.z);
    // the fragment reads of pixel row py+1 (2 NI + 18) are issued between the 9 NI MFMAs of row py (two register
    // sets; 1 read : 1 MFMA via sched_group_barrier), so no row waits for its LDS reads
    bf16x8 fa[2][WG_NI], fb[2][9];
    auto rd = [&](int py, int b) {
#pragma unroll
      for (int i = 0; i < WG_NI; ++i)
#pragma unroll
        for (int half = 0; half < 2; ++half) {
          const s16x4 v = __builtin_amdgcn_ds_read_tr16_b64_v4i16((LDS_PTR(s16x4))(sdy + aoff[i][half] + py * 32 * 64));
#pragma unroll
          for (int e = 0; e < 4; ++e) fa[b][i][half * 4 + e] = __builtin_bit_cast(bf16, (short)v[e]);
        }
#pragma unroll
      for (int tap = 0; tap < 9; ++tap) {
        const int ky = tap / 3, kx = tap - ky * 3;
#pragma unroll
        for (int half = 0; half < 2; ++half) {
          const s16x4 v = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
              (LDS_PTR(s16x4))(shp + boff[half][kx] + (py + ky) * W3_P * 32));
#pragma unroll
          for (int e = 0; e < 4; ++e) fb[b][tap][half * 4 + e] = __builtin_bit_cast(bf16, (short)v[e]);
        }
      }
    };
    auto mm = [&](int b) {
#pragma unroll
      for (int tap = 0; tap < 9; ++tap)
#pragma unroll
        for (int i = 0; i < WG_NI; ++i)
          acc[i][tap] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[b][i], fb[b][tap], acc[i][tap], 0, 0, 0);
    };
    rd(0, 0);
#pragma unroll
    for (int py = 0; py < W3_TH; ++py) {
      const int b = py & 1;
      __builtin_amdgcn_sched_barrier(0);
      if (py + 1 < W3_TH) rd(py + 1, b ^ 1);
      mm(b);
      if (py + 1 < W3_TH) {
        constexpr int NRD = 2 * WG_NI + 18, NMF = 9 * WG_NI;
        constexpr int NPAIR = NRD < NMF ? NRD : NMF;
#pragma unroll
        for (int q2 = 0; q2 < NPAIR; ++q2) {
          __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);  // 1 DS read
          __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);  // 1 MFMA
        }
        if (NRD > NPAIR) __builtin_amdgcn_sched_group_barrier(0x100, NRD - NPAIR, 0);
        if (NMF > NPAIR) __builtin_amdgcn_sched_group_barrier(0x008, NMF - NPAIR, 0);
      }
      __builtin_amdgcn_sched_barrier(0);
    }
  }
  const int K = 9 * Cin;
  float* out = slab + (int64_t)blockIdx.z * g.Cout * K;
#pragma unroll
  for (int i = 0; i < WG_NI; ++i)
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
      const int ci = ci0 + cit * 16 + lr;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int co = co0 + (cot0 + i) * 16 + lg * 4 + r;
        out[(int64_t)co * K + tap * Cin + ci] = acc[i][tap][r];
      }
    }
}

// Weight gradient of the 4x4 / stride-2 / pad-1 conv (Downsample; the Upsample's weight gradient is the same
// operation with dOut as the input and x as dY), halo-tiled like wgrad3x3c64_kernel on the low-resolution
// dY grid.  Block = (64 co) x (32 ci chunk) x one input parity (a, b) = its 4 live taps ky = (1-a) + 2t,
// kx = (1-b) + 2u, whose inputs are the (TH+2) x (TW+2) halo of x_ab[Y][X] = x[2Y+a][2X+b] at offsets
// (1-a+t, 1-b+u) - the forward's parity split (convs2_bf16_kernel).  Replaces the wide-tile wgrad, which
// gathered every (pixel, tap) pair (315 TF/s on the bench shapes).
template <int BY, int BX>
__device__ __forceinline__ void ws2_taps(const bf16* sdy, const bf16* shx, const int (&aoff)[2][2],
                                         const int (&boff)[2][3], f32x4 (&acc)[2][4]) {
#pragma unroll 1
  for (int py = 0; py < W3_TH; ++py) {
    bf16x8 af[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
#pragma unroll
      for (int half = 0; half < 2; ++half) {
        const s16x4 v = __builtin_amdgcn_ds_read_tr16_b64_v4i16((LDS_PTR(s16x4))(sdy + aoff[i][half] + py * 32 * 64));
#pragma unroll
        for (int e = 0; e < 4; ++e) af[i][half * 4 + e] = __builtin_bit_cast(bf16, (short)v[e]);
      }
    }
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int oy = BY + (t >> 1), ox = BX + (t & 1);
      bf16x8 bfr;
#pragma unroll
      for (int half = 0; half < 2; ++half) {
        const s16x4 v =
            __builtin_amdgcn_ds_read_tr16_b64_v4i16((LDS_PTR(s16x4))(shx + boff[half][ox] + (py + oy) * W3_P * 32));
#pragma unroll
        for (int e = 0; e < 4; ++e) bfr[half * 4 + e] = __builtin_bit_cast(bf16, (short)v[e]);
      }
      acc[0][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[0], bfr, acc[0][t], 0, 0, 0);
      acc[1][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[1], bfr, acc[1][t], 0, 0, 0);
    }
  }
}

__global__ __launch_bounds__(256, 2) void wgrads2_bf16_kernel(const bf16* __restrict__ x, const bf16* __restrict__ dy,
                                                              float* __restrict__ slab, ConvGeom g, int tiles_x,
                                                              int ntiles) {
  __shared__ __attribute__((aligned(16))) bf16 sdy[W3_TH * W3_TW * 64];        // 32 KB, 128-B rows
  __shared__ __attribute__((aligned(16))) bf16 shx[(W3_TH + 2) * W3_P * 32];  // 30 KB, 64-B rows
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int cot0 = (wid >> 1) * 2, cit = wid & 1;
  const int co0 = blockIdx.x * 64;
  const int ab = (int)blockIdx.y & 3, a = ab >> 1, b = ab & 1;
  const int ci0 = ((int)blockIdx.y >> 2) * 32;
  const int Cin = g.C1;
  const int tiles_per_img = tiles_x * ((g.Ho + W3_TH - 1) / W3_TH);

  f32x4 acc[2][4];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[i][t] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int lr = lane & 15, lg = lane >> 4, q = lr >> 2, pp = lr & 3;
  int aoff[2][2], boff[2][3];
#pragma unroll
  for (int half = 0; half < 2; ++half) {
    const int r = lg * 8 + half * 4 + q;
#pragma unroll
    for (int i = 0; i < 2; ++i) aoff[i][half] = r * 64 + ((((cot0 + i) * 4 + pp) ^ w3_swz_dy(r)) * 4);
#pragma unroll
    for (int kx = 0; kx < 3; ++kx) boff[half][kx] = (r + kx) * 32 + (((cit * 4 + pp) ^ w3_swz_x(r + kx)) * 4);
  }
  for (int tile = blockIdx.z; tile < ntiles; tile += gridDim.z) {
    const int n = tile / tiles_per_img;
    const int rem = tile - n * tiles_per_img;
    const int ty = rem / tiles_x, tx = rem - ty * tiles_x;
    const int y0 = ty * W3_TH, x0 = tx * W3_TW;
    __syncthreads();
    {
      bf16x8 yv[8], hv[6];
#pragma unroll
      for (int k = 0; k < 8; ++k) {  // dY: 256 px x 8 vectors
        const int e = tid + k * 256;
        const int p = e >> 3, part = e & 7;
        const int oy = y0 + (p >> 5), ox = x0 + (p & 31);
        bf16x8 v = {};
        if (oy < g.Ho && ox < g.Wo)
          v = *reinterpret_cast<const bf16x8*>(dy + (((int64_t)n * g.Ho + oy) * g.Wo + ox) * g.Cout + co0 + part * 8);
        yv[k] = v;
      }
#pragma unroll
      for (int k = 0; k < 6; ++k) {  // halo of x_ab: 340 px x 4 vectors
        const int e = tid + k * 256;
        bf16x8 v = {};
        if (e < W3_NPIX * 4) {
          const int hp = e >> 2, part = e & 3;
          const int r = hp / W3_HW, c = hp - r * W3_HW;
          const int iy = 2 * (y0 - 1 + r) + a, ix = 2 * (x0 - 1 + c) + b;
          if ((unsigned)iy < (unsigned)g.Hi && (unsigned)ix < (unsigned)g.Wi)
            v = *reinterpret_cast<const bf16x8*>(x + (((int64_t)n * g.Hi + iy) * g.Wi + ix) * Cin + ci0 + part * 8);
        }
        hv[k] = v;
      }
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const int e = tid + k * 256;
        const int p = e >> 3, part = e & 7;
        const int ch = (part * 2) ^ w3_swz_dy(p);
        *reinterpret_cast<bf16x8*>(sdy + p * 64 + ch * 4) = yv[k];
      }
#pragma unroll
      for (int k = 0; k < 6; ++k) {
        const int e = tid + k * 256;
        if (e < W3_NPIX * 4) {
          const int hp = e >> 2, part = e & 3;
          const int r = hp / W3_HW, row = r * W3_P + (hp - r * W3_HW);
          const int ch = (part * 2) ^ w3_swz_x(row);
          *reinterpret_cast<bf16x8*>(shx + row * 32 + ch * 4) = hv[k];
        }
      }
    }
    __syncthreads();
    switch (ab) {  // block-uniform: tap bases 1-a, 1-b
      case 0: ws2_taps<1, 1>(sdy, shx, aoff, boff, acc); break;
      case 1: ws2_taps<1, 0>(sdy, shx, aoff, boff, acc); break;
      case 2: ws2_taps<0, 1>(sdy, shx, aoff, boff, acc); break;
      default: ws2_taps<0, 0>(sdy, shx, aoff, boff, acc); break;
    }
  }
  // D[co][ci] per tap: lane col lr -> ci, rows 4lg+r -> co; tap = ky*4 + kx
  const int K = 16 * Cin;
  float* out = slab + (int64_t)blockIdx.z * g.Cout * K;
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int tap = (1 - a + 2 * (t >> 1)) * 4 + (1 - b + 2 * (t & 1));
      const int ci = ci0 + cit * 16 + lr;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int co = co0 + (cot0 + i) * 16 + lg * 4 + r;
        out[(int64_t)co * K + tap * Cin + ci] = acc[i][t][r];
      }
    }
}

// Same weight gradient on 8 x 36 pixel tiles (288 px = 9 K-chunks of 32 flat pixels): every U-Net
// level's width (288/144/72/36) is a multiple of 36, so no tile column is wasted (the 8 x 32 tiles
// above compute 36-px rows as two 32-px tiles: 56 % useful at 24 x 36).  A K-chunk may span two
// image rows: each lane derives its own halo row per chunk (the transposed ds_read takes per-lane
// addresses).
constexpr int W36_TH = 8, W36_TW = 36, W36_HW = W36_TW + 2, W36_NPIX = (W36_TH + 2) * W36_HW;  // 380 halo px
constexpr int W36_NP = W36_TH * W36_TW;                                                          // 288 px

// sum slabs over splits (fixed order) and scatter into the PyTorch weight layout
// dst[((d0*D1 + d1)*KH + kyt)*KW + kxt], with (d0,d1) = swap ? (ci,co) : (co,ci) and
// (kyt,kxt) = flip ? (KH-1-ky, KW-1-kx) : (ky,kx).
// 8 x 36 tiles (levels 2-3) with the 64 co x 64 ci / 8-wave blocking and the K-chunk software pipeline of
// wgrad3x3c64_kernel: each wave's 22 fragment reads of K-chunk kc+1 are issued between the 18 MFMAs of chunk kc
__global__ __launch_bounds__(WG_NT, 1) void wgrad3x3w36c64_kernel(const bf16* __restrict__ x1, const bf16* __restrict__ x2,
                                                                const bf16* __restrict__ dy1, const bf16* __restrict__ dy2,
                                                                float* __restrict__ slab, ConvGeom g, int tiles_x,
                                                                int ntiles) {
  __shared__ __attribute__((aligned(16))) bf16 sdy[W36_NP * 64];  // 36 KB, 128-B rows
  __shared__ __attribute__((aligned(16))) bf16 shx[2 * W3_PLANE];  // 2 x 30 KB, 64-B rows
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int cot0 = (wid >> 2) * 2, cit = wid & 3;
  const int co0 = blockIdx.x * 64, ci0 = blockIdx.y * 64;
  const int Cin = g.C1 + g.C2;
  const bf16* xs; int xcs, xcc;
  if (ci0 < g.C1) { xs = x1; xcs = g.C1; xcc = ci0; } else { xs = x2; xcs = g.C2; xcc = ci0 - g.C1; }
  const bf16* ys; int ycs, ycc;
  const int Co2 = g.Cout - g.Co1;
  if (co0 < g.Co1) { ys = dy1; ycs = g.Co1; ycc = co0; } else { ys = dy2; ycs = Co2; ycc = co0 - g.Co1; }
  const int tiles_per_img = tiles_x * ((g.Ho + W36_TH - 1) / W36_TH);

  f32x4 acc[WG_NI][9];
#pragma unroll
  for (int i = 0; i < WG_NI; ++i)
#pragma unroll
    for (int t = 0; t < 9; ++t) acc[i][t] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int lr = lane & 15, lg = lane >> 4, q = lr >> 2, pp = lr & 3;
  const bf16* shp = shx + (cit >> 1) * W3_PLANE;
  const int cx = (cit & 1) * 4 + pp;
  int aoff[WG_NI][2];
#pragma unroll
  for (int half = 0; half < 2; ++half) {
    const int r = lg * 8 + half * 4 + q;
#pragma unroll
    for (int i = 0; i < WG_NI; ++i) aoff[i][half] = r * 64 + ((((cot0 + i) * 4 + pp) ^ w3_swz_dy(r)) * 4);
  }
  constexpr int YV = (W36_NP * 8 + WG_NT - 1) / WG_NT, HV = (W36_NPIX * 8 + WG_NT - 1) / WG_NT;
  bf16x8 yv[YV], hv[HV];
  auto gload = [&](int tile) {
    const int n = tile / tiles_per_img;
    const int rem = tile - n * tiles_per_img;
    const int ty = rem / tiles_x, tx = rem - ty * tiles_x;
    const int y0 = ty * W36_TH, x0 = tx * W36_TW;
#pragma unroll
    for (int k = 0; k < YV; ++k) {       // dY: 288 px x 8 vectors
      const int e = tid + k * WG_NT;
      const int p = e >> 3, part = e & 7;
      const int oy = y0 + p / W36_TW, ox = x0 + (p - (p / W36_TW) * W36_TW);
      const bool ok = e < W36_NP * 8 && oy < g.Ho && ox < g.Wo;
      const bf16x8 v = *reinterpret_cast<const bf16x8*>(
          ys + (ok ? (((int64_t)n * g.Ho + oy) * g.Wo + ox) * ycs : 0) + ycc + part * 8);
      yv[k] = ok ? v : bf16x8{};
    }
#pragma unroll
    for (int k = 0; k < HV; ++k) {       // halo: 380 px x 8 vectors (64 ci)
      const int e = tid + k * WG_NT;
      const int hp = e >> 3, part = e & 7;
      const int r = hp / W36_HW, c = hp - r * W36_HW;
      const int iy = y0 - 1 + r, ix = x0 - 1 + c;
      const bool ok = e < W36_NPIX * 8 && (unsigned)iy < (unsigned)g.Hi && (unsigned)ix < (unsigned)g.Wi;
      const bf16x8 v = *reinterpret_cast<const bf16x8*>(
          xs + (ok ? (((int64_t)n * g.Hi + iy) * g.Wi + ix) * xcs : 0) + xcc + part * 8);
      hv[k] = ok ? v : bf16x8{};
    }
  };
  if ((int)blockIdx.z < ntiles) gload(blockIdx.z);
  for (int tile = blockIdx.z; tile < ntiles; tile += gridDim.z) {
    __syncthreads();
#pragma unroll
    for (int k = 0; k < YV; ++k) {
      const int e = tid + k * WG_NT;
      if (e < W36_NP * 8) {
        const int p = e >> 3, part = e & 7;
        const int ch = (part * 2) ^ w3_swz_dy(p);
        *reinterpret_cast<bf16x8*>(sdy + p * 64 + ch * 4) = yv[k];
      }
    }
#pragma unroll
    for (int k = 0; k < HV; ++k) {
      const int e = tid + k * WG_NT;
      if (e < W36_NPIX * 8) {
        const int hp = e >> 3, part = e & 7;
        const int r = hp / W36_HW, row = r * W3_P + (hp - r * W36_HW);
        const int ch = ((part & 3) * 2) ^ w3_swz_x(row);
        *reinterpret_cast<bf16x8*>(shx + (part >> 2) * W3_PLANE + row * 32 + ch * 4) = hv[k];
      }
    }
    __syncthreads();
    if (tile + (int)gridDim.z < ntiles) gload(tile + gridDim.z);
    // flat pixel of this lane's two 4-pixel groups in K-chunk kc: P = kc*32 + r0[half] -> (row, col) of the
    // 36-wide tile (32 < 36: at most one wrap per chunk)
    int prow[2], pcol[2];
#pragma unroll
    for (int half = 0; half < 2; ++half) { prow[half] = 0; pcol[half] = lg * 8 + half * 4 + q; }
    bf16x8 fa[2][WG_NI], fb[2][9];
    auto rd = [&](int kc, int b) {
#pragma unroll
      for (int i = 0; i < WG_NI; ++i)
#pragma unroll
        for (int half = 0; half < 2; ++half) {
          const s16x4 v = __builtin_amdgcn_ds_read_tr16_b64_v4i16((LDS_PTR(s16x4))(sdy + aoff[i][half] + kc * 32 * 64));
#pragma unroll
          for (int e = 0; e < 4; ++e) fa[b][i][half * 4 + e] = __builtin_bit_cast(bf16, (short)v[e]);
        }
      int bo[2][3];
#pragma unroll
      for (int half = 0; half < 2; ++half) {
        const int hb = prow[half] * W3_P + pcol[half];
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) bo[half][kx] = (hb + kx) * 32 + ((cx ^ w3_swz_x(hb + kx)) * 4);
        pcol[half] += 32;
        if (pcol[half] >= W36_TW) { pcol[half] -= W36_TW; ++prow[half]; }
      }
#pragma unroll
      for (int tap = 0; tap < 9; ++tap) {
        const int ky = tap / 3, kx = tap - ky * 3;
#pragma unroll
        for (int half = 0; half < 2; ++half) {
          const s16x4 v = __builtin_amdgcn_ds_read_tr16_b64_v4i16((LDS_PTR(s16x4))(shp + bo[half][kx] + ky * W3_P * 32));
#pragma unroll
          for (int e = 0; e < 4; ++e) fb[b][tap][half * 4 + e] = __builtin_bit_cast(bf16, (short)v[e]);
        }
      }
    };
    auto mm = [&](int b) {
#pragma unroll
      for (int tap = 0; tap < 9; ++tap) {
#pragma unroll
        for (int i = 0; i < WG_NI; ++i)
          acc[i][tap] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[b][i], fb[b][tap], acc[i][tap], 0, 0, 0);
      }
    };
    constexpr int NKC = W36_NP / 32;
    rd(0, 0);
#pragma unroll
    for (int kc = 0; kc < NKC; ++kc) {
      const int b = kc & 1;
      __builtin_amdgcn_sched_barrier(0);
      if (kc + 1 < NKC) rd(kc + 1, b ^ 1);
      mm(b);
      if (kc + 1 < NKC) {
        constexpr int NRD = 2 * WG_NI + 18, NMF = 9 * WG_NI;
        constexpr int NPAIR = NRD < NMF ? NRD : NMF;
#pragma unroll
        for (int q2 = 0; q2 < NPAIR; ++q2) {
          __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);  // 1 DS read
          __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);  // 1 MFMA
        }
        if (NRD > NPAIR) __builtin_amdgcn_sched_group_barrier(0x100, NRD - NPAIR, 0);
        if (NMF > NPAIR) __builtin_amdgcn_sched_group_barrier(0x008, NMF - NPAIR, 0);
      }
      __builtin_amdgcn_sched_barrier(0);
    }
  }
  const int K = 9 * Cin;
  float* out = slab + (int64_t)blockIdx.z * g.Cout * K;
#pragma unroll
  for (int i = 0; i < WG_NI; ++i)
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
      const int ci = ci0 + cit * 16 + lr;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int co = co0 + (cot0 + i) * 16 + lg * 4 + r;
        out[(int64_t)co * K + tap * Cin + ci] = acc[i][tap][r];
      }
    }
}

// dst (+)= sum over the nsplit slabs, remapped to the PyTorch layout.  Block = 64 consecutive slab
// elements x 4 split-groups (coalesced 256-B rows per split), fixed-order combine in LDS.
__global__ __launch_bounds__(256) void conv_wgrad_reduce_kernel(const float* __restrict__ slab, float* __restrict__ dst,
                                                                int nsplit, int Cout, int Cin, int KH, int KW, int swap,
                                                                int flip, int accumulate) {
  const int64_t K = (int64_t)KH * KW * Cin;
  const int64_t total = (int64_t)Cout * K;
  const int64_t e = blockIdx.x * 64ll + (threadIdx.x & 63);
  const int grp = threadIdx.x >> 6;
  float s = 0.f;
  if (e < total) {
    // 8 slab loads in flight, summed in the same order as one at a time (the loop waited out every load: 18.5 us per
    // call, 78 calls per step)
    int k = grp;
    for (; k + 28 < nsplit; k += 32) {
      float v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) v[u] = slab[(int64_t)(k + 4 * u) * total + e];
#pragma unroll
      for (int u = 0; u < 8; ++u) s += v[u];
    }
    for (; k < nsplit; k += 4) s += slab[(int64_t)k * total + e];
  }
  __shared__ float red[4][64];
  red[grp][threadIdx.x & 63] = s;
  __syncthreads();
  if (grp != 0 || e >= total) return;
  s = ((red[0][threadIdx.x] + red[1][threadIdx.x]) + red[2][threadIdx.x]) + red[3][threadIdx.x];
  const int co = (int)(e / K);
  const int kc = (int)(e - (int64_t)co * K);
  const int tap = kc / Cin, ci = kc - tap * Cin;
  int ky = tap / KW, kx = tap - ky * KW;
  if (flip) { ky = KH - 1 - ky; kx = KW - 1 - kx; }
  const int d0 = swap ? ci : co, d1 = swap ? co : ci, D1 = swap ? Cout : Cin;
  const int64_t di = (((int64_t)d0 * D1 + d1) * KH + ky) * KW + kx;
  dst[di] = accumulate ? dst[di] + s : s;
}

// per-channel column sum over rows of a channels-last matrix: partial[split][c]
template <typename T>
__global__ void colsum_partial_kernel(const T* __restrict__ x, float* __restrict__ part, int64_t rows, int C,
                                      int64_t rows_per_split) {
  // block: 256 threads = (256/ (C/4)) row-lanes x (C/4) channel-quads  (C <= 1024, C % 4 == 0)
  const int cq = C / 4;
  const int rl = 256 / cq;
  const int tid = threadIdx.x;
  const int q = tid % cq, rr = tid / cq;
  __shared__ float red[256 * 4];
  float s[4] = {0.f, 0.f, 0.f, 0.f};
  const int64_t r0 = blockIdx.x * rows_per_split;
  const int64_t r1 = min(rows, r0 + rows_per_split);
  if (rr < rl) {
    for (int64_t r = r0 + rr; r < r1; r += rl) {
      float v[4];
      load4(x + r * C + q * 4, v);
      s[0] += v[0]; s[1] += v[1]; s[2] += v[2]; s[3] += v[3];
    }
  }
  for (int i = 0; i < 4; ++i) red[tid * 4 + i] = s[i];
  __syncthreads();
  if (tid < cq) {
    float t[4] = {0.f, 0.f, 0.f, 0.f};
    for (int k = 0; k < rl; ++k)
      for (int i = 0; i < 4; ++i) t[i] += red[(k * cq + tid) * 4 + i];
    for (int i = 0; i < 4; ++i) part[(int64_t)blockIdx.x * C + tid * 4 + i] = t[i];
  }
}

// one 64-lane wave per channel: lanes stride over the splits, then a fixed-order wave sum
__global__ void colsum_final_kernel(const float* __restrict__ part, float* __restrict__ dst, int nsplit, int C,
                                    int accumulate) {
  const int c = blockIdx.x;
  float s = 0.f;
  for (int k = threadIdx.x; k < nsplit; k += 64) s += part[(int64_t)k * C + c];
  s = wave_sum(s);
  if (threadIdx.x == 0) dst[c] = accumulate ? dst[c] + s : s;
}

// Kernel selection and launch shape of cesm_conv_wgrad (host only): the launcher and every cesm_conv_wgrad_* query go
// through wgrad_plan, so the caller's slab, the launch and the tests see one decision.
enum WgradVariant { WGV_WIDE = 0, WGV_SQ, WGV_GEN, WGV_S2, WGV_W32C64, WGV_W36C64 };

// Target block counts of the split-K launches.  Every split writes a full fp32 [Cout][K] slab that conv_wgrad_reduce
// reads back, so more blocks than ~2-4 per CU only adds slab traffic (round 3: 512 / 2048 blocks 144.7 / 131.2 ms per
// step against 129.7 at 1024).  The split count fixes the summation order, and with it the bits, of every dW.
constexpr int WG_BLOCKS = 1024;      // wide kernel with 64- / 128-row tiles, generic kernel
constexpr int WG_BLOCKS_BIG = 512;   // wide kernel with 256-row tiles; halo / stride-2 kernels (64 co x 32 ci blocks)
constexpr int WG_BLOCKS_SQ = 256;    // square-tile kernel (512 threads, 64 KB of LDS: two per CU) at 256 rows ...
constexpr int WG_BLOCKS_SQ64 = 512;  // ... and at 64 rows (100 registers, two per CU)
constexpr int WG_SPLIT_PX = 256;     // a split takes at least 256 pixels

struct WgradPlan {
  WgradVariant v = WGV_GEN;
  int bm = 64, bn = 64;   // output tile (co rows x K columns) of the wide / square-tile kernels
  int nsplit = 1;         // pixel splits: what a caller sizes the slabs for
  bool bias = false;      // this launch also produces the bias gradient (with_bias and a kernel that carries it)
  bool can_bias = false;  // a caller that wants the bias gradient should ask for it here (else: cesm_colsum)
};

static WgradPlan wgrad_plan(int dtype, int Nb, int Hi, int Wi, int C1, int C2, int Ho, int Wo, int Cout, int Co1,
                            int KH, int KW, int S, int P, int U, bool with_bias) {
  WgradPlan pl;
  const bool bf = dtype == CESM_DT_BF16;
  const int Cin = C1 + C2, K = KH * KW * Cin;
  const int64_t M = (int64_t)Nb * Ho * Wo;
  const bool same_hw = Ho == Hi && Wo == Wi, single = C2 == 0 && Co1 == Cout;  // one source, one destination
  int64_t blocks = WG_BLOCKS, tiles;
  if (bf && KH == 3 && KW == 3 && S == 1 && P == 1 && U == 1 && same_hw) {
    // halo kernels, blocks of 64 co x 32 ci over all 9 taps (C1 % 64 == 0: cesm_conv_wgrad).  8 x 36 tiles only where
    // 32-wide tiles waste >= 20 % of the columns (W = 36, 72); at W = 144 / 288 the 8 x 32 kernel's row-aligned K
    // chunks are faster despite the partial last tile
    pl.v = ((Wo % W36_TW) == 0 && 5 * Wo <= 4 * (int)cdiv(Wo, W3_TW) * W3_TW) ? WGV_W36C64 : WGV_W32C64;
    blocks = WG_BLOCKS_BIG;
    tiles = (int64_t)(Cout / 64) * (Cin / 32);
  } else if (bf && KH == 4 && KW == 4 && S == 2 && P == 1 && U == 1 && Hi == 2 * Ho && Wi == 2 * Wo && Wo >= 64 &&
             single && !with_bias) {
    // 4x4 stride-2 (Downsample / the Upsample's weight gradient): blocks of 64 co x 32 ci x one input parity (4 taps);
    // no concat, no split and no bias gradient (those take the wide kernel below)
    // (32-wide pixel tiles: at Wo = 36 the second tile of a row is 8/9 empty and the wide kernel is faster)
    pl.v = WGV_S2;
    blocks = WG_BLOCKS_BIG;
    tiles = (int64_t)(Cout / 64) * (Cin / 32) * 4;
  } else {
    // wide-tile kernel, or for fp32 / M >= 2^31 the generic one.  Square 256 (64) x bn tiles instead for the 1x1 convs
    // whose dY the wide kernel would re-read once per 64 input channels: one source, one destination; Cout % 256 == 0
    // with bn = 256 when Cin % 256 == 0, else 128; or Cout = 64 with Cin % 256 == 0 (the level-0 to_out)
    const bool wide = bf && M < (1ll << 31);
    int sq = 0;
    if (wide && KH == 1 && KW == 1 && S == 1 && P == 0 && U == 1 && same_hw && single) {
      if (Cout == 64) sq = C1 % 256 == 0 ? 256 : 0;
      else if (Cout % 256 == 0) sq = C1 % 256 == 0 ? 256 : (C1 % 128 == 0 ? 128 : 0);
    }
    pl.v = sq ? WGV_SQ : (wide ? WGV_WIDE : WGV_GEN);
    if (sq) {
      pl.bm = Cout == 64 ? 64 : 256;
      pl.bn = sq;
      blocks = pl.bm == 64 ? WG_BLOCKS_SQ64 : WG_BLOCKS_SQ;
    } else {
      // (the generic kernel's tiles are 64 x 64; a bf16 launch it takes keeps the wide kernel's split count)
      pl.bm = !bf ? 64 : (Cout % 256 == 0 && Co1 % 256 == 0) ? 256 : (Cout % 128 == 0 && Co1 % 128 == 0) ? 128 : 64;
      blocks = pl.bm == 256 ? WG_BLOCKS_BIG : WG_BLOCKS;
    }
    tiles = (int64_t)std::max(1, Cout / pl.bm) * std::max(1, K / pl.bn);
    pl.bias = with_bias && wide;
    // (the wide kernel could also carry the bias gradient of a split destination; those layers have taken it from the
    // column sum since round 3, and moving them would change db's summation order)
    pl.can_bias = wide && Co1 == Cout;
  }
  pl.nsplit = (int)std::max<int64_t>(
      1, std::min(blocks / std::max<int64_t>(1, tiles), std::max<int64_t>(1, M / WG_SPLIT_PX)));
  return pl;
}
}  // namespace

extern "C" {

const char* cesm_conv_wgrad_variant(int dtype, int Nb, int Hi, int Wi, int C1, int C2, int Ho, int Wo, int Cout,
                                    int Co1, int KH, int KW, int S, int P, int U, int with_bias) {
  const WgradPlan pl = wgrad_plan(dtype, Nb, Hi, Wi, C1, C2, Ho, Wo, Cout, Co1, KH, KW, S, P, U, with_bias != 0);
  switch (pl.v) {
    case WGV_W32C64: return "wgrad3x3c64_kernel";
    case WGV_W36C64: return "wgrad3x3w36c64_kernel";
    case WGV_S2: return "wgrads2_bf16_kernel";
    case WGV_SQ: {
      static const char* const sqn[6] = {"wgrad_sq_kernel<64,256>", "wgrad_sq_kernel<64,256,true>",
                                         "wgrad_sq_kernel<256,256>", "wgrad_sq_kernel<256,256,true>",
                                         "wgrad_sq_kernel<256,128>", "wgrad_sq_kernel<256,128,true>"};
      return sqn[(pl.bm == 64 ? 0 : pl.bn == 256 ? 2 : 4) + (with_bias ? 1 : 0)];
    }
    case WGV_WIDE: {
      static const char* const names[6] = {"wgrad_wide_kernel<64,false>", "wgrad_wide_kernel<64,true>",
                                           "wgrad_wide_kernel<128,false>", "wgrad_wide_kernel<128,true>",
                                           "wgrad_wide_kernel<256,false>", "wgrad_wide_kernel<256,true>"};
      return names[(pl.bm == 256 ? 4 : pl.bm == 128 ? 2 : 0) + (with_bias ? 1 : 0)];
    }
    default: return dtype == CESM_DT_BF16 ? "conv_wgrad_kernel<__bf16>" : "conv_wgrad_kernel<float>";
  }
}

int cesm_conv_wgrad_nsplit(int dtype, int Nb, int Hi, int Wi, int C1, int C2, int Ho, int Wo, int Cout, int Co1, int KH,
                           int KW, int S, int P, int U, int with_bias) {
  return wgrad_plan(dtype, Nb, Hi, Wi, C1, C2, Ho, Wo, Cout, Co1, KH, KW, S, P, U, with_bias != 0).nsplit;
}

int cesm_conv_wgrad_bias_rides(int dtype, int Nb, int Hi, int Wi, int C1, int C2, int Ho, int Wo, int Cout, int Co1,
                               int KH, int KW, int S, int P, int U) {
  return wgrad_plan(dtype, Nb, Hi, Wi, C1, C2, Ho, Wo, Cout, Co1, KH, KW, S, P, U, false).can_bias ? 1 : 0;
}

// Weight gradient of the conv whose forward launch had geometry (…, KH, KW, S, P, U).
// x = forward input (two sources), dy = forward output grad (two destinations, Co1 split).
// Result accumulated/written into the PyTorch weight tensor `dw` ([D0][D1][1][KH][KW] with the
// (swap, flip) mapping of the pack).  `slab` is an fp32 workspace of nsplit*Cout*K floats; nsplit is the caller's
// (cesm_conv_wgrad_nsplit in the product path; any value >= 1 is correct).
int cesm_conv_wgrad(int dtype, const void* x1, const void* x2, const void* dy1, const void* dy2, float* dw,
                    float* slab, float* db, float* bslab, int nsplit, int Nb, int Hi, int Wi, int C1, int C2, int Ho,
                    int Wo, int Cout, int Co1, int KH, int KW, int S, int P, int U, int swap, int flip, int accumulate,
                    hipStream_t stream) {
  if (db && !bslab) return CESM_EINVAL;
  const int Cin = C1 + C2;
  if ((Cin % 64) || (C1 % 64) || (Cout % 64) || (Co1 % 64) || nsplit <= 0) return CESM_EINVAL;
  if (dtype != CESM_DT_BF16 && dtype != CESM_DT_F32) return CESM_EINVAL;
  const WgradPlan pl = wgrad_plan(dtype, Nb, Hi, Wi, C1, C2, Ho, Wo, Cout, Co1, KH, KW, S, P, U, db != nullptr);
  if (db && !pl.bias) return CESM_EUNSUPPORTED;  // the bias gradient rides only on the wide / square-tile kernels
  ConvGeom g{Nb, Hi, Wi, Ho, Wo, C1, C2, Cout, Co1, KH, KW, S, P, U};
  const int64_t M = (int64_t)Nb * Ho * Wo;
  const int64_t pps = cdiv(cdiv(M, nsplit), WG_BP) * WG_BP;
  const int K = KH * KW * Cin;
  switch (pl.v) {
    case WGV_W36C64: {
      const int tx = Wo / W36_TW;
      const int ntiles = Nb * tx * (int)cdiv(Ho, W36_TH);
      dim3 g3(Cout / 64, Cin / 64, std::min(nsplit, ntiles));
      wgrad3x3w36c64_kernel<<<g3, WG_NT, 0, stream>>>((const bf16*)x1, (const bf16*)x2, (const bf16*)dy1,
                                                    (const bf16*)dy2, slab, g, tx, ntiles);
      nsplit = (int)g3.z;
      break;
    }
    case WGV_W32C64: {
      const int tx = (int)cdiv(Wo, W3_TW);
      const int ntiles = Nb * tx * (int)cdiv(Ho, W3_TH);
      dim3 g3(Cout / 64, Cin / 64, std::min(nsplit, ntiles));
      wgrad3x3c64_kernel<<<g3, WG_NT, 0, stream>>>((const bf16*)x1, (const bf16*)x2, (const bf16*)dy1,
                                                 (const bf16*)dy2, slab, g, tx, ntiles);
      nsplit = (int)g3.z;
      break;
    }
    case WGV_S2: {
      const int tx = (int)cdiv(Wo, W3_TW);
      const int ntiles = Nb * tx * (int)cdiv(Ho, W3_TH);
      dim3 g3(Cout / 64, (Cin / 32) * 4, std::min(nsplit, ntiles));
      wgrads2_bf16_kernel<<<g3, 256, 0, stream>>>((const bf16*)x1, (const bf16*)dy1, slab, g, tx, ntiles);
      nsplit = (int)g3.z;
      break;
    }
    case WGV_SQ: {
      const dim3 gq(Cout / pl.bm, Cin / pl.bn, nsplit);
      const bf16 *qx = (const bf16*)x1, *qy = (const bf16*)dy1;
#define SQL(BMv, BNv, Bv) \
  wgrad_sq_kernel<BMv, BNv, Bv><<<gq, 512, 0, stream>>>(qx, qy, slab, bslab, (int)M, Cout, Cin, (int)pps)
      if (pl.bm == 64) { if (db) SQL(64, 256, true); else SQL(64, 256, false); }
      else if (pl.bn == 256) { if (db) SQL(256, 256, true); else SQL(256, 256, false); }
      else { if (db) SQL(256, 128, true); else SQL(256, 128, false); }
#undef SQL
      break;
    }
    case WGV_WIDE: {
      const dim3 gw(Cout / pl.bm, K / 64, nsplit);
      auto launch = [&](auto bmc, auto biasc) {
        constexpr int BMv = decltype(bmc)::value;
        constexpr bool Bv = decltype(biasc)::value;
        wgrad_wide_kernel<BMv, Bv><<<gw, 256, 0, stream>>>((const bf16*)x1, (const bf16*)x2, (const bf16*)dy1,
                                                           (const bf16*)dy2, slab, bslab, g, (int)M, (int)pps);
      };
      using T0 = std::false_type;
      using T1 = std::true_type;
      if (pl.bm == 256) { if (db) launch(std::integral_constant<int, 256>{}, T1{}); else launch(std::integral_constant<int, 256>{}, T0{}); }
      else if (pl.bm == 128) { if (db) launch(std::integral_constant<int, 128>{}, T1{}); else launch(std::integral_constant<int, 128>{}, T0{}); }
      else { if (db) launch(std::integral_constant<int, 64>{}, T1{}); else launch(std::integral_constant<int, 64>{}, T0{}); }
      break;
    }
    case WGV_GEN: {
      dim3 grid(Cout / 64, K / 64, nsplit);
      if (dtype == CESM_DT_BF16)
        conv_wgrad_kernel<bf16><<<grid, 256, 0, stream>>>((const bf16*)x1, (const bf16*)x2, (const bf16*)dy1,
                                                          (const bf16*)dy2, slab, g, M, pps);
      else
        conv_wgrad_kernel<float><<<grid, 256, 0, stream>>>((const float*)x1, (const float*)x2, (const float*)dy1,
                                                           (const float*)dy2, slab, g, M, pps);
      break;
    }
  }
  if (db) colsum_final_kernel<<<Cout, 64, 0, stream>>>(bslab, db, nsplit, Cout, 1);
  const int64_t total = (int64_t)Cout * K;
  conv_wgrad_reduce_kernel<<<(unsigned)cdiv(total, 64), 256, 0, stream>>>(slab, dw, nsplit, Cout, Cin, KH, KW, swap,
                                                                          flip, accumulate);
  return cesm_launch_status();
}

// dst[c] (+)= sum_r x[r][c] ; part = workspace nsplit*C floats
int cesm_colsum(int dtype, const void* x, float* dst, float* part, int nsplit, int64_t rows, int C, int accumulate,
                hipStream_t stream) {
  if (C % 4 || C > 1024 || nsplit <= 0) return CESM_EINVAL;
  const int64_t rps = cdiv(rows, nsplit);
  if (dtype == CESM_DT_BF16)
    colsum_partial_kernel<bf16><<<nsplit, 256, 0, stream>>>((const bf16*)x, part, rows, C, rps);
  else if (dtype == CESM_DT_F32)
    colsum_partial_kernel<float><<<nsplit, 256, 0, stream>>>((const float*)x, part, rows, C, rps);
  else
    return CESM_EINVAL;
  colsum_final_kernel<<<C, 64, 0, stream>>>(part, dst, nsplit, C, accumulate);
  return cesm_launch_status();
}

}  // extern "C"
