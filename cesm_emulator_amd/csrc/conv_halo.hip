// Halo-tiled implicit-GEMM convolutions (bf16): the 3x3 / stride-1 conv of levels 1-3 (conv3x3_bf16_kernel) and the 4x4 /
// stride-2 down- and up-sampling convs (convs2_bf16_kernel), with their launchers.  conv_fwd_plan (conv_fwd.hip) decides
// when they run and with which tile; conv_fwd_launch calls conv_halo3_launch / conv_s2_launch below.
#include "conv_common.h"

namespace {

// ----------------------------------------------------------------------------------------
// 3x3 / stride 1 / pad 1 conv (bf16): halo-tiled implicit GEMM.  Block = 8 x 32 output pixels of
// one image x 64 output channels.  Per 32-channel input chunk the (8+2) x (32+2) input halo and
// the 9 taps x 64 co weights are staged in LDS once and all 9 taps read shifted windows of the
// halo (9x fewer input loads than im2col).  The next chunk is prefetched into registers while the
// current one is consumed.  4 waves = 2 (co halves) x 2 (pixel halves of 4 rows).
// ----------------------------------------------------------------------------------------
// (H3_TH, H3_TW, H3_BN -- the default tile and the 64 output channels of a block: conv_common.h)
constexpr int H3_P = 40;                 // LDS halo row pitch (pixels): >= TW+2, multiple of 8 (see below)
constexpr int H3_NROW = 10 * H3_P;       // LDS halo rows ((TH+2) <= 10 tile rows of H3_P pixels)
constexpr int H3_LD = 32;                // bf16 per LDS row: 32 channels = 64 B, no padding
// element offset of 16-B chunk `ch` (8 channels) of LDS row `row`: 64-B rows, chunk index XORed with
// bit 2 of the row.  ds_read_b128 of 16 rows r0..r0+15 (lane = row, lane group = chunk) is then
// bank-conflict free for any r0 (the 80-B padded rows it replaces ran 2-3-way conflicted: PMC
// SQ_LDS_BANK_CONFLICT = 51 % of LDS cycles at level 3).  Steps of 8 rows keep the swizzle, so the
// tap offsets ky * H3_P and tap * 64 stay immediate.
__device__ __forceinline__ int h3_off(int row, int ch) { return row * H3_LD + ((ch ^ ((row >> 1) & 2)) << 3); }

// The halo conv's measured alternatives, removed in round 6 (profiles/r2_*, r3_*, r5_prio_ab.txt): staging
// through registers instead of LDS-DMA, the compiler's read -> MFMA tap order, 32 co x 128 px wave tiles, co-block-
// slowest (not XCD-grouped) block order, 256-pixel tiles only, and s_setprio around the MFMA phase.
// epilogue of the halo conv (conv3x3_bf16_kernel; a function since round 5's double-buffered variant): bias, residual, bf16 stores and the GroupNorm
// statistics partials; lane holds co = n0 + wr*32 + i*16 + 4*lg + r of pixel pyx[j] (packed (py << 16) | px, -1 past TH)
template <int NI, int NJ>
__device__ __forceinline__ void h3_epilogue(const f32x4 (&acc)[NI][NJ], const int (&pyx)[NJ], const ConvGeom& g,
                                            const float* __restrict__ bias, const bf16* __restrict__ res,
                                            const bf16* __restrict__ res2, bf16* __restrict__ y1, bf16* __restrict__ y2,
                                            float* __restrict__ gnp, int gn_fimg, int n, int tt, int ntile, int y0,
                                            int x0, int n0, int wr, int wc, int lane) {
  const int lr = lane & 15, lg = lane >> 4;
  const int Co2 = g.Cout - g.Co1;
  float bv[NI][4];
#pragma unroll
  for (int i = 0; i < NI; ++i) epi_bias(bias, n0 + wr * 32 + i * 16 + lg * 4, bv[i]);
  int64_t mj[NJ];
  bool okj[NJ];
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const int oy = y0 + (pyx[j] >> 16), ox = x0 + (pyx[j] & 0xffff);
    okj[j] = pyx[j] >= 0 && oy < g.Ho && ox < g.Wo;
    mj[j] = okj[j] ? ((int64_t)n * g.Ho + oy) * g.Wo + ox : 0;
  }
  bf16x4 rv[NJ][NI];
  if (res || res2) {  // uniform
#pragma unroll
    for (int j = 0; j < NJ; ++j)
#pragma unroll
      for (int i = 0; i < NI; ++i) rv[j][i] = epi_res(res, res2, mj[j], n0 + wr * 32 + i * 16 + lg * 4, g.Co1, Co2, okj[j]);
  } else {
#pragma unroll
    for (int j = 0; j < NJ; ++j)
#pragma unroll
      for (int i = 0; i < NI; ++i) rv[j][i] = bf16x4{};
  }
  // GroupNorm statistics partials (gnp: the Block conv feeding a GroupNorm): per channel quad (i, lg) the sum
  // and sum of squares of the stored bf16 output over this wave's valid pixels
  float gsum[NI], gsq[NI];
#pragma unroll
  for (int i = 0; i < NI; ++i) gsum[i] = gsq[i] = 0.f;
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    if (!okj[j]) continue;
    const int64_t m = mj[j];
#pragma unroll
    for (int i = 0; i < NI; ++i) {
      const int co = n0 + wr * 32 + i * 16 + lg * 4;
      float v[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) v[r] = acc[i][j][r] + bv[i][r] + b2f(rv[j][i], r);
      if (gnp) {  // uniform: the statistics of the stored (bf16-rounded) y, which GroupNorm then normalises
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = (float)(bf16)v[r];
      }
      if (co < g.Co1) store4(y1 + m * g.Co1 + co, v);
      else store4(y2 + m * Co2 + (co - g.Co1), v);
      if (gnp) {  // uniform
        gsum[i] += (v[0] + v[1]) + (v[2] + v[3]);
        gsq[i] += fmaf(v[3], v[3], fmaf(v[2], v[2], fmaf(v[1], v[1], v[0] * v[0])));
      }
    }
  }
  if (gnp) {
    const int b = n / gn_fimg, f = n - b * gn_fimg;
    constexpr int SPT = 4;  // GroupNorm slots per tile (= pixel ranges): h3_gn_slots
    const int64_t nslot = (int64_t)gn_fimg * ntile * SPT;
    const int64_t slot = ((int64_t)f * ntile + tt) * SPT + wc;
    float2* dst = reinterpret_cast<float2*>(gnp) + ((int64_t)b * nslot + slot) * (g.Cout / 4) + (n0 + wr * 32) / 4 + lg;
#pragma unroll
    for (int i = 0; i < NI; ++i) {
      const float a = row16_sum(gsum[i]), q = row16_sum(gsq[i]);
      if (lr == 0) dst[i * 4] = make_float2(a, q);
    }
  }
}

// (Round 3: double-buffered chunks at one block per CU measured slower, conv total 64.0 -> 68.2 ms per step: the
// second co-resident block hides the staging better than an in-block prefetch.  Removed.  Round 6: 16-channel stages in
// a double buffer at two blocks per CU, each K = 32 MFMA step taking two taps of a stage (so the K = 32 rate is kept,
// unlike round 5's K = 16 form), 44-pixel halo pitch with a conflict-free 32-B-row swizzle: correct, 385 vs 336 us per
// launch -- the extra zero-half step for the 9th tap, twice the barriers and the per-tap address VALU outweigh the
// overlap (profiles/r6o_tap_pair_conv_ab.txt).  Removed.  Also round 6: an L2 touch of chunk ch + 1's weight and
// halo lines (4 B per 128-B line, LDS-direct) issued while chunk ch computes -- the step's halo conv calls 1 % faster,
// the step 0.3 ms slower (profiles/r6late_h3_touch_ab.txt).  Removed.)
#ifdef CESM_H3_STAMPS
__device__ uint64_t* g_h3_stamp_buf = nullptr;
__device__ int g_h3_stamp_blocks = 0;
#endif
template <int TW, int NJv = 4>
__global__ __launch_bounds__(256, 2) void conv3x3_bf16_kernel(const bf16* __restrict__ x1, const bf16* __restrict__ x2,
                                                              const bf16* __restrict__ w, const float* __restrict__ bias,
                                                              const bf16* __restrict__ res, const bf16* __restrict__ res2,
                                                              bf16* __restrict__ y1, bf16* __restrict__ y2, ConvGeom g,
                                                              int tiles_x, int TH, float* __restrict__ gnp = nullptr,
                                                              int gn_fimg = 1) {
  // NJv = 7: tiles of up to 448 pixels ((TH+2) <= 16 halo rows of H3_P), 64 co x 112 px per wave: 11
  // fragment reads per 28 MFMAs per tap (0.39 per MFMA instead of 0.5) and the 36-KiB weight chunk staged once
  // per 448 instead of 256 pixels; 77 KiB of LDS, still 2 blocks per CU
  static_assert(NJv == 4 || NJv == 7, "256- or 448-pixel tiles");
  constexpr int NROWS = (NJv == 7 ? 16 : 10) * H3_P;
  __shared__ __attribute__((aligned(16))) bf16 sh[NROWS * H3_LD];
  // the weight tile as three arrays of 3 taps each: distinct LDS objects, so the compiler's wait insertion can see that
  // reads of taps 0-2 do not depend on the DMA still landing taps 3-8
  __shared__ __attribute__((aligned(16))) bf16 sw0[3 * H3_BN * H3_LD];
  __shared__ __attribute__((aligned(16))) bf16 sw1[3 * H3_BN * H3_LD];
  __shared__ __attribute__((aligned(16))) bf16 sw2[3 * H3_BN * H3_LD];
  auto swt = [&](int k) { return k == 0 ? sw0 : (k == 1 ? sw1 : sw2); };  // k compile-time after unrolling
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  // wave tile (round 3): 64 co x 16 NJv px = 4 x NJv MFMA tiles per wave (8 fragment reads per 16 MFMAs per
  // tap at NJv = 4); else 32 co x 128 px = 2 x 8 (10 reads per 16 MFMAs: the 4 waves' reads exceeded the LDS
  // array's 256 B/clk)
  constexpr int NI = 4, NJ = NJv;
  const int wr = 0, wc = wid;
  constexpr int PXW = 16 * NJ;  // pixels per wave
  // 1-D grid (h3_grid): the ncob co blocks of a (image, tile) run back to back on ONE XCD (linear id mod 8), so
  // its input halo is fetched into that XCD's L2 once (co-block-slowest order re-read every halo ncob times)
  const int ntile = tiles_x * ((g.Ho + TH - 1) / TH), ncob = g.Cout / H3_BN;
  const int L = blockIdx.x, jx = L >> 3;
  const int cb = jx % ncob;
  const int tflat = (jx / ncob) * 8 + (L & 7);
  if (tflat >= g.Nb * ntile) return;  // padded items (whole block)
  const int n = tflat / ntile, tt = tflat - n * ntile;
  const int ty = tt / tiles_x, tx = tt - ty * tiles_x;
  const int y0 = ty * TH, x0 = tx * TW;
  constexpr int HWd = TW + 2;
  const int n0 = cb * H3_BN;
  const int Cin = g.C1 + g.C2;
  const int nchunk = Cin / 32;

  // stage one 32-channel chunk by buffer-LDS-DMA (no registers, no address VALU per element beyond one per
  // 16-B piece): 1-KiB pieces of 16 LDS rows, each lane fetching the global chunk that the row swizzle puts in
  // its slot (chunk = slot ^ ((row >> 1) & 2)); halo rows outside the tile / image read as zeros (out-of-range
  // offset).  The second co-resident block computes while this one waits.
  auto stage = [&](int ch) {
    const int c0 = ch * 32;
    const bf16* src;
    int cs, cc;
    if (c0 < g.C1) { src = x1; cs = g.C1; cc = c0; } else { src = x2; cs = g.C2; cc = c0 - g.C1; }
    const int64_t img = (int64_t)g.Hi * g.Wi * cs;
    const __amdgpu_buffer_rsrc_t xrs =
        __builtin_amdgcn_make_buffer_rsrc((void*)(src + n * img + cc), (short)0, (int)(img * 2 - cc * 2), 0x00020000);
    // this (co block, chunk)'s weight tile: one contiguous [tap][co][32] block of the chunked pack (wpk_index)
    const __amdgpu_buffer_rsrc_t wrs = __builtin_amdgcn_make_buffer_rsrc(
        (void*)(w + ((int64_t)cb * nchunk + ch) * (9 * H3_BN * 32)), (short)0, 9 * H3_BN * 32 * 2, 0x00020000);
    const int prow = lane >> 2, pslot = lane & 3;
    constexpr int HPC = NROWS / 16;  // halo pieces (25 / 40)
    // NJv = 7: only the pieces the tile's halo rows span (pixels past the tile read row 0);
    // NJv = 4 at TW = 32 reads rows up to 9 for pixels past a short tile (discarded), so all 25 are staged
    const int hpc = NJv == 4 ? HPC : ((TH + 2) * H3_P + 15) >> 4;
#pragma unroll
    for (int k = 0; k < (HPC + 3) / 4; ++k) {
      const int q = wid + 4 * k;
      if (q < hpc) {  // wave-uniform
        const int row = 16 * q + prow;
        const int r = row / H3_P, col = row - r * H3_P;
        const int iy = y0 - 1 + r, ix = x0 - 1 + col;
        const bool in = r < TH + 2 && col < HWd && (unsigned)iy < (unsigned)g.Hi && (unsigned)ix < (unsigned)g.Wi;
        const int chunk = pslot ^ ((row >> 1) & 2);
        const int vo = in ? ((iy * g.Wi + ix) * cs + chunk * 8) * 2 : 0x7ffffff0;
        __builtin_amdgcn_raw_ptr_buffer_load_lds(xrs, (__attribute__((address_space(3))) void*)(sh + q * 512), 16, vo, 0,
                                                 0, 0);
      }
    }
#pragma unroll
    for (int k = 0; k < 9; ++k) {  // weights: 9 taps x 64 co rows = 36 pieces, each 1 KiB of the tile
      const int q = wid + 4 * k, row = 16 * q + prow;  // row = tap * 64 + co
      const int chunk = pslot ^ ((row >> 1) & 2);
      __builtin_amdgcn_raw_ptr_buffer_load_lds(wrs, (__attribute__((address_space(3))) void*)(swt(k / 3) + (q - 12 * (k / 3)) * 512),
                                               16, (row * 32 + chunk * 8) * 2, 0, 0, 0);
    }
  };
#ifdef CESM_H3_STAMPS
  // diagnostic build only (tools/h3_stamps.py): per wave, cycles spent in each phase of the chunk loop
  uint64_t hs[8] = {}, hland[8] = {};
  const uint64_t h_t0 = __builtin_amdgcn_s_memtime();
  uint64_t h_t = h_t0;
  auto hstamp = [&](int k) {
    const uint64_t t = __builtin_amdgcn_s_memtime();
    hs[k] += t - h_t;
    h_t = t;
  };
#define H3STAMP(k) hstamp(k)
#else
#define H3STAMP(k)
#endif

  f32x4 acc[NI][NJ];
#pragma unroll
  for (int i = 0; i < NI; ++i)
#pragma unroll
    for (int j = 0; j < NJ; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int lr = lane & 15, lg = lane >> 4;
  // pixel group j of this wave: tile pixel p = wc*PXW + j*16 + lr -> halo row of tap (0,0)
  int hoff[NJ], pyx[NJ];
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    int py, px;
    if constexpr (TW == 32 && NJ % 2 == 0) {  // rows of two 16-pixel groups: compile-time offsets per j
      py = wc * (NJ / 2) + (j >> 1);
      px = (j & 1) * 16 + lr;
    } else {
      const int p = wc * PXW + j * 16 + lr;
      py = p / TW;
      px = p - py * TW;
    }
    const bool in = py < TH;
    // TW == 32: rows past TH stay inside the LDS halo buffer (results discarded), no select needed
    hoff[j] = ((TW == 32 && NJ % 2 == 0) || in) ? py * H3_P + px : 0;
    pyx[j] = in ? (py << 16) | px : -1;
  }
  // fragment addresses for ky = 0 / tap = 0; the other taps add immediates (swizzle-preserving steps)
  int boff[NJ][3], aoff[NI];
#pragma unroll
  for (int j = 0; j < NJ; ++j)
#pragma unroll
    for (int kx = 0; kx < 3; ++kx) boff[j][kx] = h3_off(hoff[j] + kx, lg);
#pragma unroll
  for (int i = 0; i < NI; ++i) aoff[i] = h3_off(wr * 32 + i * 16 + lr, lg);
  for (int ch = 0; ch < nchunk; ++ch) {
    if (ch) __syncthreads();  // previous chunk fully consumed
    H3STAMP(0);
    stage(ch);
    H3STAMP(1);
    // progressive landing: each wave's 9 weight pieces are the youngest, piece k = tap k; wait for the halo and taps
    // 0-2 only, and for taps 3-5 / 6-8 at the tap loop's two later barriers
    asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
    H3STAMP(2);
    __builtin_amdgcn_s_barrier();
    H3STAMP(3);
#ifdef CESM_H3_STAMPS
    if (ch < 8) hland[ch] = h_t;
#endif
    // the 10 fragment reads of tap t+1 are issued between the 16 MFMAs of tap t (two register sets), so no
    // MFMA waits on a read issued just before it (the compiler's order was read -> wait -> 2 MFMAs)
    bf16x8 fa[2][NI], fb[2][NJ];
    auto rd = [&](int tap, int b) {
      const int ky = tap / 3, kx = tap - ky * 3;
#pragma unroll
      for (int i = 0; i < NI; ++i)
        fa[b][i] = *reinterpret_cast<const bf16x8*>(swt(tap / 3) + aoff[i] + (tap % 3) * H3_BN * H3_LD);
#pragma unroll
      for (int j = 0; j < NJ; ++j) fb[b][j] = *reinterpret_cast<const bf16x8*>(sh + boff[j][kx] + ky * H3_P * H3_LD);
    };
    rd(0, 0);
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
      const int b = tap & 1;
      const bool gate = tap == 2 || tap == 5;  // the next tap's weights land behind a barrier
      __builtin_amdgcn_sched_barrier(0);
      if (tap + 1 < 9 && !gate) rd(tap + 1, b ^ 1);
#pragma unroll
      for (int j = 0; j < NJ; ++j)
#pragma unroll
        for (int i = 0; i < NI; ++i)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[b][i], fb[b][j], acc[i][j], 0, 0, 0);
      if (gate) {
        __builtin_amdgcn_sched_barrier(0);
        if (tap == 2) asm volatile("s_waitcnt vmcnt(3)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        rd(tap + 1, b ^ 1);
      } else if (tap + 1 < 9) {
#pragma unroll
        for (int q2 = 0; q2 < NI + NJ; ++q2) {
          __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);  // 1 DS read
          __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);  // 1 MFMA
        }
        __builtin_amdgcn_sched_group_barrier(0x008, NI * NJ - (NI + NJ), 0);
      }
      __builtin_amdgcn_sched_barrier(0);
    }
    H3STAMP(4);
  }
  h3_epilogue<NI, NJ>(acc, pyx, g, bias, res, res2, y1, y2, gnp, gn_fimg, n, tt, ntile, y0, x0, n0, wr, wc, lane);
#ifdef CESM_H3_STAMPS
  H3STAMP(5);
  // record: [hw_id | xcc_id << 32, t0, t_end, hs[0..5], land[0..6]] -- vector stores from lane 0 to the diagnostic
  // buffer only
  if (g_h3_stamp_buf && lane == 0 && L < g_h3_stamp_blocks) {
    uint64_t* o = g_h3_stamp_buf + ((int64_t)L * 4 + wid) * 16;
    const uint32_t hwid = __builtin_amdgcn_s_getreg((31 << 11) | 4), xcc = __builtin_amdgcn_s_getreg((15 << 11) | 20);
    o[0] = hwid | ((uint64_t)xcc << 32);
    o[1] = h_t0;
    o[2] = h_t;
#pragma unroll
    for (int k = 0; k < 6; ++k) o[3 + k] = hs[k];
#pragma unroll
    for (int k = 0; k < 7; ++k) o[9 + k] = hland[k];
  }
#endif
}
#undef H3STAMP



// ----------------------------------------------------------------------------------------
// 4x4 / stride-2 / pad-1 convs (Downsample, video_net.py:61-62) and their transposes (Upsample, :65-66;
// each is also the other's data gradient) as halo-tiled implicit GEMMs on the low-resolution grid.  Both
// are 3x3 stride-1 neighbourhoods in which only a 2x2 subset of the taps is live per parity:
//   DOWN  y[oy][ox] = sum_{ky,kx} W[ky*4+kx] . x[2oy-1+ky][2ox-1+kx]; split by the input parity (a, b)
//         (x_ab[Y][X] = x[2Y+a][2X+b]) the live taps are ky = (1-a) + 2t (t = 0, 1), read at halo row
//         offset (1-a) + t of the (TH+2) x (TW+2) halo of x_ab around the output tile;
//   UP    the transposed conv in its gather form (S = 1, U = 2, P = 2, taps flipped by the packing):
//         y[2Y+py][2X+px] = sum over ky = py + 2t, kx = px + 2u of W[ky*4+kx] . x[Y-1+py+t][X-1+px+u].
// The tap base (1-a or py) is a template parameter of the per-stage MFMA loop, so every LDS address stays
// compile-time + lane constant as in conv3x3_bf16_kernel (same 2 x 2 wave tiling, 64 co per block, two
// blocks per CU).  DOWN runs 4 parity stages per 32-channel chunk (consecutive stages touch the same input
// lines); UP gives each output parity its own blocks (blockIdx.z = parity * Cout/64 + co block).  The
// generic implicit GEMM it replaces gathered every (pixel, tap) pair from global memory, 16 K-steps of 8
// MFMAs per wave per chunk (190-260 TF/s on the bench shapes).
// ----------------------------------------------------------------------------------------
template <int TW, int BY, int BX>
__device__ __forceinline__ void s2_taps(const bf16* sh, const bf16* sw, const int (&boff)[8][3], const int (&aoff)[2],
                                        f32x4 (&acc)[2][8]) {
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int oy = BY + (t >> 1), ox = BX + (t & 1);
    bf16x8 af[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) af[i] = *reinterpret_cast<const bf16x8*>(sw + aoff[i] + t * H3_BN * H3_LD);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const bf16x8 bfr = *reinterpret_cast<const bf16x8*>(sh + boff[j][ox] + oy * H3_P * H3_LD);
      acc[0][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[0], bfr, acc[0][j], 0, 0, 0);
      acc[1][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[1], bfr, acc[1][j], 0, 0, 0);
    }
  }
}
template <int TW, int BY, int BX>
__device__ __forceinline__ void s2_taps_pipe(const bf16* sh, const bf16* sw, const int (&boff)[8][3], const int (&aoff)[2],
                                        f32x4 (&acc)[2][8]) {
  // tap t+1's 10 fragment reads issued between tap t's 16 MFMAs (as conv3x3_bf16_kernel)
  bf16x8 fa[2][2], fb[2][8];
  auto rd = [&](int t, int b) {
    const int oy = BY + (t >> 1), ox = BX + (t & 1);
#pragma unroll
    for (int i = 0; i < 2; ++i) fa[b][i] = *reinterpret_cast<const bf16x8*>(sw + aoff[i] + t * H3_BN * H3_LD);
#pragma unroll
    for (int j = 0; j < 8; ++j) fb[b][j] = *reinterpret_cast<const bf16x8*>(sh + boff[j][ox] + oy * H3_P * H3_LD);
  };
  rd(0, 0);
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int b = t & 1;
    __builtin_amdgcn_sched_barrier(0);
    if (t + 1 < 4) rd(t + 1, b ^ 1);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      acc[0][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[b][0], fb[b][j], acc[0][j], 0, 0, 0);
      acc[1][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[b][1], fb[b][j], acc[1][j], 0, 0, 0);
    }
    if (t + 1 < 4) {
#pragma unroll
      for (int q2 = 0; q2 < 10; ++q2) {
        __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);  // 1 DS read
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);  // 1 MFMA
      }
      __builtin_amdgcn_sched_group_barrier(0x008, 6, 0);
    }
    __builtin_amdgcn_sched_barrier(0);
  }
}

template <int TW, bool UP>
__global__ __launch_bounds__(256, 2) void convs2_bf16_kernel(const bf16* __restrict__ x, const bf16* __restrict__ w,
                                                             const float* __restrict__ bias, const bf16* __restrict__ res,
                                                             bf16* __restrict__ y, ConvGeom g, int tiles_x, int TH,
                                                             int Hl, int Wl) {
  __shared__ __attribute__((aligned(16))) bf16 sh[H3_NROW * H3_LD];
  __shared__ __attribute__((aligned(16))) bf16 sw[4 * H3_BN * H3_LD];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int wr = wid >> 1, wc = wid & 1;
  const int n = blockIdx.y;
  const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
  const int y0 = ty * TH, x0 = tx * TW;  // tile origin on the low-resolution grid
  constexpr int HWd = TW + 2;
  const int ncob = g.Cout / H3_BN;
  const int par = UP ? (int)blockIdx.z / ncob : 0;
  const int n0 = ((int)blockIdx.z - par * ncob) * H3_BN;
  const int ppy = par >> 1, ppx = par & 1;
  const int Cin = g.C1;
  const int nchunk = Cin / 32;
  constexpr int WPT = 4 * H3_BN * 4 / 256;  // weight vectors per thread (4 taps x 64 co x 4 vectors)

  // stage s by buffer-LDS-DMA (as conv3x3_bf16_kernel): halo of the (parity sub-)image and the 4 live taps'
  // weights for one 32-channel chunk
  (void)WPT;
  const __amdgpu_buffer_rsrc_t xrs = __builtin_amdgcn_make_buffer_rsrc(
      (void*)(x + (int64_t)n * g.Hi * g.Wi * Cin), (short)0, (int)((int64_t)g.Hi * g.Wi * Cin * 2), 0x00020000);
  const __amdgpu_buffer_rsrc_t wrs = __builtin_amdgcn_make_buffer_rsrc(
      (void*)(w + (int64_t)n0 * 16 * Cin), (short)0, H3_BN * 16 * Cin * 2, 0x00020000);
  auto stage = [&](int ch, int a, int b, int by, int bx) {
    const int c0 = ch * 32;
    const int prow = lane >> 2, pslot = lane & 3;
    constexpr int HPC = H3_NROW / 16;
#pragma unroll
    for (int k = 0; k < (HPC + 3) / 4; ++k) {
      const int q = wid + 4 * k;
      if (q < HPC) {  // wave-uniform
        const int row = 16 * q + prow;
        const int r = row / H3_P, col = row - r * H3_P;
        const int Y = y0 - 1 + r, X = x0 - 1 + col;
        const int iy = UP ? Y : 2 * Y + a, ix = UP ? X : 2 * X + b;
        const bool in = r < TH + 2 && col < HWd && (unsigned)iy < (unsigned)g.Hi && (unsigned)ix < (unsigned)g.Wi;
        const int chunk = pslot ^ ((row >> 1) & 2);
        const int vo = in ? ((iy * g.Wi + ix) * Cin + c0 + chunk * 8) * 2 : 0x7ffffff0;
        __builtin_amdgcn_raw_ptr_buffer_load_lds(xrs, (__attribute__((address_space(3))) void*)(sh + q * 512), 16, vo, 0,
                                                 0, 0);
      }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {  // 4 taps x 64 co rows = 16 pieces
      const int q = wid + 4 * k, row = 16 * q + prow;  // row = t * 64 + co
      const int t = row >> 6, co = row & 63;
      const int tap = (by + 2 * (t >> 1)) * 4 + bx + 2 * (t & 1);
      const int chunk = pslot ^ ((row >> 1) & 2);
      __builtin_amdgcn_raw_ptr_buffer_load_lds(wrs, (__attribute__((address_space(3))) void*)(sw + q * 512), 16,
                                               (((ch * 16 + tap) * 64 + co) * 32 + chunk * 8) * 2, 0, 0, 0);  // chunked
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  };

  f32x4 acc[2][8];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int lr = lane & 15, lg = lane >> 4;
  int hoff[8], pyx[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int p = wc * 128 + j * 16 + lr;
    const int py = p / TW, px = p - py * TW;
    const bool in = py < TH;
    hoff[j] = in ? py * H3_P + px : 0;
    pyx[j] = in ? (py << 16) | px : -1;
  }
  int boff[8][3], aoff[2];
#pragma unroll
  for (int j = 0; j < 8; ++j)
#pragma unroll
    for (int kx = 0; kx < 3; ++kx) boff[j][kx] = h3_off(hoff[j] + kx, lg);
#pragma unroll
  for (int i = 0; i < 2; ++i) aoff[i] = h3_off(wr * 32 + i * 16 + lr, lg);

  if constexpr (UP) {
    for (int ch = 0; ch < nchunk; ++ch) {
      if (ch) __syncthreads();  // previous chunk fully consumed
      stage(ch, 0, 0, ppy, ppx);
      __syncthreads();
      switch (par) {  // block-uniform
        case 0: s2_taps<TW, 0, 0>(sh, sw, boff, aoff, acc); break;
        case 1: s2_taps<TW, 0, 1>(sh, sw, boff, aoff, acc); break;
        case 2: s2_taps<TW, 1, 0>(sh, sw, boff, aoff, acc); break;
        default: s2_taps<TW, 1, 1>(sh, sw, boff, aoff, acc); break;
      }
    }
  } else {
    for (int ch = 0; ch < nchunk; ++ch) {
#pragma unroll
      for (int ab = 0; ab < 4; ++ab) {
        const int a = ab >> 1, b = ab & 1;
        if (ch || ab) __syncthreads();
        stage(ch, a, b, 1 - a, 1 - b);
        __syncthreads();
        // (down: the software-pipelined taps; the up kernel keeps the plain loop, pipelined it spills)
        if (ab == 0) s2_taps_pipe<TW, 1, 1>(sh, sw, boff, aoff, acc);       // a = 0, b = 0
        else if (ab == 1) s2_taps_pipe<TW, 1, 0>(sh, sw, boff, aoff, acc);  // a = 0, b = 1
        else if (ab == 2) s2_taps_pipe<TW, 0, 1>(sh, sw, boff, aoff, acc);  // a = 1, b = 0
        else s2_taps_pipe<TW, 0, 0>(sh, sw, boff, aoff, acc);                // a = 1, b = 1
      }
    }
  }
  // epilogue: lane holds co = n0 + wr*32 + i*16 + 4*lg + r of tile pixel (py, px)
  float bv[2][4];
#pragma unroll
  for (int i = 0; i < 2; ++i) epi_bias(bias, n0 + wr * 32 + i * 16 + lg * 4, bv[i]);
  int64_t mj[8];
  bool okj[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int Y = y0 + (pyx[j] >> 16), X = x0 + (pyx[j] & 0xffff);
    okj[j] = pyx[j] >= 0 && Y < Hl && X < Wl;
    const int oy = UP ? 2 * Y + ppy : Y, ox = UP ? 2 * X + ppx : X;
    mj[j] = okj[j] ? ((int64_t)n * g.Ho + oy) * g.Wo + ox : 0;
  }
  bf16x4 rv[8][2];
  if (res) {  // uniform
#pragma unroll
    for (int j = 0; j < 8; ++j)
#pragma unroll
      for (int i = 0; i < 2; ++i) rv[j][i] = epi_res(res, nullptr, mj[j], n0 + wr * 32 + i * 16 + lg * 4, g.Cout, 0, okj[j]);
  } else {
#pragma unroll
    for (int j = 0; j < 8; ++j)
#pragma unroll
      for (int i = 0; i < 2; ++i) rv[j][i] = bf16x4{};
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    if (!okj[j]) continue;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int co = n0 + wr * 32 + i * 16 + lg * 4;
      float v[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) v[r] = acc[i][j][r] + bv[i][r] + b2f(rv[j][i], r);
      store4(y + mj[j] * g.Cout + co, v);
    }
  }
}

}  // namespace

void conv_halo3_launch(const ConvLaunchArgs& a) {
  const ConvGeom g = conv_geom(a);
  const int Nb = a.Nb, Ho = a.Ho, Wo = a.Wo, Cout = a.Cout, TH = a.TH, TW = a.TW;
  const int tx = (int)cdiv(Wo, TW), ty = (int)cdiv(Ho, TH);
  const unsigned g3 = (unsigned)(Cout / H3_BN) * 8u * (unsigned)cdiv((int64_t)tx * ty * Nb, 8);
  const bool big = TH * TW > 256;  // h3_big_tile chose a 448-pixel tile
#define H3L(TWv, NJv)                                                                                           \
  conv3x3_bf16_kernel<TWv, NJv><<<g3, 256, 0, a.stream>>>(a.x1, a.x2, a.wp, a.bias, a.res, a.res2, a.y1, a.y2, g, tx, \
                                                          TH, a.gnp, a.gn_fimg)
  if (TW == 36) { if (big) H3L(36, 7); else H3L(36, 4); }
  else { if (big) H3L(32, 7); else H3L(32, 4); }
#undef H3L
}

void conv_s2_launch(const ConvLaunchArgs& a) {
  const ConvGeom g = conv_geom(a);
  const int Nb = a.Nb, Hi = a.Hi, Wi = a.Wi, Ho = a.Ho, Wo = a.Wo, Cout = a.Cout, TH = a.TH, TW = a.TW;
  const bool up = a.U == 2;  // the transposed conv in its gather form
  const int Hl = up ? Hi : Ho, Wl = up ? Wi : Wo;
  const int tx = (int)cdiv(Wl, TW), ty = (int)cdiv(Hl, TH);
  dim3 g3(tx * ty, Nb, (Cout / H3_BN) * (up ? 4 : 1));
  if (!up && TW == 36)
    convs2_bf16_kernel<36, false><<<g3, 256, 0, a.stream>>>(a.x1, a.wp, a.bias, a.res, a.y1, g, tx, TH, Hl, Wl);
  else if (!up)
    convs2_bf16_kernel<32, false><<<g3, 256, 0, a.stream>>>(a.x1, a.wp, a.bias, a.res, a.y1, g, tx, TH, Hl, Wl);
  else if (TW == 36)
    convs2_bf16_kernel<36, true><<<g3, 256, 0, a.stream>>>(a.x1, a.wp, a.bias, a.res, a.y1, g, tx, TH, Hl, Wl);
  else
    convs2_bf16_kernel<32, true><<<g3, 256, 0, a.stream>>>(a.x1, a.wp, a.bias, a.res, a.y1, g, tx, TH, Hl, Wl);
}

#ifdef CESM_H3_STAMPS
// diagnostic build only (tools/h3_stamps.py): point the halo conv's phase stamps at buf (16 u64 per wave, 4 waves per
// block, blocks [0, nblocks)); buf = nullptr turns them off
extern "C" int cesm_diag_h3_stamps_set(void* buf, int nblocks) {
  uint64_t* p = static_cast<uint64_t*>(buf);
  if (hipMemcpyToSymbol(HIP_SYMBOL(g_h3_stamp_buf), &p, sizeof(p)) != hipSuccess) return CESM_EINVAL;
  if (hipMemcpyToSymbol(HIP_SYMBOL(g_h3_stamp_blocks), &nblocks, sizeof(nblocks)) != hipSuccess) return CESM_EINVAL;
  return 0;
}
#endif
