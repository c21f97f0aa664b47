// The two persistent 3x3 / stride-1 convs of level 0 (bf16, 64 output channels per item): conv3x3p_kernel (resident
// weights, Cin = Cout = 64) and the warp-specialized conv3x3ws_kernel, with their launchers.  conv_fwd_plan (conv_fwd.hip)
// decides when they run and with which tile; conv_fwd_launch calls conv_p32_launch / conv_ws_launch below.
#include "conv_common.h"

namespace {

// ----------------------------------------------------------------------------------------
// LDS image of the persistent 3x3 convs (conv3x3p_kernel, conv3x3ws_kernel): halo and weight tiles of one 32-channel
// chunk in 64-B rows, staged by LDS-DMA in 1-KiB pieces of 16 rows; the 16-B chunk index of a row is XORed with
// (row >> 1) & 2 -- conflict-free for ds_read_b128 over any 16 consecutive rows.
// ----------------------------------------------------------------------------------------
constexpr int CW_HROWS = 640;                       // max halo rows (TH+2)(TW+2)
constexpr int CW_WROWS = 9 * 64;                    // weight rows (tap*64 + co)
constexpr int CW_HPIECE = CW_HROWS / 16;            // 1-KiB glds pieces
constexpr int CW_WPIECE = CW_WROWS / 16;
constexpr int CW_HPW = CW_HPIECE / 4;               // halo pieces per wave (10)
constexpr int CW_WPW = CW_WPIECE / 4;               // weight pieces per wave (9)

__device__ __forceinline__ int cw_swz(int row) { return (row >> 1) & 2; }
// byte offset of 16-B chunk c (8 channels) of row `row`
__device__ __forceinline__ int cw_off(int row, int c) { return (row << 6) + ((c ^ cw_swz(row)) << 4); }

// ----------------------------------------------------------------------------------------
// persistent 3x3 conv (conv3x3p_kernel) and the tap routine it shares with the warp-specialized conv
// ----------------------------------------------------------------------------------------
constexpr int CP_ELD = 68;                            // epilogue tile row (bf16): 136 B, conflict-free 8-B writes
constexpr int CP_PITCH = 40;                          // halo row pitch (pixels): multiple of 8
// (CP_TH = 14, the max tile rows -- (14 + 2) * 40 = 640 halo rows: conv_common.h)

// taps of one staged chunk for NG fragment groups per wave.  Halo rows use a pitch of 40 pixels, so a
// ky step (+40 rows) keeps bits 0..2 of the row and with them the chunk swizzle: the B address of
// (group j, ky, kx) = bad[j][kx] + ky * 40 * 64 -> immediate offsets, no per-read VALU.  Fragment reads
// of tap t+1 are interleaved with tap t's MFMAs (sched_group_barrier: 1 ds_read, 2 MFMA, ...).
struct NoHook {
  __device__ __forceinline__ void operator()(int) const {}
};

template <int NG, typename Hook = NoHook>
__device__ __forceinline__ void cp_taps(const char* sh, const char* sw, const int (&bad)[NG][3], int a_lane,
                                        f32x4 (&acc)[4][NG], const Hook& hook = Hook()) {
  bf16x8 af[2][4], bfr[2][NG];
  auto load = [&](int tap, int b) {
    const int ky = tap / 3, kx = tap - ky * 3;
#pragma unroll
    for (int i = 0; i < 4; ++i) af[b][i] = *reinterpret_cast<const bf16x8*>(sw + a_lane + (tap * 64 + i * 16) * 64);
#pragma unroll
    for (int j = 0; j < NG; ++j)
      bfr[b][j] = *reinterpret_cast<const bf16x8*>(sh + bad[j][kx] + ky * CP_PITCH * 64);
  };
  load(0, 0);
#pragma unroll
  for (int tap = 0; tap < 9; ++tap) {
    const int b = tap & 1;
    __builtin_amdgcn_sched_barrier(0);
    hook(tap);  // e.g. this tap's share of the next step's LDS-DMA, spread over the MFMA phase
    __builtin_amdgcn_sched_barrier(0);
    if (tap + 1 < 9) load(tap + 1, b ^ 1);
#pragma unroll
    for (int j = 0; j < NG; ++j)
#pragma unroll
      for (int i = 0; i < 4; ++i) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[b][i], bfr[b][j], acc[i][j], 0, 0, 0);
    if (tap + 1 < 9) {
#pragma unroll
      for (int q = 0; q < 4 + NG; ++q) {
        __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);  // 1 DS read
        __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);  // 2 MFMA
      }
      __builtin_amdgcn_sched_group_barrier(0x008, 4 * NG - 2 * (4 + NG), 0);
    }
    __builtin_amdgcn_sched_barrier(0);
  }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
}

// ----------------------------------------------------------------------------------------
// 3x3 conv (bf16), v4 "pipelined wide wave": persistent (one block per CU) with TWO LDS stages:
// the buffer-LDS-DMA of step s+1 (next 32-channel chunk, or the next item's first chunk) is issued
// right after the barrier that opens step s and lands while step s's MFMAs run.  Steps run over
// the block's items (it = blockIdx.x + k * gridDim.x; item = (image, TH x TW tile, 64-channel co
// block), co block fastest so a tile's co blocks run concurrently and share its halo in L2).
// Wave w owns tile pixels [16*NG*w, 16*NG*(w+1)) x all 64 co.  The epilogue stages (acc + bias) as
// bf16 in the stage just consumed and writes full 128-B pixel rows (+ residual) with exactly 2*NG
// buffer stores per wave, so the next step waits for its DMA with vmcnt(2*NG), not for the stores.
// ----------------------------------------------------------------------------------------
// Items are split statically (item it = blockIdx.x + k * gridDim.x): the kernel keeps no state between launches,
// so concurrent launches (two streams, graph branches, two model instances) are independent.  (Round 3 claimed
// items from a process-global atomic counter instead: 596.6 vs 599.1 us per launch, not worth the hidden state.)

template <int TW>
__global__ __launch_bounds__(256, 1) void conv3x3p_kernel(const bf16* __restrict__ x1, const bf16* __restrict__ x2,
                                                          const bf16* __restrict__ w, const float* __restrict__ bias,
                                                          const bf16* __restrict__ res, const bf16* __restrict__ res2,
                                                          bf16* __restrict__ y1, bf16* __restrict__ y2, ConvGeom g,
                                                          int tiles_x, int tiles_per_img, int TH, int ncob, int nitems,
                                                          float* __restrict__ gnp, int gn_fimg) {
  constexpr int NG = 7;  // fragment groups of 16 pixels per wave: 4 waves x 7 x 16 = 448 = CP_TH x 32 pixels
  static_assert(TW + 2 <= CP_PITCH && 2 * NG == 14, "tile geometry; the vmcnt(14) / vmcnt(18) waits count 2*NG stores");
  // one LDS array (a second __shared__ object can make hipcc drain the DMA before ds_reads):
  // 2 stages | resident weights, both chunks | bias [Cout = 64] fp32.  Cin = Cout = 64: a stage holds only the
  // halo and the 2 x 36 KiB weight chunks are loaded once per block
  constexpr int NST = 2, HPW = CW_HPW;
  constexpr int STG = HPW * 4 * 1024;
  constexpr int WRES = 2 * CW_WROWS * 64;
  constexpr int BIASB = 256;
  __shared__ __attribute__((aligned(1024))) char lds[NST * STG + WRES + BIASB + 16];
  char* wres = lds + NST * STG;
  float* sbias = reinterpret_cast<float*>(lds + NST * STG + WRES);
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int lr = lane & 15, lg = lane >> 4;
  const int HP = (TH + 2) * CP_PITCH;
  for (int c = tid; c < g.Cout; c += 256) sbias[c] = bias ? bias[c] : 0.f;
  const int hpieces = (HP + 15) >> 4;
  const int Cin = g.C1 + g.C2;
  const int nchunk = Cin / 32;
  const int prow = lane >> 2, pslot = lane & 3;
  const int nmine = nitems > (int)blockIdx.x ? (nitems - 1 - (int)blockIdx.x) / (int)gridDim.x + 1 : 0;
  const int nsteps = nmine * nchunk;

  // per-lane halo row -> tile-relative (hy, hx) of piece k (item independent); -1: zero row
  int hrel[HPW];
#pragma unroll
  for (int k = 0; k < HPW; ++k) {
    const int row = 16 * (wid + 4 * k) + prow;
    const int hy = row / CP_PITCH, hx = row - (row / CP_PITCH) * CP_PITCH;
    hrel[k] = (row < HP && hx < TW + 2) ? (hy << 16) | hx : -1;
  }
  // B-fragment addresses of tap (0, kx) per group; A lane constant
  int bad[NG][3];
#pragma unroll
  for (int j = 0; j < NG; ++j) {
    const int p = wid * 16 * NG + j * 16 + lr;
    const int h0 = p < TH * TW ? (p / TW) * CP_PITCH + (p - (p / TW) * TW) : 0;
#pragma unroll
    for (int kx = 0; kx < 3; ++kx) bad[j][kx] = cw_off(h0 + kx, lg);
  }
  const int a_lane = (lr << 6) + ((lg ^ cw_swz(lr)) << 4);

  auto item_geo = [&](int it, int& n, int& y0, int& x0, int& cob) {
    cob = it % ncob;
    const int t = it / ncob;
    n = t / tiles_per_img;
    const int r = t - n * tiles_per_img;
    const int ty = r / tiles_x;
    y0 = ty * TH;
    x0 = (r - ty * tiles_x) * TW;
  };
  // LDS-DMA of step s, piece by piece (halo pieces only: the weights are resident).
  // Source descriptor of the step being prefetched (set by step_src):
  __amdgpu_buffer_rsrc_t dxrs;
  int dcs = 0, dy0 = 0, dx0 = 0;
  char* dsh = lds;
  auto step_src = [&](int s, int it, int ch) {
    int n, cob;
    item_geo(it, n, dy0, dx0, cob);
    const int c0 = ch * 32;
    const bf16* src;
    int cc;
    if (c0 < g.C1) { src = x1; dcs = g.C1; cc = c0; } else { src = x2; dcs = g.C2; cc = c0 - g.C1; }
    const int64_t img_elems = (int64_t)g.Hi * g.Wi * dcs;
    dxrs = __builtin_amdgcn_make_buffer_rsrc((void*)(src + (int64_t)n * img_elems + cc), (short)0,
                                             (int)(img_elems * 2 - cc * 2), 0x00020000);
    dsh = lds + (s % NST) * STG;
  };
  auto issue_piece = [&](int k) {
    const int q = wid + 4 * k;
    if (q < hpieces) {  // wave-uniform
      const int chunk = pslot ^ cw_swz(16 * q + prow);
      const int iy = dy0 - 1 + (hrel[k] >> 16), ix = dx0 - 1 + (hrel[k] & 0xffff);
      const bool in = hrel[k] >= 0 && (unsigned)iy < (unsigned)g.Hi && (unsigned)ix < (unsigned)g.Wi;
      const int vo = in ? ((iy * g.Wi + ix) * dcs + chunk * 8) * 2 : 0x7ffffff0;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(dxrs, (__attribute__((address_space(3))) void*)(dsh + q * 1024), 16,
                                               vo, 0, 0, 0);
    }
  };
  constexpr int NPIECE = HPW;  // per wave per step
  auto issue = [&](int s, int it, int ch) {
    step_src(s, it, ch);
#pragma unroll
    for (int k = 0; k < NPIECE; ++k) issue_piece(k);
  };
  {  // the whole (64 co x 9 taps x 64 ci) weight, chunk-major, waited for by step 0
    const __amdgpu_buffer_rsrc_t wrs0 = __builtin_amdgcn_make_buffer_rsrc((void*)w, (short)0, 64 * 9 * 64 * 2, 0x00020000);
#pragma unroll
    for (int ch = 0; ch < 2; ++ch)
#pragma unroll
      for (int k = 0; k < CW_WPW; ++k) {
        const int q = wid + 4 * k;
        const int row = 16 * q + prow;
        const int chunk = pslot ^ cw_swz(row);
        const int vo = (ch * 9 * 64 * 32 + row * 32 + chunk * 8) * 2;  // chunked pack (wpk_index)
        __builtin_amdgcn_raw_ptr_buffer_load_lds(
            wrs0, (__attribute__((address_space(3))) void*)(wres + ch * CW_WROWS * 64 + q * 1024), 16, vo, 0, 0, 0);
      }
  }

#pragma unroll
  for (int q = 0; q < NST - 1; ++q)
    if (q < nsteps) issue(q, (int)blockIdx.x + (q / nchunk) * (int)gridDim.x, q % nchunk);
  int s = 0;
  bool epi = false;
  int it = (int)blockIdx.x;
  for (int k = 0; it < nitems; ++k) {
    (void)k;  // unused, but a plain `while` compiles to different code (register allocation, two instructions)
    const int nxt = it + (int)gridDim.x;
    f32x4 acc[4][NG];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < NG; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int ch = 0; ch < nchunk; ++ch, ++s) {
      // step s landed: after an epilogue only its 2*NG stores are younger than step s's DMA
      if (epi) {
        // younger than step s's DMA: the epilogue's 2*NG output stores (+ 4 GroupNorm partial stores)
        if (gnp) asm volatile("s_waitcnt vmcnt(18)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(14)" ::: "memory");
      } else {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      }
      epi = false;
      __builtin_amdgcn_s_barrier();                     // ... for every wave; step s-1's reads are done
      const char* sh = lds + (s % NST) * STG;
      const char* sw = wres + ch * CW_WROWS * 64;
      const int sp = s + NST - 1;  // step prefetched now, into the stage step s-1 used
      // its item / chunk: the next chunk of this item, or the next item's first chunk
      const int sp_it = ch + 1 < nchunk ? it : nxt;
      const int sp_ch = ch + 1 < nchunk ? ch + 1 : 0;
      const bool pf = sp_it < nitems;
      // the prefetch DMA spread over this step's taps (issuing all of it up front stalls the wave on the
      // vector-memory queue before its first MFMA).  ONE tap loop for both cases (pf is a uniform branch inside
      // the hook): with a second, hook-less copy of the loop the compiler gave the two copies different
      // accumulator registers and copied all 112 of them AGPR -> VGPR -> AGPR at every step (224 v_accvgpr
      // moves per 252 MFMAs)
      if (pf) step_src(sp, sp_it, sp_ch);
      auto hook = [&](int tap) {
        if (pf) {
#pragma unroll
          for (int k = 0; k < NPIECE; ++k)
            if (k * 9 / NPIECE == tap) issue_piece(k);
        }
      };
      cp_taps<NG>(sh, sw, bad, a_lane, acc, hook);
    }
    int n, y0, x0, cob;
    item_geo(it, n, y0, x0, cob);
    const int n0 = cob * 64;
    it = nxt;
    // epilogue through LDS, wave-private, in rounds of up to 4 fragment groups (64 px): (acc + bias)
    // -> bf16 rows [64 px][CP_ELD] in this wave's slice of the stage just consumed (barrier: every wave
    // is past its taps), then 8 lanes per pixel write full 128-B rows with 16-B buffer stores (+
    // residual read the same way); exactly 2*NG stores per wave (rows outside the image -> out-of-range
    // offset, dropped) so the next step waits for its DMA with vmcnt(2*NG), not for these stores
    __builtin_amdgcn_s_barrier();
    constexpr int RG = (4 * 16 * CP_ELD * 2 * 4 <= STG) ? 4 : 2;  // groups per epilogue round (fits the stage)
    bf16* so = reinterpret_cast<bf16*>(lds + ((s - 1) % NST) * STG) + wid * RG * 16 * CP_ELD;
    const bool first = n0 < g.Co1;
    const int cstride = first ? g.Co1 : g.Cout - g.Co1;
    const int cofs = (first ? n0 : n0 - g.Co1) + (lane & 7) * 8;
    const int64_t img = (int64_t)n * g.Ho * g.Wo * cstride;
    const int img_bytes = g.Ho * g.Wo * cstride * 2;
    const __amdgpu_buffer_rsrc_t yrs =
        __builtin_amdgcn_make_buffer_rsrc((void*)((first ? y1 : y2) + img), (short)0, img_bytes, 0x00020000);
    const bf16* rsrc = first ? res : res2;
    const __amdgpu_buffer_rsrc_t rrs =
        __builtin_amdgcn_make_buffer_rsrc((void*)((rsrc ? rsrc : y1) + img), (short)0, img_bytes, 0x00020000);
    // GroupNorm statistics partials of this wave's pixels (gnp: the Block conv feeding a GroupNorm):
    // per channel quad (i, lg) the sum and sum of squares of bf16(acc + bias) over the valid pixels
    float gsum[4] = {0.f, 0.f, 0.f, 0.f}, gsq[4] = {0.f, 0.f, 0.f, 0.f};
    float gm[NG];
#pragma unroll
    for (int j = 0; j < NG; ++j) {
      const int p = wid * 16 * NG + j * 16 + lr;
      const int oy = y0 + p / TW, ox = x0 + (p - (p / TW) * TW);
      gm[j] = (p < TH * TW && oy < g.Ho && ox < g.Wo) ? 1.f : 0.f;
    }
#pragma unroll
    for (int r0 = 0; r0 < NG; r0 += RG) {
      const int nj = NG - r0 < RG ? NG - r0 : RG;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int co = i * 16 + lg * 4;
        const f32x4 bv = *reinterpret_cast<const f32x4*>(sbias + n0 + co);
#pragma unroll
        for (int jj = 0; jj < RG; ++jj) {
          if (jj < nj) {
            const int j = r0 + jj;
            float v[4] = {acc[i][j][0] + bv[0], acc[i][j][1] + bv[1], acc[i][j][2] + bv[2], acc[i][j][3] + bv[3]};
            store4(so + (jj * 16 + lr) * CP_ELD + co, v);
            if (gnp) {  // uniform; statistics of the stored (bf16-rounded) y, which GroupNorm then normalises
#pragma unroll
              for (int r = 0; r < 4; ++r) v[r] = (float)(bf16)v[r];
              const float sv = (v[0] + v[1]) + (v[2] + v[3]);
              const float qv = fmaf(v[3], v[3], fmaf(v[2], v[2], fmaf(v[1], v[1], v[0] * v[0])));
              gsum[i] = fmaf(gm[j], sv, gsum[i]);
              gsq[i] = fmaf(gm[j], qv, gsq[i]);
            }
          }
        }
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // own writes visible to the wave's other lanes
      // residual rows of the round in batches of CP_RB loads issued back to back (one load -> wait ->
      // add -> store chain per row made the residual-fused dgrads 1.7x slower than the plain ones);
      // the plain path keeps its own loop (uniform branch)
      constexpr int CP_RB = 4;
      if (!rsrc) {
        // all rows of the round read from LDS first, then stored (one ds_read -> wait -> store chain per row
        // exposed the LDS latency 14 times per item)
        bf16x8 rows[2 * RG];
#pragma unroll
        for (int u = 0; u < 2 * RG; ++u)
          if (u < 2 * nj) rows[u] = *reinterpret_cast<const bf16x8*>(so + (u * 8 + (lane >> 3)) * CP_ELD + (lane & 7) * 8);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int u = 0; u < 2 * RG; ++u) {
          if (u < 2 * nj) {
            const int pl = u * 8 + (lane >> 3);  // row of the round
            const int p = wid * 16 * NG + r0 * 16 + pl;
            const int oy = y0 + p / TW, ox = x0 + (p - (p / TW) * TW);
            const bool ok = p < TH * TW && oy < g.Ho && ox < g.Wo;
            const int off = (ok ? oy * g.Wo + ox : 0) * cstride + cofs;
            __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, rows[u]), yrs,
                                                   ok ? off * 2 : 0x7ffffff0, 0, 0);
          }
        }
      } else {
#pragma unroll
      for (int u0 = 0; u0 < 2 * RG; u0 += CP_RB) {
        int offs[CP_RB];
        bool oks[CP_RB];
        bf16x8 rv[CP_RB];
#pragma unroll
        for (int uu = 0; uu < CP_RB; ++uu) {
          const int u = u0 + uu;
          const int pl = u * 8 + (lane >> 3);  // row of the round
          const int p = wid * 16 * NG + r0 * 16 + pl;
          const int oy = y0 + p / TW, ox = x0 + (p - (p / TW) * TW);
          oks[uu] = u < 2 * nj && p < TH * TW && oy < g.Ho && ox < g.Wo;
          offs[uu] = (oks[uu] ? oy * g.Wo + ox : 0) * cstride + cofs;
          if (u < 2 * nj)
            rv[uu] = __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(rrs, offs[uu] * 2, 0, 0));
        }
        bf16x8 rows[CP_RB];
#pragma unroll
        for (int uu = 0; uu < CP_RB; ++uu)
          if (u0 + uu < 2 * nj) rows[uu] = *reinterpret_cast<const bf16x8*>(so + ((u0 + uu) * 8 + (lane >> 3)) * CP_ELD + (lane & 7) * 8);
#pragma unroll
        for (int uu = 0; uu < CP_RB; ++uu) {
          const int u = u0 + uu;
          if (u < 2 * nj) {
            bf16x8 v = rows[uu];
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] = (bf16)((float)v[e] + (float)rv[uu][e]);
            __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), yrs, oks[uu] ? offs[uu] * 2 : 0x7ffffff0,
                                                   0, 0);
          }
        }
      }
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // reads done before the next round overwrites
    }
    if (gnp) {  // after the output stores: exactly 4 more stores (the next step's vmcnt counts them)
      const int b = n / gn_fimg, f = n - b * gn_fimg;
      const int64_t nslot = (int64_t)gn_fimg * tiles_per_img * 4;
      const int64_t slot = ((int64_t)f * tiles_per_img + (y0 / TH) * tiles_x + x0 / TW) * 4 + wid;
      float2* dst = reinterpret_cast<float2*>(gnp) + ((int64_t)b * nslot + slot) * (g.Cout / 4) + n0 / 4 + lg;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float a = row16_sum(gsum[i]), q = row16_sum(gsq[i]);
        if (lr == 0) dst[i * 4] = make_float2(a, q);
      }
    }
    epi = true;
  }
}

// ----------------------------------------------------------------------------------------
// 3x3 / stride 1 / pad 1 conv (bf16), warp-specialized persistent kernel (round 4).  One block of 8 waves per CU
// (two per SIMD), static item split (item = (image, TH x TW tile of <= 256 px, 64-channel co block), the co blocks
// of a tile on blocks of one XCD):
//   waves 0-3 (compute): 64 co x 64 px each (4 x 4 MFMA tiles), the 9 taps of a 32-channel chunk from a halo +
//     weight stage in LDS (cp_taps: tap t+1's 8 fragment reads between tap t's 16 MFMAs); at an item's last chunk
//     they add the bias and write bf16 rows into a staging tile, and go straight on with the next item;
//   waves 4-7 (load / store): the buffer-LDS-DMA of the next step's stage while the compute waves consume the
//     current one, and the epilogue of the previous item from the staging tile -- residual (prefetched a step
//     ahead), GroupNorm partials, 16-B row stores.
// One s_barrier per step hands the stages over; the compute waves never wait on a load or a store, and the
// epilogue (~40 % of conv3x3p's time at one wave per SIMD, where it could not overlap the MFMAs) runs beside the next
// item's MFMAs.  Both roles pass exactly the same barriers.  LDS: 2 stages x 61 KiB + a 34 KiB staging tile.
// ----------------------------------------------------------------------------------------
// (Round 5, removed: s_setprio for the loader or the compute waves, within the spread -- profiles/r5_prio_ab.txt.)
// (WS_MAXTH = 8 tile rows -- (8 + 2) * 40 = 400 halo rows -- and WS_PIX = 256 pixels per item, 4 waves x 4 groups of 16:
// conv_common.h)
constexpr int WS_PITCH = 40;                               // halo row pitch (pixels): ky steps keep the swizzle
constexpr int WS_HROWS = (WS_MAXTH + 2) * WS_PITCH;        // 400
constexpr int WS_WROWS = 9 * 64;                           // weight rows (tap * 64 + co)
constexpr int WS_STAGE = (WS_HROWS + WS_WROWS) * 64;       // 62,464 B
constexpr int WS_ELD = 68;                                 // staging row (bf16): 136 B, conflict-free 8-B writes
constexpr int WS_LDS = 2 * WS_STAGE + WS_PIX * WS_ELD * 2;  // 159,744 B
static_assert(WS_LDS + 1024 <= 160 * 1024, "warp-specialized conv LDS");
static_assert(2 * WS_WROWS * 64 + 2 * WS_HROWS * 64 == 2 * WS_STAGE, "resident-weight layout = the two stages");
constexpr int WS_HPMAX = (WS_HROWS / 16 + 3) / 4;          // halo pieces per loader wave (<= 7)
constexpr int WS_WP = WS_WROWS / 16 / 4;                   // weight pieces per loader wave (9)

__device__ __forceinline__ void ws_decode(int it, int ncob, int& tile, int& cb) {
  // co blocks of a tile 8 ids apart: the blocks b, b + 8, ... that take them share an XCD (round-robin placement).
  // (Round 4: items in per-XCD runs of vertically adjacent tiles, so tiles sharing halo rows meet in one L2, measured
  // 514-516 -> 548-552 us per launch in the step, profiles/r4c15_bench_ab.txt; removed.)
  const int g = it / (8 * ncob), r = it - g * 8 * ncob;
  cb = r >> 3;
  tile = g * 8 + (r & 7);
}

template <int TW, bool GN>
__global__ __launch_bounds__(512, 1) void conv3x3ws_kernel(const bf16* __restrict__ x1, const bf16* __restrict__ x2,
                                                           const bf16* __restrict__ w, const float* __restrict__ bias,
                                                           const bf16* __restrict__ res, const bf16* __restrict__ res2,
                                                           bf16* __restrict__ y1, bf16* __restrict__ y2, ConvGeom g,
                                                           int TH, int tiles_x, int tiles_per_img, int ncob,
                                                           int nitems_pad, float* __restrict__ gnp, int gn_fimg,
                                                           int* __restrict__ queue) {
  // + the touch loads' never-read rows (1 KiB) + 3 published item ids (dynamic claiming)
  __shared__ __attribute__((aligned(1024))) char lds[WS_LDS + 1024 + 16];
  bf16* stg = reinterpret_cast<bf16*>(lds + 2 * WS_STAGE);
  int* qslot = reinterpret_cast<int*>(lds + WS_LDS + 1024);
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const bool loader = wid >= 4;  // wave-uniform role
  const int wl = wid & 3;
  const int lr = lane & 15, lg = lane >> 4;
  const int Cin = g.C1 + g.C2, nchunk = Cin / 32;
  const int ntile = g.Nb * tiles_per_img;
  const int G = (int)gridDim.x;
  // the block's valid items: it = blockIdx.x + k * G (k < nk), tile < ntile; steps = valid items x chunks
  auto next_valid = [&](int it) {
    for (; it < nitems_pad; it += G) {
      int tile, cb;
      ws_decode(it, ncob, tile, cb);
      if (tile < ntile) return it;
    }
    return nitems_pad;
  };
  // Item order.  Static (queue == null): item k of the block is the k-th valid id of blockIdx.x + j * G.  Dynamic
  // (round 5; a caller-owned counter, see cesm_conv_fwd): every item is claimed from queue[0] by one returning atomic
  // add -- a block slowed by co-running kernels (RCCL's, on the communication stream) or placed late takes fewer items
  // (none, if it starts after the queue has run dry) instead of leaving a static split's tail.  Claims run two items
  // ahead so every wave knows item k + 1 (the stage DMA, the L2 touch, the compute waves' bias and loop end) a full
  // item before it starts: loader wave 0 claims item k + 2 at item k's first step and publishes it in
  // qslot[(k + 2) % 3], which every wave reads at item k + 1's first step, a barrier later (the slot it overwrites
  // held item k - 1, read a barrier before); items 0 and 1 are claimed before a block barrier ahead of the loops.
  // The outputs do not depend on the order: an item is one block's whole 9 x Cin sum, and the GroupNorm partial slot
  // belongs to the tile.  Needs nchunk >= 2 (else the static order).  The last block to finish resets the counter,
  // so it is zero again for the next launch on the same stream.
  const bool dyn = queue != nullptr && nchunk >= 2;
  auto claim = [&]() {  // one lane; the next valid claimed id, or nitems_pad
    while (true) {
      const int it = atomicAdd(queue, 1);
      if (it >= nitems_pad) return nitems_pad;
      int tile, cb;
      ws_decode(it, ncob, tile, cb);
      if (tile < ntile) return it;
    }
  };
  auto publish = [&](int k, int val) {  // loader wave 0: item k's id into its slot (readers: after a barrier)
    if (lane == 0) qslot[k % 3] = val;
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  };
  auto finish_queue = [&]() {  // every block once, after its last claim: the last one resets the counter
    if (dyn && tid == 0) {  // (device-scope atomics: no fence, nothing else is published through the counter)
      if (atomicAdd(queue + 1, 1) == G - 1) {
        atomicExch(queue, 0);
        atomicExch(queue + 1, 0);
      }
    }
  };
  auto geo = [&](int it, int& n, int& y0, int& x0, int& cb, int& tile) {
    ws_decode(it, ncob, tile, cb);
    n = tile / tiles_per_img;
    const int r = tile - n * tiles_per_img, ty = r / tiles_x;
    y0 = ty * TH;
    x0 = (r - ty * tiles_x) * TW;
  };

  // ---------------- loader role state
  const int prow = lane >> 2, pslot = lane & 3;
  const int hpieces = ((TH + 2) * WS_PITCH + 15) >> 4;
  int hrel[WS_HPMAX];  // halo piece k of this loader wave: lane row -> (hy << 16 | hx), -1 outside the halo
#pragma unroll
  for (int k = 0; k < WS_HPMAX; ++k) {
    const int row = 16 * (wl + 4 * k) + prow;
    const int hy = row / WS_PITCH, hx = row - hy * WS_PITCH;
    hrel[k] = (hy < TH + 2 && hx < TW + 2) ? (hy << 16) | hx : -1;
  }
  // RW (resident weights): with 64 input channels and one co block the two weight chunks never change, so
  // they are staged once and the per-step DMA carries only the halo chunk (25 KB instead of 61 KB: the LDS-DMA
  // fill rate per CU, not HBM, bounded the step).  The layout is the same 156 KB rearranged: weight chunks 0 / 1 at
  // [0, 73728), halo stages at 73728 + st * 25600 (else stage st = halo + weights at st * WS_STAGE).
  const bool rw = Cin == 64 && ncob == 1;
  auto hbase = [&](int st) { return lds + (rw ? 2 * WS_WROWS * 64 + st * WS_HROWS * 64 : st * WS_STAGE); };
  auto wbase = [&](int st, int ch) { return rw ? lds + ch * WS_WROWS * 64 : lds + st * WS_STAGE + WS_HROWS * 64; };
  auto issue_w = [&](int cb, int ch, char* dst) {  // the weight chunk ch of co block cb
    const __amdgpu_buffer_rsrc_t wrs = __builtin_amdgcn_make_buffer_rsrc(
        (void*)(w + ((int64_t)cb * (Cin / 32) + ch) * (9 * 64 * 32)), (short)0, 9 * 64 * 32 * 2, 0x00020000);
#pragma unroll
    for (int k = 0; k < WS_WP; ++k) {  // one contiguous tile of the chunked pack (wpk_index)
      const int q = wl + 4 * k, row = 16 * q + prow;  // row = tap * 64 + co
      const int chunk = pslot ^ cw_swz(row);
      const int vo = (row * 32 + chunk * 8) * 2;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(wrs, (__attribute__((address_space(3))) void*)(dst + q * 1024), 16, vo,
                                               0, 0, 0);
    }
  };
  auto issue_stage = [&](int it, int ch, int st) {  // loader waves: chunk ch of item it -> stage st
    int n, y0, x0, cb, tile;
    geo(it, n, y0, x0, cb, tile);
    const int c0 = ch * 32;
    const bf16* src;
    int cs, cc;
    if (c0 < g.C1) { src = x1; cs = g.C1; cc = c0; } else { src = x2; cs = g.C2; cc = c0 - g.C1; }
    const int64_t img = (int64_t)g.Hi * g.Wi * cs;
    const __amdgpu_buffer_rsrc_t xrs =
        __builtin_amdgcn_make_buffer_rsrc((void*)(src + n * img + cc), (short)0, (int)(img * 2 - cc * 2), 0x00020000);
    char* dst = hbase(st);
#pragma unroll
    for (int k = 0; k < WS_HPMAX; ++k) {
      const int q = wl + 4 * k;
      if (q < hpieces) {  // wave-uniform
        const int chunk = pslot ^ cw_swz(16 * q + prow);
        const int iy = y0 - 1 + (hrel[k] >> 16), ix = x0 - 1 + (hrel[k] & 0xffff);
        const bool in = hrel[k] >= 0 && (unsigned)iy < (unsigned)g.Hi && (unsigned)ix < (unsigned)g.Wi;
        const int vo = in ? ((iy * g.Wi + ix) * cs + chunk * 8) * 2 : 0x7ffffff0;
        __builtin_amdgcn_raw_ptr_buffer_load_lds(xrs, (__attribute__((address_space(3))) void*)(dst + q * 1024), 16, vo,
                                                 0, 0, 0);
      }
    }
    if (!rw) issue_w(cb, ch, wbase(st, ch));
  };
  // epilogue rows of loader wave wl: pixels 64 wl + 8 u + (lane >> 3), u = 0..7, channels (lane & 7) * 8 .. + 7
  bf16x8 resv[8];
  auto out_px = [&](int y0, int x0, int u, int& oy, int& ox, bool& ok) {
    const int p = 64 * wl + 8 * u + (lane >> 3);
    const int py = p / TW, px = p - py * TW;
    oy = y0 + py;
    ox = x0 + px;
    ok = py < TH && oy < g.Ho && ox < g.Wo;
  };
  auto out_rsrc = [&](int n, int cb, const bf16* a1, const bf16* a2, int& cofs, int& cstride) {
    const int n0 = cb * 64;
    const bool first = n0 < g.Co1;
    cstride = first ? g.Co1 : g.Cout - g.Co1;
    cofs = (first ? n0 : n0 - g.Co1) + (lane & 7) * 8;
    const bf16* base = first ? a1 : a2;
    const int64_t img = (int64_t)n * g.Ho * g.Wo * cstride;
    return __builtin_amdgcn_make_buffer_rsrc((void*)((base ? base : y1) + img), (short)0, g.Ho * g.Wo * cstride * 2,
                                             0x00020000);
  };
  auto load_res = [&](int it) {  // residual rows of item it (issued a step before its epilogue)
    int n, y0, x0, cb, tile;
    geo(it, n, y0, x0, cb, tile);
    int cofs, cstride;
    const __amdgpu_buffer_rsrc_t rrs = out_rsrc(n, cb, res, res2, cofs, cstride);
    const bool have = (cb * 64 < g.Co1 ? res : res2) != nullptr;  // this split's residual (none: loads return 0)
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      int oy, ox;
      bool ok;
      out_px(y0, x0, u, oy, ox, ok);
      const int off = have ? ((ok ? oy * g.Wo + ox : 0) * cstride + cofs) * 2 : 0x7ffffff0;
      resv[u] = __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(rrs, off, 0, 0));
    }
  };
  const bool has_res = (res != nullptr) || (res2 != nullptr);
  // L2 touch of the next item's input halo: one 4-B load per halo pixel line of x1, issued at an item's
  // first step, so the stage DMA of that item -- a step later -- finds its lines in L2 instead of waiting out HBM
  // latency with one stage in flight.  Covers every channel of a pixel when C1 * 2 <= 128 B (level 0).  The loads
  // go LDS-direct into a never-read 256-B row per loader wave: no VGPRs held while they fly.
  auto touch = [&](int it) {
    int n, y0, x0, cb, tile;
    geo(it, n, y0, x0, cb, tile);
    const int64_t img = (int64_t)g.Hi * g.Wi * g.C1;
    const __amdgpu_buffer_rsrc_t xrs =
        __builtin_amdgcn_make_buffer_rsrc((void*)(x1 + n * img), (short)0, (int)(img * 2), 0x00020000);
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const int q = lane + 64 * (wl + 4 * k);
      const int hy = q / (TW + 2), hx = q - hy * (TW + 2);
      const int iy = y0 - 1 + hy, ix = x0 - 1 + hx;
      const bool in = hy < TH + 2 && (unsigned)iy < (unsigned)g.Hi && (unsigned)ix < (unsigned)g.Wi;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(xrs, (__attribute__((address_space(3))) void*)(lds + WS_LDS + wl * 256),
                                               4, in ? (iy * g.Wi + ix) * g.C1 * 2 : 0x7ffffff0, 0, 0, 0);
    }
  };
  // s_waitcnt vmcnt(n) for the counts the loader loop leaves in flight
  auto vm_wait = [&](int n) {
    switch (n) {
      case 0: asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); break;
      case 2: asm volatile("s_waitcnt vmcnt(2)" ::: "memory"); break;
      case 8: asm volatile("s_waitcnt vmcnt(8)" ::: "memory"); break;
      case 9: asm volatile("s_waitcnt vmcnt(9)" ::: "memory"); break;
      case 10: asm volatile("s_waitcnt vmcnt(10)" ::: "memory"); break;
      case 11: asm volatile("s_waitcnt vmcnt(11)" ::: "memory"); break;
      case 16: asm volatile("s_waitcnt vmcnt(16)" ::: "memory"); break;
      case 17: asm volatile("s_waitcnt vmcnt(17)" ::: "memory"); break;
      case 18: asm volatile("s_waitcnt vmcnt(18)" ::: "memory"); break;
      case 19: asm volatile("s_waitcnt vmcnt(19)" ::: "memory"); break;
      default: asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); break;
    }
  };
  // epilogue of item it from the staging tile; returns after issuing its stores (8 rows + GN partial)
  auto epilogue = [&](int it) {
    int n, y0, x0, cb, tile;
    geo(it, n, y0, x0, cb, tile);
    bf16x8 rows[8];
#pragma unroll
    for (int u = 0; u < 8; ++u)
      rows[u] = *reinterpret_cast<const bf16x8*>(stg + (64 * wl + 8 * u + (lane >> 3)) * WS_ELD + (lane & 7) * 8);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    int cofs, cstride;
    const __amdgpu_buffer_rsrc_t yrs = out_rsrc(n, cb, y1, y2, cofs, cstride);
    float gs[2] = {0.f, 0.f}, gq[2] = {0.f, 0.f};
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      int oy, ox;
      bool ok;
      out_px(y0, x0, u, oy, ox, ok);
      bf16x8 v = rows[u];
      if (has_res) {  // uniform
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = (bf16)((float)v[e] + (float)resv[u][e]);
      }
      if constexpr (GN) {  // statistics of the stored bf16 y (a GroupNorm conv has no residual)
        const float m = ok ? 1.f : 0.f;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const float a0 = (float)v[4 * h], a1 = (float)v[4 * h + 1], a2 = (float)v[4 * h + 2], a3 = (float)v[4 * h + 3];
          gs[h] = fmaf(m, (a0 + a1) + (a2 + a3), gs[h]);
          gq[h] = fmaf(m, fmaf(a3, a3, fmaf(a2, a2, fmaf(a1, a1, a0 * a0))), gq[h]);
        }
      }
      const int off = ok ? ((oy * g.Wo + ox) * cstride + cofs) * 2 : 0x7ffffff0;
      __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), yrs, off, 0, 0);
    }
    if constexpr (GN) {
      // lanes with equal (lane & 7) hold the same 8 channels: sum over lane bits 3..5 (fixed order)
#pragma unroll
      for (int h = 0; h < 2; ++h) {
#pragma unroll
        for (int o = 8; o < 64; o <<= 1) {
          gs[h] += __shfl_xor(gs[h], o, 64);
          gq[h] += __shfl_xor(gq[h], o, 64);
        }
      }
      const int b = n / gn_fimg, f = n - b * gn_fimg;
      const int64_t nslot = (int64_t)gn_fimg * tiles_per_img * 4;
      const int64_t slot = ((int64_t)f * tiles_per_img + (tile - n * tiles_per_img)) * 4 + wl;
      // [B][nslot][C/4] float2: this wave's slot, the co block's 16 quads; lane c < 8 writes quads 2c, 2c + 1
      float* dst = gnp + (((int64_t)b * nslot + slot) * (g.Cout / 4) + cb * 16) * 2;
      const f32x4 v4 = {gs[0], gq[0], gs[1], gq[1]};
      const __amdgpu_buffer_rsrc_t grs = __builtin_amdgcn_make_buffer_rsrc((void*)dst, (short)0, 128, 0x00020000);
      __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v4), grs, lane < 8 ? lane * 16 : 0x7ffffff0, 0,
                                             0);
    }
  };

  // ---------------- compute role state
  int bad[4][3];
  {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int p = 64 * wl + 16 * j + lr;
      const int py = p / TW, px = p - py * TW;
      const int h0 = py < TH ? py * WS_PITCH + px : 0;
#pragma unroll
      for (int kx = 0; kx < 3; ++kx) bad[j][kx] = cw_off(h0 + kx, lg);
    }
  }
  const int a_lane = (lr << 6) + ((lg ^ cw_swz(lr)) << 4);
  f32x4 bv4[4];  // the item's bias (co = i * 16 + 4 lg + r), loaded at its first chunk, used at its last
  f32x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  // ---------------- the step loops: one per role, the same sequence of steps and barriers (a loop per role keeps
  // the two roles' registers apart: one shared loop held the loader's residual rows live through the MFMAs)
  int it0;
  if (dyn) {  // items 0 and 1, claimed by loader wave 0 and published before a block barrier
    if (wid == 4) {
      int s0 = nitems_pad, s1 = nitems_pad;
      if (lane == 0) {
        s0 = claim();
        if (s0 < nitems_pad) s1 = claim();
      }
      publish(0, __builtin_amdgcn_readfirstlane(s0));
      publish(1, __builtin_amdgcn_readfirstlane(s1));
    }
    __syncthreads();
    it0 = qslot[0];
    if (it0 >= nitems_pad) {  // the queue ran dry before this block started (whole block)
      finish_queue();
      return;
    }
  } else {
    it0 = next_valid((int)blockIdx.x);
    if (it0 >= nitems_pad) return;  // whole block, before any barrier
  }
  // the item after `it` (item k): static order, or the published claim (read at item k's first step)
  auto successor = [&](int k, int it) { return dyn ? qslot[(k + 1) % 3] : next_valid(it + G); };
  if (loader) {
    if (rw) {
      issue_w(0, 0, wbase(0, 0));
      issue_w(0, 1, wbase(0, 1));
    }
    issue_stage(it0, 0, 0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    int it = it0, ch = 0, s = 0, prev_it = -1, k = 0, succ = nitems_pad;
    const bool do_touch = g.C1 * 2 <= 128 && nchunk >= 2;
    while (true) {
      __builtin_amdgcn_s_barrier();  // stage s landed; stage s - 1 consumed; staging of prev_it written (ch == 0)
      if (ch == 0) {
        succ = successor(k, it);
        if (dyn && wid == 4) {  // claim item k + 2 (none once the queue has run dry)
          int s2 = nitems_pad;
          if (lane == 0 && succ < nitems_pad) s2 = claim();
          publish(k + 2, __builtin_amdgcn_readfirstlane(s2));
        }
      }
      const int nxt_ch = ch + 1 < nchunk ? ch + 1 : 0;
      const int nxt_it = ch + 1 < nchunk ? it : succ;
      const bool more = nxt_it < nitems_pad;
      const bool epi = ch == 0 && prev_it >= 0;
      if (epi) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // residual rows of prev_it
      if (more) issue_stage(nxt_it, nxt_ch, (s + 1) & 1);
      if (epi) epilogue(prev_it);
      // the next step ends item nxt_it (nchunk >= 2): its residual rows now, in registers at its epilogue
      const bool pre = more && has_res && nxt_ch == nchunk - 1;
      if (pre) load_res(nxt_it);
      // the item after next: its halo lines into L2 while this item's chunks run
      int tit = nitems_pad;
      if (do_touch && ch == 0) tit = succ;
      const bool tch = tit < nitems_pad;
      if (tch) touch(tit);
      // wait for this step's DMA only: the epilogue's stores (8 rows [+ 1 GN partial]), the residual loads (8) and
      // the touches (2) issued after it may stay in flight
      vm_wait((epi ? (GN ? 9 : 8) : 0) + (pre ? 8 : 0) + (tch ? 2 : 0));
      if (ch == nchunk - 1) {
        prev_it = it;
        ++k;
      }
      ch = nxt_ch;
      it = nxt_it;
      ++s;
      if (!more) break;
    }
    __builtin_amdgcn_s_barrier();  // the last item's staging rows written
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    epilogue(prev_it);
  } else {
    int it = it0, ch = 0, s = 0, k = 0, succ = nitems_pad;
    while (true) {
      __builtin_amdgcn_s_barrier();  // stage s landed; the staging tile free again (ch == 0)
      if (ch == 0) succ = successor(k, it);
      const int nxt_ch = ch + 1 < nchunk ? ch + 1 : 0;
      const int nxt_it = ch + 1 < nchunk ? it : succ;
      if (ch == 0) {
        int n, y0, x0, cb, tile;
        geo(it, n, y0, x0, cb, tile);
#pragma unroll
        for (int i = 0; i < 4; ++i)
          bv4[i] = bias ? *reinterpret_cast<const f32x4*>(bias + cb * 64 + i * 16 + lg * 4) : f32x4{0.f, 0.f, 0.f, 0.f};
      }
      cp_taps<4>(hbase(s & 1), wbase(s & 1, ch), bad, a_lane, acc);
      if (ch == nchunk - 1) {  // item end: (acc + bias) as bf16 rows of the staging tile
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int co = i * 16 + lg * 4;
          const f32x4 bv = bv4[i];
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            float v[4] = {acc[i][j][0] + bv[0], acc[i][j][1] + bv[1], acc[i][j][2] + bv[2], acc[i][j][3] + bv[3]};
            store4(stg + (64 * wl + 16 * j + lr) * WS_ELD + co, v);
            acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
          }
        }
        ++k;
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // staging rows visible at the barrier
      ch = nxt_ch;
      it = nxt_it;
      ++s;
      if (it >= nitems_pad) break;
    }
    __builtin_amdgcn_s_barrier();  // pairs with the loaders' last barrier
  }
  finish_queue();
}

}  // namespace

void conv_p32_launch(const ConvLaunchArgs& a) {
  const ConvGeom g = conv_geom(a);
  const int Nb = a.Nb, Ho = a.Ho, Wo = a.Wo, Cout = a.Cout, TH = a.TH, TW = a.TW;
  const int tx = (int)cdiv(Wo, TW), ty = (int)cdiv(Ho, TH);
  const int ncob = Cout / 64;
  const int nitems = Nb * tx * ty * ncob;
  const int nblk = std::min(nitems, cesm_num_cus());
  conv3x3p_kernel<32><<<nblk, 256, 0, a.stream>>>(a.x1, a.x2, a.wp, a.bias, a.res, a.res2, a.y1, a.y2, g, tx, tx * ty, TH,
                                                  ncob, nitems, a.gnp, a.gn_fimg);
}

void conv_ws_launch(const ConvLaunchArgs& a) {
  const ConvGeom g = conv_geom(a);
  const int Nb = a.Nb, Ho = a.Ho, Wo = a.Wo, Cout = a.Cout, TH = a.TH, TW = a.TW;
  const int tx = (int)cdiv(Wo, TW), ty = (int)cdiv(Ho, TH);
  const int ncob = Cout / 64;
  const int ntile = Nb * tx * ty;
  const int nitems_pad = (int)cdiv(ntile, 8) * 8 * ncob;
  const int nblk = std::min(nitems_pad, cesm_num_cus());
  // a stale count (a launch cut short, an aborted capture) would make every block of this launch find the queue
  // dry: zero it in stream order first (the kernel's last block also resets it)
  if (a.queue) (void)hipMemsetAsync(a.queue, 0, 2 * sizeof(int), a.stream);
#define WSL(TWv, GNv)                                                                                                \
  conv3x3ws_kernel<TWv, GNv><<<nblk, 512, 0, a.stream>>>(a.x1, a.x2, a.wp, a.bias, a.res, a.res2, a.y1, a.y2, g, TH, tx, \
                                                         tx * ty, ncob, nitems_pad, a.gnp, a.gn_fimg, a.queue)
  if (TW == 36) { if (a.gnp) WSL(36, true); else WSL(36, false); }
  else { if (a.gnp) WSL(32, true); else WSL(32, false); }
#undef WSL
}
