// Ensemble verification statistics (cesm_ens_stats in cesm_hip.h): per pixel, over the M members x_m of an ensemble
// [B][M][V][H][W] and an optional observation y [B][V][H][W], all in fp32,
//   s = sum x_m, mean = s / M;  q = sum (x_m - mean)^2, var = q / (M - 1)   (two passes over the staged members)
//   A = sum |x_m - y|,  P = sum_{i<j} |x_i - x_j|,  crps = A / M - P / (M (M - 1))   (fair CRPS, Ferro 2014)
//   rank = #{m : x_m < y}
// and per variable the row-weighted sums of (mean - y)^2, var, crps and of the rank histogram.
//
// Layout.  The unit of work is a chunk: PXB (32 or 64) consecutive pixels of one (b, v, h) row.  A 256-thread block
// stages the chunk's M x PXB member values in LDS with one pass of coalesced loads (16 bytes per lane where W % 4 == 0
// and ens is 16-byte aligned, else 4) -- ens is read from HBM exactly once -- and every statistic is then formed from
// LDS.  A thread owns a PAIR of neighbouring pixels (one ds_read_b64 feeds two pixels) and one of NP = 512 / PXB
// "parts" of the member index: part k takes i = k, k + NP, ...  The per-part partials of s, q, A, P and rank meet in
// LDS and are added in the fixed order k = 0 .. NP - 1, so the result does not depend on timing.
//
// P is formed pairwise, circularly: member i meets j = i + 1 .. i + D (mod M), D = (M - 1) / 2, and for even M also
// i + M / 2 when i < M / 2.  That is every unordered pair once, the same trip count for every i (no triangular
// imbalance between the parts, no divergence), and with rows 0 .. D - 1 of the tile repeated behind row M - 1 the
// inner loop is a fixed-stride walk without a wrap.  M is a run-time value: nothing is padded.  Cost per pixel:
// M (M - 1) / 2 subtract + |.|-add pairs and half as many 8-byte LDS reads; LDS bytes: (M + D) PXB 4 + 10.8 KB, at
// most 59.9 KB (M = 128, PXB = 64), so the default 64 KB limit holds.
//
// Accumulator.  Each block keeps fp32 partials: a chunk's sums over its pixels (wave butterfly, fixed order) meet the
// row weight once; the rank counts of a chunk are integers (LDS integer adds) before the weight touches them.  The
// block partials part[v][blk][4 + M + 1] are added over blocks in double, in a fixed order, by ens_final_kernel.  No
// float atomics anywhere.
#include <algorithm>

#include "common.h"
#include "cesm_hip.h"

namespace {

constexpr int ENS_MAX_M = 128;
constexpr int ENS_MAX_BLOCKS = 2048;  // blocks over all variables; part holds ENS_MAX_BLOCKS * (4 + M + 1) floats
constexpr int ENS_RED = 512;          // NP * PXB: one partial per (part, pixel)

__host__ __device__ constexpr int ens_lds_floats(int M, int pxb) {
  return (M + (M - 1) / 2) * pxb + 5 * ENS_RED + 64 + (M + 1);
}

template <int PXB, bool VEC>
__global__ __launch_bounds__(256) void ens_stats_kernel(const float* __restrict__ ens, const float* __restrict__ obs,
                                                        const float* __restrict__ w, const int64_t* __restrict__ row0,
                                                        float* __restrict__ mean_o, float* __restrict__ var_o,
                                                        float* __restrict__ crps_o, int* __restrict__ rank_o,
                                                        float* __restrict__ part, int B, int M, int V, int H, int W,
                                                        int Hg) {
  extern __shared__ __attribute__((aligned(16))) float ens_lds[];
  constexpr int HP = PXB / 2;   // pixel pairs of a chunk
  constexpr int NP = 256 / HP;  // parts of the member index
  const int D = (M - 1) >> 1;
  float* tile = ens_lds;  // [M + D][PXB], rows M .. M + D - 1 repeat rows 0 .. D - 1
  float* redS = tile + (M + D) * PXB;
  float* redQ = redS + ENS_RED;
  float* redA = redQ + ENS_RED;
  float* redP = redA + ENS_RED;
  int* redR = reinterpret_cast<int*>(redP + ENS_RED);
  float* ytile = reinterpret_cast<float*>(redR + ENS_RED);  // [64] the chunk's observations
  int* cnt = reinterpret_cast<int*>(ytile + 64);            // [M + 1] rank counts of the current chunk

  const int t = (int)threadIdx.x;
  const int v = (int)blockIdx.y;
  const int pp = t % HP, pk = t / HP;
  const int cpr = (W + PXB - 1) / PXB;
  const int64_t nchunk = (int64_t)B * H * cpr;
  const int64_t ms = (int64_t)V * H * W;  // member stride
  const float Mf = (float)M;
  if (t <= M) cnt[t] = 0;  // ordered before the first use by the barriers of the first chunk
  float hist = 0.f;                             // thread r <= M: sum over chunks of w_row * count[r]
  float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;  // thread 0: sum w, sum w (mean - y)^2, sum w var, sum w crps

  for (int64_t c = blockIdx.x; c < nchunk; c += gridDim.x) {
    const int64_t rowi = c / cpr;
    const int c0 = (int)(c - rowi * cpr) * PXB;
    const int b = (int)(rowi / H);
    const int h = (int)(rowi - (int64_t)b * H);
    int64_t g = (row0 ? row0[b] : 0) + h;
    g = g < 0 ? 0 : (g > Hg - 1 ? Hg - 1 : g);  // a wrong offset gives a wrong number, never a read outside w
    const float wr = w[g];
    const int64_t pix = (((int64_t)b * V + v) * H + h) * W + c0;          // the chunk's first pixel in a map
    const float* e0 = ens + (((int64_t)b * M * V + v) * H + h) * W + c0;  // ... in member 0
    const int npx = W - c0 < PXB ? W - c0 : PXB;                           // pixels of the chunk that exist

    // stage the members (pixels past the row's end: 0, never read from memory, masked at the end).  Fetching the next
    // chunk into registers while this one is worked on was tried and bought nothing (the kernel is bound by the
    // pairwise arithmetic, not by the loads) at 30 - 160 more registers.
    if (VEC) {
      constexpr int QL = PXB / 4;
      const int q4 = (t % QL) * 4;
      for (int m = t / QL; m < M; m += 256 / QL) {
        float xv[4] = {0.f, 0.f, 0.f, 0.f};
        if (q4 < npx) load4(e0 + m * ms + q4, xv);  // W % 4 == 0: a quad exists whole or not at all
        store4(tile + m * PXB + q4, xv);
        if (m < D) store4(tile + (M + m) * PXB + q4, xv);
      }
    } else {
      const int p = t % PXB;
      for (int m = t / PXB; m < M; m += 256 / PXB) {
        const float x = p < npx ? e0[m * ms + p] : 0.f;
        tile[m * PXB + p] = x;
        if (m < D) tile[(M + m) * PXB + p] = x;
      }
    }
    const int p0 = 2 * pp;
    const float yc0 = (obs && p0 < npx) ? obs[pix + p0] : 0.f;
    const float yc1 = (obs && p0 + 1 < npx) ? obs[pix + p0 + 1] : 0.f;
    if (pk == 0) ytile[p0] = yc0, ytile[p0 + 1] = yc1;
    __syncthreads();

    // pass 1: the sum
    float s0 = 0.f, s1 = 0.f;
    for (int i = pk; i < M; i += NP) {
      const f32x2 x = *reinterpret_cast<const f32x2*>(tile + i * PXB + p0);
      s0 += x[0], s1 += x[1];
    }
    redS[pk * PXB + p0] = s0, redS[pk * PXB + p0 + 1] = s1;
    __syncthreads();
    s0 = 0.f, s1 = 0.f;
#pragma unroll
    for (int k = 0; k < NP; ++k) s0 += redS[k * PXB + p0], s1 += redS[k * PXB + p0 + 1];
    const float m0 = s0 / Mf, m1 = s1 / Mf;

    // pass 2: squared deviations, |x - y|, rank and the pairwise sum
    float q0 = 0.f, q1 = 0.f, A0 = 0.f, A1 = 0.f, P0 = 0.f, P1 = 0.f;
    int r0 = 0, r1 = 0;
    for (int i = pk; i < M; i += NP) {
      const float* ti = tile + i * PXB + p0;
      const f32x2 x = *reinterpret_cast<const f32x2*>(ti);
      const float d0 = x[0] - m0, d1 = x[1] - m1;
      q0 = fmaf(d0, d0, q0), q1 = fmaf(d1, d1, q1);
      if (obs) {
        A0 += fabsf(x[0] - yc0), A1 += fabsf(x[1] - yc1);
        r0 += x[0] < yc0 ? 1 : 0, r1 += x[1] < yc1 ? 1 : 0;
#pragma unroll 4
        for (int dd = 1; dd <= D; ++dd) {
          const f32x2 xj = *reinterpret_cast<const f32x2*>(ti + dd * PXB);
          P0 += fabsf(x[0] - xj[0]), P1 += fabsf(x[1] - xj[1]);
        }
        if (!(M & 1) && i < (M >> 1)) {
          const f32x2 xj = *reinterpret_cast<const f32x2*>(ti + (M >> 1) * PXB);
          P0 += fabsf(x[0] - xj[0]), P1 += fabsf(x[1] - xj[1]);
        }
      }
    }
    const int ro = pk * PXB + p0;
    redQ[ro] = q0, redQ[ro + 1] = q1;
    redA[ro] = A0, redA[ro + 1] = A1;
    redP[ro] = P0, redP[ro + 1] = P1;
    redR[ro] = r0, redR[ro + 1] = r1;
    __syncthreads();

    // one pixel per lane of wave 0: the maps, the chunk's sums and its rank counts
    if (t < 64) {
      const bool ok = t < npx;  // npx <= PXB <= 64
      float se = 0.f, vr = 0.f, cr = 0.f;
      if (ok) {
        float s = 0.f, q = 0.f;
#pragma unroll
        for (int k = 0; k < NP; ++k) s += redS[k * PXB + t], q += redQ[k * PXB + t];
        const float mean = s / Mf;
        vr = q / (Mf - 1.f);
        if (mean_o) mean_o[pix + t] = mean;
        if (var_o) var_o[pix + t] = vr;
        if (obs) {
          float A = 0.f, P = 0.f;
          int rk = 0;
#pragma unroll
          for (int k = 0; k < NP; ++k) A += redA[k * PXB + t], P += redP[k * PXB + t], rk += redR[k * PXB + t];
          const float y = ytile[t];
          cr = A / Mf - P / (Mf * (Mf - 1.f));
          const float dm = mean - y;
          se = dm * dm;
          if (crps_o) crps_o[pix + t] = cr;
          if (rank_o) rank_o[pix + t] = rk;
          if (part) atomicAdd(&cnt[rk], 1);  // integer add in LDS; 0 <= rk <= M whatever the data
        }
      }
      if (part) {
        se = wave_sum(se), vr = wave_sum(vr), cr = wave_sum(cr);
        if (t == 0) {
          a0 = fmaf(wr, (float)npx, a0);
          a1 = fmaf(wr, se, a1);
          a2 = fmaf(wr, vr, a2);
          a3 = fmaf(wr, cr, a3);
        }
      }
    }
    __syncthreads();
    if (part && obs && t <= M) {
      hist = fmaf(wr, (float)cnt[t], hist);
      cnt[t] = 0;
    }
  }
  if (part) {
    float* pb = part + ((int64_t)v * gridDim.x + blockIdx.x) * (4 + M + 1);
    if (t == 0) pb[0] = a0, pb[1] = a1, pb[2] = a2, pb[3] = a3;
    if (t <= M) pb[4 + t] = hist;
  }
}

// acc[v][k] (+)= sum over blocks of part[v][blk][k], in double: lane l adds blocks l, l + 64, ... in that order, then
// the lanes meet in wave_sum_d's butterfly.  One wave per (k, v).  Without obs only columns 0 and 2 exist.
__global__ __launch_bounds__(64) void ens_final_kernel(const float* __restrict__ part, double* __restrict__ acc,
                                                       int nblk, int M, int has_obs, int accumulate) {
  const int k = (int)blockIdx.x, v = (int)blockIdx.y, K = 4 + M + 1;
  if (!has_obs && k != 0 && k != 2) return;
  const float* p = part + (int64_t)v * nblk * K + k;
  double s = 0.0;
  for (int j = (int)threadIdx.x; j < nblk; j += 64) s += (double)p[(int64_t)j * K];
  s = wave_sum_d(s);
  if (threadIdx.x == 0) {
    double* a = acc + (int64_t)v * K + k;
    *a = accumulate ? *a + s : s;
  }
}

// Launch of one variant; returns the blocks per variable.  Every block stays resident for the whole launch (the grid is
// the number of blocks the device holds at once, from the occupancy of this kernel at this LDS size, at most
// ENS_MAX_BLOCKS over all variables) and walks its share of the chunks, so there is no second, partly filled round
// of blocks.
template <int PXB, bool VEC>
int ens_stats_run(int64_t nchunk, size_t lds, hipStream_t stream, const float* ens, const float* obs, const float* w,
                  const int64_t* row0, float* mean, float* var, float* crps, int* rank, float* part, int B, int M,
                  int V, int H, int W, int Hg) {
  int occ = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, ens_stats_kernel<PXB, VEC>, 256, lds) != hipSuccess || occ < 1)
    occ = 4;
  const int64_t slots = std::min<int64_t>((int64_t)cesm_num_cus() * occ, ENS_MAX_BLOCKS);
  const int nblk = (int)std::max<int64_t>(1, std::min<int64_t>(nchunk, slots / V));
  ens_stats_kernel<PXB, VEC><<<dim3((unsigned)nblk, (unsigned)V), 256, lds, stream>>>(ens, obs, w, row0, mean, var, crps,
                                                                                    rank, part, B, M, V, H, W, Hg);
  return nblk;
}

int ens_stats_launch(const float* ens, const float* obs, const float* w, const int64_t* row0, float* mean, float* var,
                     float* crps, int* rank, double* acc, float* part, int B, int M, int V, int H, int W, int Hg,
                     int accumulate, hipStream_t stream) {
  if (!ens || !w || B < 1 || M < 2 || M > ENS_MAX_M || V < 1 || V > ENS_MAX_BLOCKS || H < 1 || W < 1 || Hg < H)
    return CESM_EINVAL;
  if ((crps || rank) && !obs) return CESM_EINVAL;
  if (acc && !part) return CESM_EINVAL;
  if (!mean && !var && !crps && !rank && !acc) return CESM_EINVAL;
  const bool vec = W % 4 == 0 && ((uintptr_t)ens & 15) == 0;
  // 64-pixel chunks unless their empty tail lanes cost more than 6 % over 32-pixel chunks (W = 288: 320 against 288)
  const int64_t cover64 = cdiv(W, 64) * 64, cover32 = cdiv(W, 32) * 32;
  const int pxb = cover64 * 100 > cover32 * 106 ? 32 : 64;
  const int64_t nchunk = (int64_t)B * H * cdiv(W, pxb);
  const size_t lds = (size_t)ens_lds_floats(M, pxb) * sizeof(float);
  static_assert(ens_lds_floats(ENS_MAX_M, 64) * sizeof(float) <= 64 * 1024, "over the default LDS limit");
  float* pt = acc ? part : nullptr;
  int nblk;
  if (pxb == 64) {
    nblk = vec ? ens_stats_run<64, true>(nchunk, lds, stream, ens, obs, w, row0, mean, var, crps, rank, pt, B, M, V, H, W, Hg)
               : ens_stats_run<64, false>(nchunk, lds, stream, ens, obs, w, row0, mean, var, crps, rank, pt, B, M, V, H, W, Hg);
  } else {
    nblk = vec ? ens_stats_run<32, true>(nchunk, lds, stream, ens, obs, w, row0, mean, var, crps, rank, pt, B, M, V, H, W, Hg)
               : ens_stats_run<32, false>(nchunk, lds, stream, ens, obs, w, row0, mean, var, crps, rank, pt, B, M, V, H, W, Hg);
  }
  if (acc)
    ens_final_kernel<<<dim3((unsigned)(4 + M + 1), (unsigned)V), 64, 0, stream>>>(part, acc, nblk, M, obs != nullptr,
                                                                                 accumulate);
  return cesm_launch_status();
}

}  // namespace

// ensemble mean / variance / fair CRPS / rank maps and their row-weighted sums
extern "C" int cesm_ens_stats(const float* ens, const float* obs, const float* w, const int64_t* row0, float* mean,
                              float* var, float* crps, int* rank, double* acc, float* part, int B, int M, int V, int H,
                              int W, int Hg, int accumulate, hipStream_t stream) {
  return ens_stats_launch(ens, obs, w, row0, mean, var, crps, rank, acc, part, B, M, V, H, W, Hg, accumulate, stream);
}
