// Small ops of the training step:
//  * time embedding + small linears (video_net.py:101-113 SinusoidalPosEmb, :651-656 time_mlp,
//    :238-242 ResnetBlock.mlp = SiLU -> Linear) — M = batch rows, fp32
//  * diffusion q_sample + MSE loss and its gradient (model.py:196-208); the latitude / min-SNR weighted loss
//  * global grad-norm clip (torch/nn/utils/clip_grad.py:165-180) + fused AdamW
//    (torch/optim/adam.py:417-547, decoupled weight decay) over one flat fp32 parameter buffer
//  * dtype casts and the training-window gather (dataset_single_member.py:168-196)
#include "common.h"
#include "cesm_hip.h"

namespace {

__global__ void sinusoidal_kernel(const int64_t* __restrict__ t, float* __restrict__ emb, int B, int dim) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const int half = dim / 2;
  if (i >= B * half) return;
  const int b = i / half, k = i % half;
  const float step = logf(10000.f) / (float)(half - 1);
  const float fr = expf((float)k * -step);
  const float a = (float)t[b] * fr;
  emb[b * dim + k] = sinf(a);
  emb[b * dim + half + k] = cosf(a);
}

// y[r][o] = bias[o] + sum_i act(x[r][i]) * W[o][i]; act = silu if silu_in
// one wave per output feature o (coalesced W row), rows r looped (R = batch, small)
__global__ void linear_small_fwd_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                        const float* __restrict__ bias, float* __restrict__ y, int R, int I, int O,
                                        int silu_in) {
  const int o = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (o >= O) return;
  const float* wr = w + (int64_t)o * I;
  for (int r0 = 0; r0 < R; r0 += 8) {
    float s[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
    for (int i = lane; i < I; i += 64) {
      const float wv = wr[i];
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        if (r0 + k < R) {
          const float xv = x[(int64_t)(r0 + k) * I + i];
          s[k] = fmaf(silu_in ? silu_p(xv) : xv, wv, s[k]);
        }
      }
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      if (r0 + k >= R) break;
      const float t = wave_sum(s[k]);
      if (lane == 0) y[(int64_t)(r0 + k) * O + o] = t + (bias ? bias[o] : 0.f);
    }
  }
}

// dx[r][i] (+)= act'(x) * sum_o dy[r][o] W[o][i]
// block = 4 waves x 64 lanes: lane <-> i (64 consecutive), wave <-> quarter of the o range
__global__ __launch_bounds__(256) void linear_small_dx_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                              const float* __restrict__ dy, float* __restrict__ dx,
                                                              int R, int I, int O, int silu_in, int accumulate) {
  // block = 16 inputs i x 16 slices of the O reduction (short dependent chains: O/16 FMAs per thread);
  // the 16 i of a slice read 64 consecutive bytes of each W row
  __shared__ float red[16][17];
  const int r = blockIdx.y;
  const int il = threadIdx.x & 15, os = threadIdx.x >> 4;
  const int i = blockIdx.x * 16 + il;
  float s = 0.f;
  if (i < I) {
#pragma unroll 8
    for (int o = os; o < O; o += 16) s = fmaf(dy[(int64_t)r * O + o], w[(int64_t)o * I + i], s);
  }
  red[os][il] = s;
  __syncthreads();
  if (os == 0 && i < I) {
    s = 0.f;
#pragma unroll
    for (int k = 0; k < 16; ++k) s += red[k][il];
    const int64_t t = (int64_t)r * I + i;
    if (silu_in) s *= dsilu_p(x[t]);
    dx[t] = accumulate ? dx[t] + s : s;
  }
}

// dW[o][i] (+)= sum_r dy[r][o] act(x[r][i]); db[o] (+)= sum_r dy[r][o]
__global__ void linear_small_dw_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                                       float* __restrict__ dw, float* __restrict__ db, int R, int I, int O,
                                       int silu_in, int accumulate) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t < O * I) {
    const int o = t / I, i = t % I;
    float s = 0.f;
    for (int r = 0; r < R; ++r) {
      const float xv = silu_in ? silu_p(x[(int64_t)r * I + i]) : x[(int64_t)r * I + i];
      s = fmaf(dy[(int64_t)r * O + o], xv, s);
    }
    dw[t] = accumulate ? dw[t] + s : s;
  }
  if (db && t < O) {
    float s = 0.f;
    for (int r = 0; r < R; ++r) s += dy[(int64_t)r * O + t];
    db[t] = accumulate ? db[t] + s : s;
  }
}

// x_t = a[t_b] x0 + s[t_b] noise   (x0, noise, x_t: [B][HW] fp32)
__global__ void q_sample_kernel(const float* __restrict__ x0, const float* __restrict__ noise,
                                const int64_t* __restrict__ t, const float* __restrict__ sa,
                                const float* __restrict__ s1a, float* __restrict__ xt, int B, int64_t HW) {
  const int64_t n = (int64_t)B * HW;
  for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < n; e += (int64_t)gridDim.x * blockDim.x) {
    const int b = (int)(e / HW);
    const int64_t ti = t[b];
    xt[e] = sa[ti] * x0[e] + s1a[ti] * noise[e];
  }
}

// The guidance combine of the *_cfg kernels (classifier-free guidance, Ho & Salimans 2022): eps_g = eps_u + s (eps_c -
// eps_u), one subtraction and one FMA, each named so that no contraction choice can move it.  s (eu - eu) is an exact
// zero for finite eu, so equal halves give eps_c back bit for bit.
__device__ __forceinline__ float cfg_combine(float scale, float ec, float eu) {
  return __fmaf_rn(scale, __fsub_rn(ec, eu), eu);
}

// The three update kernels take the guidance scale as a trailing parameter pack S: empty for the unguided kernels,
// whose argument lists (and code) are those from before guidance existed, {float} for the *_cfg entries (GUIDED).
__device__ __forceinline__ float cfg_scale() { return 1.f; }
__device__ __forceinline__ float cfg_scale(float s) { return s; }

// DDPM ancestral step (model.py:168-183), fused:
//   x_{t-1} = r_t (x_t - (b_t / s1_t) eps) + sqrt(pv_t) z
// with the reference's operation order and no contraction (agrees with the eager torch expression to
// fp32 rounding).  pv_0 = 0 (alphas_cumprod_prev[0] = 1), so the t = 0 step adds no noise either way;
// z == nullptr skips the noise term (the reference's `(t == 0).all()` branch).  out may alias x.
// GUIDED: B counts samples, x / eps / out have 2 B rows: eps rows [0, B) are eps_c and rows [B, 2B) eps_u, x is read
// from rows [0, B) only, and x_prev goes to row b and to row b + B (the next evaluation's two halves); z has B rows.
template <typename... S>
__global__ void ddpm_step_kernel(const float* __restrict__ x, const float* __restrict__ eps,
                                 const float* __restrict__ z, const int64_t* __restrict__ t,
                                 const float* __restrict__ sra, const float* __restrict__ betas,
                                 const float* __restrict__ s1a, const float* __restrict__ pv, float* out, int B,
                                 int64_t HW, S... sc) {
  constexpr bool GUIDED = sizeof...(S) != 0;
  const int64_t n = (int64_t)B * HW;
  for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < n; e += (int64_t)gridDim.x * blockDim.x) {
    const int64_t ti = t[e / HW];
    const float c = __fdiv_rn(betas[ti], s1a[ti]);
    const float xv = x[e];
    float ev = eps[e];
    if constexpr (GUIDED) ev = cfg_combine(cfg_scale(sc...), ev, eps[e + n]);
    float m = __fmul_rn(sra[ti], __fsub_rn(xv, __fmul_rn(c, ev)));
    if (z) m = __fadd_rn(m, __fmul_rn(__fsqrt_rn(pv[ti]), z[e]));
    out[e] = m;
    if constexpr (GUIDED) out[e + n] = m;
  }
}

// Generalized DDIM step (Song et al. 2021, eq. 12) from t to t_prev < t, per sample (Diffusion.ddim_coefs is the
// same arithmetic on the host):
//   x_prev = a x_t + b eps + sigma z,  with ac = alphas_cumprod[t], ap = t_prev < 0 ? 1 : alphas_cumprod[t_prev],
//   sigma = eta sqrt((1-ap)/(1-ac)) sqrt(1 - ac/ap),  a = sqrt(ap/ac),
//   b = sqrt(max(1 - ap - sigma^2, 0)) - sqrt(ap (1-ac)/ac)
// a, b, sigma formed in double from the two fp32 table values and rounded to fp32 once each; the update itself is
// fp32.  eta = 0 is the deterministic DDIM, eta = 1 with t_prev = t - 1 the DDPM step (there 1 - ap - sigma^2 is
// exactly 0 on the last step and may round below it, hence the max).  blockIdx.y = sample, so the coefficients cost
// every thread two table reads; VEC: HW % 4 == 0 and every pointer 16-byte aligned -> 16-byte accesses (no tail is
// left then), else one element per access.  z == nullptr: no noise term, z is not read.  out may alias x (each thread
// reads its elements before it writes them), so neither carries __restrict__.
// GUIDED (cesm_ddim_step_cfg): gridDim.y = B samples, x / eps / out have 2 B rows as in ddpm_step_kernel; sample b
// reads x row b, eps rows b and b + B, and writes rows b and b + B of out; t, t_prev and z have B rows.
template <bool VEC, typename... S>
__global__ __launch_bounds__(256) void ddim_step_kernel(const float* x, const float* __restrict__ eps,
                                                        const float* __restrict__ z, const int64_t* __restrict__ t,
                                                        const int64_t* __restrict__ tprev,
                                                        const float* __restrict__ acp, float eta, float* out,
                                                        int64_t HW, S... sc) {
  constexpr bool GUIDED = sizeof...(S) != 0;
  const int b = blockIdx.y;
  const int64_t tp = tprev[b];
  const double ac = (double)acp[t[b]];
  const double ap = tp < 0 ? 1.0 : (double)acp[tp];
  const double sg = (double)eta * sqrt((1.0 - ap) / (1.0 - ac)) * sqrt(1.0 - ac / ap);
  const float ca = (float)sqrt(ap / ac);
  const float cb = (float)(sqrt(fmax(1.0 - ap - sg * sg, 0.0)) - sqrt(ap * (1.0 - ac) / ac));
  const float cs = (float)sg;
  const int64_t base = (int64_t)b * HW;
  const int64_t half = (int64_t)gridDim.y * HW;  // GUIDED: the distance from a row to its twin in the other half
  x += base, eps += base, out += base;
  if (z) z += base;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  if (VEC) {
    const int64_t nv = HW >> 2;
    for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < nv; e += stride) {
      float xv[4], ev[4], m[4];
      load4(x + e * 4, xv);
      load4(eps + e * 4, ev);
      if constexpr (GUIDED) {
        float uv[4];
        load4(eps + half + e * 4, uv);
#pragma unroll
        for (int i = 0; i < 4; ++i) ev[i] = cfg_combine(cfg_scale(sc...), ev[i], uv[i]);
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) m[i] = ca * xv[i] + cb * ev[i];
      if (z) {
        float zv[4];
        load4(z + e * 4, zv);
#pragma unroll
        for (int i = 0; i < 4; ++i) m[i] += cs * zv[i];
      }
      store4(out + e * 4, m);
      if constexpr (GUIDED) store4(out + half + e * 4, m);
    }
  } else {
    for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < HW; e += stride) {
      const float xv = x[e];
      float ev = eps[e];
      if constexpr (GUIDED) ev = cfg_combine(cfg_scale(sc...), ev, eps[half + e]);
      float m = ca * xv + cb * ev;
      if (z) m += cs * z[e];
      out[e] = m;
      if constexpr (GUIDED) out[half + e] = m;
    }
  }
}

// DPM-Solver++(2M) step (Lu et al. 2022) from t to t_prev < t with the x0 estimate of the previous executed step at
// t_last > t as history, per sample (Diffusion.dpmpp_coefs is the same arithmetic on the host; formulas in
// cesm_hip.h):
//   x_prev = a x + b eps + c x0_last,   x0 = c1 x + c2 eps
// Thread 0 of a block forms the sample's five coefficients in double from the fp32 table (log and expm1 included),
// rounds each to fp32 once and hands them to the block through LDS; the update itself is fp32.  Every table index is
// clamped into 0 … T-1 before it is used (a wrong device index gives a wrong number, never a read outside the table);
// t_prev < 0 (last step: x_prev is the x0 estimate, c = 0) and t_last < 0 (no history: the DDIM step) keep their
// meaning.  x0_last is read only for samples with history (t_prev >= 0 and t_last >= 0) and may be null when none has.
// blockIdx.y = sample; VEC as in ddim_step_kernel.  out may alias x and x0_out may alias x0_last (each thread reads its
// elements before it writes them), so none of the four carries __restrict__.
__device__ __forceinline__ int64_t clamp_i64(int64_t v, int64_t hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// GUIDED (cesm_dpmpp_step_cfg): gridDim.y = B samples, x / eps / out have 2 B rows as in ddpm_step_kernel; x0_last,
// x0_out, t, t_prev and t_last have B rows.
template <bool VEC, typename... S>
__global__ __launch_bounds__(256) void dpmpp_step_kernel(const float* x, const float* __restrict__ eps,
                                                         const float* x0_last, const int64_t* __restrict__ t,
                                                         const int64_t* __restrict__ tprev,
                                                         const int64_t* __restrict__ tlast,
                                                         const float* __restrict__ acp, float* out, float* x0_out,
                                                         int64_t HW, int T, S... sc) {
  constexpr bool GUIDED = sizeof...(S) != 0;
  __shared__ float coef[5];
  const int b = blockIdx.y;
  const int64_t tp = tprev[b], tl = tlast[b];
  const bool hist = x0_last != nullptr && tp >= 0 && tl >= 0;
  if (threadIdx.x == 0) {
    const double ac = (double)acp[clamp_i64(t[b], T - 1)];
    const double al_t = sqrt(ac), sg_t = sqrt(1.0 - ac), lam_t = 0.5 * log(ac / (1.0 - ac));
    const double c1 = 1.0 / al_t, c2 = -sg_t / al_t;
    double a = c1, bb = c2, c = 0.0;
    if (tp >= 0) {
      const double ap = (double)acp[clamp_i64(tp, T - 1)];
      const double al_p = sqrt(ap), sg_p = sqrt(1.0 - ap), lam_p = 0.5 * log(ap / (1.0 - ap));
      const double h = lam_p - lam_t;
      const double G = -al_p * expm1(-h);
      double wc = 1.0, wp = 0.0;
      if (tl >= 0) {
        const double al = (double)acp[clamp_i64(tl, T - 1)];
        const double r = (lam_t - 0.5 * log(al / (1.0 - al))) / h;
        wc = 1.0 + 1.0 / (2.0 * r);
        wp = -1.0 / (2.0 * r);
      }
      a = sg_p / sg_t + G * wc / al_t;
      bb = -G * wc * sg_t / al_t;
      c = G * wp;
    }
    coef[0] = (float)a, coef[1] = (float)bb, coef[2] = (float)c, coef[3] = (float)c1, coef[4] = (float)c2;
  }
  __syncthreads();
  const float ca = coef[0], cb = coef[1], cc = coef[2], c1 = coef[3], c2 = coef[4];
  const int64_t base = (int64_t)b * HW;
  const int64_t half = (int64_t)gridDim.y * HW;  // GUIDED: the distance from a row to its twin in the other half
  x += base, eps += base, out += base, x0_out += base;
  if (hist) x0_last += base;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  if (VEC) {
    const int64_t nv = HW >> 2;
    for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < nv; e += stride) {
      float xv[4], ev[4], m[4], p[4];
      load4(x + e * 4, xv);
      load4(eps + e * 4, ev);
      if constexpr (GUIDED) {
        float uv[4];
        load4(eps + half + e * 4, uv);
#pragma unroll
        for (int i = 0; i < 4; ++i) ev[i] = cfg_combine(cfg_scale(sc...), ev[i], uv[i]);
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) m[i] = ca * xv[i] + cb * ev[i];
      if (hist) {
        float hv[4];
        load4(x0_last + e * 4, hv);
#pragma unroll
        for (int i = 0; i < 4; ++i) m[i] += cc * hv[i];
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) p[i] = c1 * xv[i] + c2 * ev[i];
      store4(out + e * 4, m);
      if constexpr (GUIDED) store4(out + half + e * 4, m);
      store4(x0_out + e * 4, p);
    }
  } else {
    for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < HW; e += stride) {
      const float xv = x[e];
      float ev = eps[e];
      if constexpr (GUIDED) ev = cfg_combine(cfg_scale(sc...), ev, eps[half + e]);
      float m = ca * xv + cb * ev;
      if (hist) m += cc * x0_last[e];
      out[e] = m;
      if constexpr (GUIDED) out[half + e] = m;
      x0_out[e] = c1 * xv + c2 * ev;
    }
  }
}

// Condition dropout of classifier-free-guidance training (cesm_cond_mask): out[b] = keep[b] ? cond[b] : 0 over the n
// elements of sample b = blockIdx.y.  A select, not a multiply: a dropped sample's cond is not read.  out may alias
// cond (each thread reads its elements before it writes them), so neither carries __restrict__.  VEC as in
// ddim_step_kernel.
template <bool VEC>
__global__ __launch_bounds__(256) void cond_mask_kernel(const float* cond, const unsigned char* __restrict__ keep,
                                                        float* out, int64_t n) {
  const int b = blockIdx.y;
  const bool k = keep[b] != 0;
  const int64_t base = (int64_t)b * n;
  cond += base, out += base;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  if (VEC) {
    const int64_t nv = n >> 2;
    for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < nv; e += stride) {
      float v[4] = {0.f, 0.f, 0.f, 0.f};
      if (k) load4(cond + e * 4, v);
      store4(out + e * 4, v);
    }
  } else {
    for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < n; e += stride) out[e] = k ? cond[e] : 0.f;
  }
}

// loss partials: part[blk] = sum (pred - noise)^2
__global__ void mse_partial_kernel(const float* __restrict__ pred, const float* __restrict__ tgt,
                                   float* __restrict__ part, int64_t n) {
  __shared__ float red[256];
  float s = 0.f;
  for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < n; e += (int64_t)gridDim.x * blockDim.x) {
    const float d = pred[e] - tgt[e];
    s = fmaf(d, d, s);
  }
  red[threadIdx.x] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) part[blockIdx.x] = red[0];
}

__global__ void mse_final_kernel(const float* __restrict__ part, float* __restrict__ loss, int nblk, int64_t n) {
  if (threadIdx.x != 0) return;
  double s = 0.0;
  for (int k = 0; k < nblk; ++k) s += part[k];
  loss[0] = (float)(s / (double)n);
}

// dpred = gscale[0] * 2 (pred - noise) / n
__global__ void mse_bwd_kernel(const float* __restrict__ pred, const float* __restrict__ tgt,
                               const float* __restrict__ gscale, float* __restrict__ dpred, int64_t n) {
  const float c = 2.f * gscale[0] / (float)n;
  for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < n; e += (int64_t)gridDim.x * blockDim.x)
    dpred[e] = c * (pred[e] - tgt[e]);
}

// ---- weighted loss (latitude weights x per-sample weights on one squared-error sum; cesm_wloss in cesm_hip.h)
// The unit of work is one (b, v, h) row of W contiguous floats.  A block holds 256 / L row slots of L threads each
// (L <= 256: the threads one row keeps busy, 16 bytes per thread on the VEC path); a thread's slot and its place in
// the row are fixed for the whole launch, so the only integer divisions are the two per row that split the row index.
struct WRow {
  float w, ac;      // w[clamp(row0[b] + h)] and a[b] * ((1 - lam) + lam * w)
  int64_t base;     // offset of the row's first element
};

__device__ __forceinline__ WRow wloss_row(int64_t r, const float* __restrict__ w, const int64_t* __restrict__ row0,
                                          const float* __restrict__ a, float lam, int V, int H, int W, int Hg) {
  const int64_t bv = r / H;
  const int h = (int)(r - bv * H);
  const int b = (int)(bv / V);
  int64_t g = (row0 ? row0[b] : 0) + h;
  g = g < 0 ? 0 : (g > Hg - 1 ? Hg - 1 : g);  // a wrong offset gives a wrong number, never a read outside w
  WRow o;
  o.w = w[g];
  const float c = (1.f - lam) + lam * o.w;
  o.ac = a ? a[b] * c : c;
  o.base = r * W;
  return o;
}

// part[blk][3] = the block's sums of d^2, w d^2 and a c d^2 (d = pred - noise); the weights meet a row's sum once
template <bool VEC>
__global__ __launch_bounds__(256) void wloss_partial_kernel(const float* __restrict__ pred,
                                                            const float* __restrict__ noise,
                                                            const float* __restrict__ w,
                                                            const int64_t* __restrict__ row0,
                                                            const float* __restrict__ a, float lam,
                                                            float* __restrict__ part, int64_t R, int V, int H, int W,
                                                            int Hg, int L) {
  __shared__ float red[4][3];
  const int slot = (int)threadIdx.x / L, li = (int)threadIdx.x - slot * L, slots = 256 / L;
  float s0 = 0.f, s1 = 0.f, s2 = 0.f;
  if (slot < slots) {
    for (int64_t r = (int64_t)blockIdx.x * slots + slot; r < R; r += (int64_t)gridDim.x * slots) {
      const WRow row = wloss_row(r, w, row0, a, lam, V, H, W, Hg);
      const float* p = pred + row.base;
      const float* q = noise + row.base;
      float rs = 0.f;
      if (VEC) {
        for (int e = li; e < (W >> 2); e += L) {
          float pv[4], qv[4];
          load4(p + e * 4, pv);
          load4(q + e * 4, qv);
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const float d = pv[i] - qv[i];
            rs = fmaf(d, d, rs);
          }
        }
      } else {
        for (int e = li; e < W; e += L) {
          const float d = p[e] - q[e];
          rs = fmaf(d, d, rs);
        }
      }
      s0 += rs;
      s1 = fmaf(row.w, rs, s1);
      s2 = fmaf(row.ac, rs, s2);
    }
  }
  s0 = wave_sum(s0), s1 = wave_sum(s1), s2 = wave_sum(s2);
  const int wv = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) red[wv][0] = s0, red[wv][1] = s1, red[wv][2] = s2;
  __syncthreads();
  if (threadIdx.x < 3)
    part[blockIdx.x * 3 + threadIdx.x] =
        ((red[0][threadIdx.x] + red[1][threadIdx.x]) + red[2][threadIdx.x]) + red[3][threadIdx.x];
}

// out = {mse_raw, mse_lat, total}: the block partials added in double in a fixed order by ONE wave -- lane l adds the
// partials of blocks l, l + 64, ... in that order, then the lanes' sums meet in wave_sum_d's butterfly.  (One thread
// walking all 512 partials, as mse_final_kernel does, measured 41 us here against 5 us for the partial kernel.)
__global__ __launch_bounds__(64) void wloss_final_kernel(const float* __restrict__ part, float* __restrict__ out,
                                                         int nblk, int64_t n) {
  double s0 = 0.0, s1 = 0.0, s2 = 0.0;
  for (int k = threadIdx.x; k < nblk; k += 64) {
    s0 += part[k * 3], s1 += part[k * 3 + 1], s2 += part[k * 3 + 2];
  }
  s0 = wave_sum_d(s0), s1 = wave_sum_d(s1), s2 = wave_sum_d(s2);
  if (threadIdx.x == 0) {
    out[0] = (float)(s0 / (double)n);
    out[1] = (float)(s1 / (double)n);
    out[2] = (float)(s2 / (double)n);
  }
}

// dpred = gscale[0] (2 / n) a[b] c(b, h) (pred - noise)
template <bool VEC>
__global__ __launch_bounds__(256) void wloss_bwd_kernel(const float* __restrict__ pred,
                                                        const float* __restrict__ noise,
                                                        const float* __restrict__ w,
                                                        const int64_t* __restrict__ row0,
                                                        const float* __restrict__ a, float lam,
                                                        const float* __restrict__ gscale, float* __restrict__ dpred,
                                                        int64_t R, int V, int H, int W, int Hg, int L) {
  const int slot = (int)threadIdx.x / L, li = (int)threadIdx.x - slot * L, slots = 256 / L;
  if (slot >= slots) return;
  const float sc = 2.f * gscale[0] / (float)(R * W);
  for (int64_t r = (int64_t)blockIdx.x * slots + slot; r < R; r += (int64_t)gridDim.x * slots) {
    const WRow row = wloss_row(r, w, row0, a, lam, V, H, W, Hg);
    const float k = sc * row.ac;
    const float* p = pred + row.base;
    const float* q = noise + row.base;
    float* o = dpred + row.base;
    if (VEC) {
      for (int e = li; e < (W >> 2); e += L) {
        float pv[4], qv[4], dv[4];
        load4(p + e * 4, pv);
        load4(q + e * 4, qv);
#pragma unroll
        for (int i = 0; i < 4; ++i) dv[i] = k * (pv[i] - qv[i]);
        store4(o + e * 4, dv);
      }
    } else {
      for (int e = li; e < W; e += L) o[e] = k * (p[e] - q[e]);
    }
  }
}

// the launch shape of the weighted-loss kernels: L threads per row slot and the grid, at most 512 blocks
struct WLossGeom {
  bool vec;
  int L;
  unsigned grid;
};
bool wloss_geom(int B, int V, int H, int W, int Hg, float lam, uintptr_t ptrs, WLossGeom* g) {
  if (B < 1 || V < 1 || H < 1 || W < 1 || Hg < H || !(lam >= 0.f && lam <= 1.f)) return false;
  g->vec = W % 4 == 0 && (ptrs & 15) == 0;
  const int units = g->vec ? W / 4 : W;       // accesses per row
  const int passes = (int)cdiv(units, 256);   // a row longer than the block takes several, evenly filled
  g->L = (int)cdiv(units, passes);
  g->grid = (unsigned)std::min<int64_t>(cdiv((int64_t)B * V * H, 256 / g->L), 512);
  return true;
}

// ---- grad norm + clip + AdamW over flat fp32 buffers
__global__ void sumsq_partial_kernel(const float* __restrict__ g, double* __restrict__ part, int64_t n) {
  __shared__ double red[256];
  double s = 0.0;
  for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < n; e += (int64_t)gridDim.x * blockDim.x) {
    const float v = g[e];
    s += (double)v * v;
  }
  red[threadIdx.x] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) part[blockIdx.x] = red[0];
}

// info[0] = total norm, info[1] = clip coef (clamped to 1), info[2] = 1 if finite (norm & loss)
__global__ void clip_coef_kernel(const double* __restrict__ part, int nblk, float max_norm,
                                 const float* __restrict__ loss, float* __restrict__ info) {
  if (threadIdx.x != 0) return;
  double s = 0.0;
  for (int k = 0; k < nblk; ++k) s += part[k];
  const float norm = (float)sqrt(s);
  info[0] = norm;
  float coef = max_norm > 0.f ? max_norm / (norm + 1e-6f) : 1.f;
  info[1] = coef < 1.f ? coef : 1.f;
  const bool fin = isfinite(norm) && (loss == nullptr || isfinite(loss[0]));
  info[2] = fin ? 1.f : 0.f;
}

// step counter kept on the device: advanced only when the step is finite (info[2]), so a skipped step
// leaves the bias corrections and the saved "step" consistent with exp_avg / exp_avg_sq (as
// torch.optim.AdamW, which never sees a skipped step).  info[3] = the step number this update uses.
__global__ void adamw_step_kernel(float* __restrict__ info, int* __restrict__ step) {
  if (threadIdx.x != 0) return;
  const int s = step[0] + ((info[2] != 0.f) ? 1 : 0);
  step[0] = s;
  info[3] = (float)s;
}

__global__ void adamw_kernel(float* __restrict__ p, float* __restrict__ g, float* __restrict__ m,
                             float* __restrict__ v, const float* __restrict__ info, int64_t n, float lr, float b1,
                             float b2, float eps, float wd, int use_clip) {
  if (info[2] == 0.f) return;  // non-finite loss/grad: no update (train step raises)
  const float coef = use_clip ? info[1] : 1.f;
  const float st = info[3];
  const float bc1 = 1.f - powf(b1, st);
  const float bc2_sqrt = sqrtf(1.f - powf(b2, st));
  const float step_size = lr / bc1;
  const float decay = 1.f - lr * wd;
  for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < n; e += (int64_t)gridDim.x * blockDim.x) {
    const float gr = g[e] * coef;
    if (use_clip) g[e] = gr;
    const float pv = p[e] * decay;
    const float mv = m[e] + (1.f - b1) * (gr - m[e]);
    const float vv = v[e] * b2 + (1.f - b2) * gr * gr;
    m[e] = mv;
    v[e] = vv;
    const float denom = sqrtf(vv) / bc2_sqrt + eps;
    p[e] = pv - step_size * (mv / denom);
  }
}

// ---- AdamW step + EMA of the weights in the same pass (cesm_adamw_ema)
// adamw_step_kernel plus the EMA bookkeeping, all of it only for a finite step: n = ++ema_n[0] counts the EMA
// updates, ema_omd[0] = 1 - decay(n) is what the main kernel blends with; decay(n) = min(beta, (1+n)/(10+n)) with
// warm-up, beta without, formed in double and rounded to fp32 once (ema.ema_decay is the host restatement).
__global__ void adamw_ema_step_kernel(float* __restrict__ info, int* __restrict__ step, int* __restrict__ ema_n,
                                      float* __restrict__ ema_omd, float beta, int warmup) {
  if (threadIdx.x != 0) return;
  const bool fin = info[2] != 0.f;
  const int s = step[0] + (fin ? 1 : 0);
  step[0] = s;
  info[3] = (float)s;
  if (!fin) return;
  const int n = ema_n[0] + 1;
  ema_n[0] = n;
  double d = (double)beta;
  if (warmup) {
    const double w = (1.0 + (double)n) / (10.0 + (double)n);
    d = w < d ? w : d;
  }
  ema_omd[0] = (float)(1.0 - d);
}

// One element of adamw_kernel (same expressions, same order) followed by the EMA blend with the parameter value just
// formed: e += omd (p_new - e).  Every operation is rounded on its own (no FMA contraction), which is what
// adamw_kernel's loop compiles to: there the packed multiplies and adds leave nothing to fuse.  Here the loop is laid
// out differently (the g store sinks below the arithmetic) and the compiler would fuse g * coef - m; p, g, m and v
// have to come out bit-identical to the plain step's, so contraction is off for this body.
__device__ __forceinline__ void adamw_ema_elem(float& pe, float& ge, float& me, float& ve, float& ee, float coef,
                                               int use_clip, float decay, float b1, float b2, float bc2_sqrt,
                                               float eps, float step_size, float omd) {
#pragma clang fp contract(off)
  const float gr = ge * coef;
  if (use_clip) ge = gr;
  const float pv = pe * decay;
  const float mv = me + (1.f - b1) * (gr - me);
  const float vv = ve * b2 + (1.f - b2) * gr * gr;
  me = mv;
  ve = vv;
  const float denom = sqrtf(vv) / bc2_sqrt + eps;
  const float pn = pv - step_size * (mv / denom);
  pe = pn;
  ee = ee + omd * (pn - ee);
}

// VEC: 128-bit accesses over the first n / 4 * 4 elements (the host checks that all five pointers are 16-byte
// aligned), the last n % 4 by the first threads of the grid; otherwise scalar grid-stride like adamw_kernel.
template <bool VEC>
__global__ void adamw_ema_kernel(float* __restrict__ p, float* __restrict__ g, float* __restrict__ m,
                                 float* __restrict__ v, float* __restrict__ ema, const float* __restrict__ info,
                                 const float* __restrict__ ema_omd, int64_t n, float lr, float b1, float b2, float eps,
                                 float wd, int use_clip) {
  if (info[2] == 0.f) return;  // non-finite loss/grad: no update, the EMA stays too
  const float coef = use_clip ? info[1] : 1.f;
  const float st = info[3];
  const float bc1 = 1.f - powf(b1, st);
  const float bc2_sqrt = sqrtf(1.f - powf(b2, st));
  const float step_size = lr / bc1;
  const float decay = 1.f - lr * wd;
  const float omd = ema_omd[0];
  const int64_t gid = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  if constexpr (VEC) {
    const int64_t n4 = n / 4;
    for (int64_t q = gid; q < n4; q += stride) {
      float4 pq = reinterpret_cast<const float4*>(p)[q];
      float4 gq = reinterpret_cast<const float4*>(g)[q];
      float4 mq = reinterpret_cast<const float4*>(m)[q];
      float4 vq = reinterpret_cast<const float4*>(v)[q];
      float4 eq = reinterpret_cast<const float4*>(ema)[q];
      adamw_ema_elem(pq.x, gq.x, mq.x, vq.x, eq.x, coef, use_clip, decay, b1, b2, bc2_sqrt, eps, step_size, omd);
      adamw_ema_elem(pq.y, gq.y, mq.y, vq.y, eq.y, coef, use_clip, decay, b1, b2, bc2_sqrt, eps, step_size, omd);
      adamw_ema_elem(pq.z, gq.z, mq.z, vq.z, eq.z, coef, use_clip, decay, b1, b2, bc2_sqrt, eps, step_size, omd);
      adamw_ema_elem(pq.w, gq.w, mq.w, vq.w, eq.w, coef, use_clip, decay, b1, b2, bc2_sqrt, eps, step_size, omd);
      if (use_clip) reinterpret_cast<float4*>(g)[q] = gq;
      reinterpret_cast<float4*>(m)[q] = mq;
      reinterpret_cast<float4*>(v)[q] = vq;
      reinterpret_cast<float4*>(p)[q] = pq;
      reinterpret_cast<float4*>(ema)[q] = eq;
    }
    const int64_t e = n4 * 4 + gid;  // tail: at most 3 elements
    if (e < n) {
      float ge = g[e];
      adamw_ema_elem(p[e], ge, m[e], v[e], ema[e], coef, use_clip, decay, b1, b2, bc2_sqrt, eps, step_size, omd);
      if (use_clip) g[e] = ge;
    }
  } else {
    for (int64_t e = gid; e < n; e += stride) {
      float ge = g[e];
      adamw_ema_elem(p[e], ge, m[e], v[e], ema[e], coef, use_clip, decay, b1, b2, bc2_sqrt, eps, step_size, omd);
      if (use_clip) g[e] = ge;
    }
  }
}

template <typename T>
__global__ void add_kernel(const T* __restrict__ a, const T* __restrict__ b, T* __restrict__ out, int64_t n8) {
  for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < n8; e += (int64_t)gridDim.x * blockDim.x) {
    float x[8], y[8];
    load8(a + e * 8, x);
    load8(b + e * 8, y);
#pragma unroll
    for (int i = 0; i < 8; ++i) x[i] += y[i];
    store8(out + e * 8, x);
  }
}

// grid (blocks, B): sample b's n16 16-byte units from src + b * sstride to dst + b * dstride (strides in units)
__global__ __launch_bounds__(256) void rows_copy_kernel(const uint4* __restrict__ src, uint4* __restrict__ dst,
                                                        int64_t n16, int64_t sstride, int64_t dstride) {
  const uint4* s = src + blockIdx.y * sstride;
  uint4* d = dst + blockIdx.y * dstride;
  for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < n16; e += (int64_t)gridDim.x * blockDim.x)
    d[e] = s[e];
}

template <typename TI, typename TO>
__global__ void cast_kernel(const TI* __restrict__ x, TO* __restrict__ y, int64_t n) {
  for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < n; e += (int64_t)gridDim.x * blockDim.x)
    y[e] = from_f<TO>(to_f(x[e]));
}

// Training-window gather (dataset_single_member.py:168-196) from arrays resident in device or
// pinned host memory: cond/tgt [T][M][H][W] fp32.  Per item i: (t0, m, anchor, rev, ci, cj):
// cond_win[i][0][k][y][x] = cond[times[k]][m][ci+y][cj+x], x0[i][0][y][x] = tgt[anchor][m][..]
// times[k] = t0 + k, with the "reverse both halves around the centre" augmentation when rev.
__global__ void window_gather_kernel(const float* __restrict__ cond, const float* __restrict__ tgt,
                                     const int64_t* __restrict__ items, float* __restrict__ cwin,
                                     float* __restrict__ x0, int nitems, int K, int M, int H, int W, int h, int w,
                                     int center) {
  const int64_t per = (int64_t)(K + 1) * h * w;
  const int64_t total = per * nitems;
  for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
    const int it = (int)(e / per);
    int64_t r = e - (int64_t)it * per;
    const int k = (int)(r / ((int64_t)h * w));
    r -= (int64_t)k * h * w;
    const int y = (int)(r / w), x = (int)(r % w);
    const int64_t* d = items + it * 6;
    const int64_t t0 = d[0], m = d[1], anchor = d[2], rev = d[3], ci = d[4], cj = d[5];
    if (k < K) {
      int kk = k;
      if (rev) {
        if (center) {
          const int mid = K / 2;
          if (k < mid) kk = mid - 1 - k;
          else if (k > mid) kk = K - 1 - (k - mid - 1);
        } else {
          kk = K - 1 - k;
        }
      }
      const int64_t tt = t0 + kk;
      cwin[(((int64_t)it * K + k) * h + y) * w + x] = cond[(((tt * M + m) * H) + ci + y) * W + cj + x];
    } else {
      x0[((int64_t)it * h + y) * w + x] = tgt[(((anchor * M + m) * H) + ci + y) * W + cj + x];
    }
  }
}

// ---- V-variable window gather (cesm_window_gather_mv in cesm_hip.h): explicit frame indices per item, so the random
// sample modes and the time reversal are nothing but a different `times` row.
// The unit of work is one output row (n, plane, y) of w contiguous floats, plane in V K (cond windows) + V (targets),
// laid out as in the weighted loss: a block holds 256 / L row slots of L threads, a thread's slot and its place in the
// row are fixed for the launch, and the integer divisions and the item's meta / times reads happen once per row.
// Every index is clamped before an address is formed: a bad index gives a wrong number, never a read outside the array.
struct GatherSel {
  int c0, c1, c2, c3;  // csel[v]: by value, picked with compares (no indexed private array, so no scratch)
};

// q = a / b for a >= 0, b > 0: 32-bit division where a fits (every realistic row count), 64-bit otherwise
__device__ __forceinline__ int64_t row_div(int64_t a, int b) {
  return (a >> 31) == 0 ? (int64_t)((uint32_t)a / (uint32_t)b) : a / b;
}

template <bool VEC>
__global__ __launch_bounds__(256) void window_gather_mv_kernel(const float* __restrict__ cond,
                                                               const float* __restrict__ tgt,
                                                               const int64_t* __restrict__ times,
                                                               const int64_t* __restrict__ meta,
                                                               float* __restrict__ cwin, float* __restrict__ x0,
                                                               GatherSel sel, int64_t R, int K, int V, int Vc, int T,
                                                               int M, int H, int W, int h, int w, int L) {
  const int slot = (int)threadIdx.x / L, li = (int)threadIdx.x - slot * L, slots = 256 / L;
  if (slot >= slots) return;
  const int VK = V * K, P = VK + V;
  for (int64_t r = (int64_t)blockIdx.x * slots + slot; r < R; r += (int64_t)gridDim.x * slots) {
    const int64_t np = row_div(r, h);
    const int y = (int)(r - np * h);
    const int64_t n = row_div(np, P);
    const int p = (int)(np - n * P);
    const int64_t* mt = meta + n * 4;  // (member, anchor, i, j)
    const int64_t m = clamp_i64(mt[0], M - 1);
    const int64_t i = clamp_i64(mt[2], H - h), j = clamp_i64(mt[3], W - w);
    const float* src;
    float* dst;
    int64_t t, plane;
    if (p < VK) {
      const int v = p / K, k = p - v * K;
      const int c = v == 0 ? sel.c0 : v == 1 ? sel.c1 : v == 2 ? sel.c2 : sel.c3;
      t = times[n * K + k];
      plane = (int64_t)Vc;
      src = cond + (int64_t)c * H * W;
      dst = cwin + ((n * VK + p) * h + y) * w;
    } else {
      const int v = p - VK;
      t = mt[1];
      plane = (int64_t)V;
      src = tgt + (int64_t)v * H * W;
      dst = x0 + ((n * V + v) * h + y) * w;
    }
    t = clamp_i64(t, T - 1);
    src += ((t * M + m) * plane * H + i + y) * W + j;
    if (VEC) {
      // 16-byte stores (dst rows are 16-byte aligned: w % 4 == 0 from an aligned base); the source row starts at an
      // arbitrary j, so it is read 16 bytes at a time only where this row happens to be aligned, else by element
      if (((uintptr_t)src & 15) == 0) {
        for (int e = li; e < (w >> 2); e += L) {
          float q[4];
          load4(src + e * 4, q);
          store4(dst + e * 4, q);
        }
      } else {
        for (int e = li; e < (w >> 2); e += L) {
          const float* s = src + e * 4;
          const float q[4] = {s[0], s[1], s[2], s[3]};
          store4(dst + e * 4, q);
        }
      }
    } else {
      for (int e = li; e < w; e += L) dst[e] = src[e];
    }
  }
}

// cesm_window_gather_mc: the kernel above with the cond plane count Cc separated from V (cwin [n][Cc][K][h][w], x0
// [n][V][h][w]; work units (n, plane in Cc K + V, y)).  A kernel of its own, so that the one above stays as it is.
template <bool VEC>
__global__ __launch_bounds__(256) void window_gather_mc_kernel(const float* __restrict__ cond,
                                                               const float* __restrict__ tgt,
                                                               const int64_t* __restrict__ times,
                                                               const int64_t* __restrict__ meta,
                                                               float* __restrict__ cwin, float* __restrict__ x0,
                                                               GatherSel sel, int64_t R, int K, int V, int Cc, int Vc,
                                                               int T, int M, int H, int W, int h, int w, int L) {
  const int slot = (int)threadIdx.x / L, li = (int)threadIdx.x - slot * L, slots = 256 / L;
  if (slot >= slots) return;
  const int CK = Cc * K, P = CK + V;
  for (int64_t r = (int64_t)blockIdx.x * slots + slot; r < R; r += (int64_t)gridDim.x * slots) {
    const int64_t np = row_div(r, h);
    const int y = (int)(r - np * h);
    const int64_t n = row_div(np, P);
    const int p = (int)(np - n * P);
    const int64_t* mt = meta + n * 4;  // (member, anchor, i, j)
    const int64_t m = clamp_i64(mt[0], M - 1);
    const int64_t i = clamp_i64(mt[2], H - h), j = clamp_i64(mt[3], W - w);
    const float* src;
    float* dst;
    int64_t t, plane;
    if (p < CK) {
      const int v = p / K, k = p - v * K;
      const int c = v == 0 ? sel.c0 : v == 1 ? sel.c1 : v == 2 ? sel.c2 : sel.c3;
      t = times[n * K + k];
      plane = (int64_t)Vc;
      src = cond + (int64_t)c * H * W;
      dst = cwin + ((n * CK + p) * h + y) * w;
    } else {
      const int v = p - CK;
      t = mt[1];
      plane = (int64_t)V;
      src = tgt + (int64_t)v * H * W;
      dst = x0 + ((n * V + v) * h + y) * w;
    }
    t = clamp_i64(t, T - 1);
    src += ((t * M + m) * plane * H + i + y) * W + j;
    if (VEC) {
      // 16-byte stores to aligned rows; 16-byte loads only where this source row happens to be aligned
      if (((uintptr_t)src & 15) == 0) {
        for (int e = li; e < (w >> 2); e += L) {
          float q[4];
          load4(src + e * 4, q);
          store4(dst + e * 4, q);
        }
      } else {
        for (int e = li; e < (w >> 2); e += L) {
          const float* s = src + e * 4;
          const float q[4] = {s[0], s[1], s[2], s[3]};
          store4(dst + e * 4, q);
        }
      }
    } else {
      for (int e = li; e < w; e += L) dst[e] = src[e];
    }
  }
}

// One-GPU stand-in for the RCCL all-reduce kernels of an overlapped data-parallel backward (a measurement aid,
// tools/overlap_sim.py): nblk blocks that each take a whole CU (the launch asks for the CU's full LDS) and idle on the
// real-time clock (100 MHz) for `ticks`, as an RCCL channel block holds its CU for a bucket's transfer time.
__global__ __launch_bounds__(64) void hold_cu_kernel(long long ticks) {
  extern __shared__ char hold_lds[];
  const long long t0 = (long long)__builtin_amdgcn_s_memrealtime();
  while ((long long)__builtin_amdgcn_s_memrealtime() - t0 < ticks) __builtin_amdgcn_s_sleep(8);
  if (ticks < 0) hold_lds[threadIdx.x] = 0;  // never taken: keeps the allocation referenced
}

}  // namespace

extern "C" {

// The header's CESM_ABI_VERSION this library was compiled against (hosts compare it with their own header)
int cesm_abi_version(void) { return CESM_ABI_VERSION; }

int cesm_hold_cus(int nblk, float usec, hipStream_t stream) {
  if (nblk < 1 || !(usec >= 0.f)) return CESM_EINVAL;
  constexpr int kLds = 160 * 1024;
  // the attribute is per device: set it on every call (cheap) rather than caching one process-wide flag, which left a
  // second device of the process without it
  if (hipFuncSetAttribute((const void*)hold_cu_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, kLds) != hipSuccess)
    return CESM_ELAUNCH;
  hold_cu_kernel<<<nblk, 64, kLds, stream>>>((long long)(usec * 100.f));
  return cesm_launch_status();
}

int cesm_sinusoidal(const int64_t* t, float* emb, int B, int dim, hipStream_t stream) {
  sinusoidal_kernel<<<(unsigned)cdiv(B * (dim / 2), 256), 256, 0, stream>>>(t, emb, B, dim);
  return cesm_launch_status();
}

int cesm_linear_small_fwd(const float* x, const float* w, const float* bias, float* y, int R, int I, int O,
                          int silu_in, hipStream_t stream) {
  linear_small_fwd_kernel<<<(unsigned)cdiv(O, 4), 256, 0, stream>>>(x, w, bias, y, R, I, O, silu_in);
  return cesm_launch_status();
}

int cesm_linear_small_bwd(const float* x, const float* w, const float* dy, float* dx, float* dw, float* db, int R,
                          int I, int O, int silu_in, int accumulate_dx, int accumulate_w, hipStream_t stream) {
  if (dx)
    linear_small_dx_kernel<<<dim3((unsigned)cdiv(I, 16), R), 256, 0, stream>>>(x, w, dy, dx, R, I, O, silu_in,
                                                                               accumulate_dx);
  if (dw)
    linear_small_dw_kernel<<<(unsigned)cdiv((int64_t)O * I, 256), 256, 0, stream>>>(x, dy, dw, db, R, I, O, silu_in,
                                                                                    accumulate_w);
  return cesm_launch_status();
}

int cesm_q_sample(const float* x0, const float* noise, const int64_t* t, const float* sa, const float* s1a,
                  float* xt, int B, int64_t HW, hipStream_t stream) {
  const unsigned grid = (unsigned)std::min<int64_t>(cdiv((int64_t)B * HW, 256), 4096);
  q_sample_kernel<<<grid, 256, 0, stream>>>(x0, noise, t, sa, s1a, xt, B, HW);
  return cesm_launch_status();
}

int cesm_ddpm_step(const float* x, const float* eps, const float* z, const int64_t* t, const float* sqrt_recip_alphas,
                   const float* betas, const float* sqrt_one_minus_ac, const float* posterior_variance, float* out,
                   int B, int64_t HW, hipStream_t stream) {
  if (B < 1 || HW < 1) return CESM_EINVAL;
  const unsigned grid = (unsigned)std::min<int64_t>(cdiv((int64_t)B * HW, 256), 4096);
  ddpm_step_kernel<><<<grid, 256, 0, stream>>>(x, eps, z, t, sqrt_recip_alphas, betas, sqrt_one_minus_ac,
                                             posterior_variance, out, B, HW);
  return cesm_launch_status();
}

int cesm_ddim_step(const float* x, const float* eps, const float* z, const int64_t* t, const int64_t* t_prev,
                   const float* alphas_cumprod, float eta, float* out, int B, int64_t HW, int T, hipStream_t stream) {
  if (B < 1 || B > 65535 || HW < 1 || T < 1 || !(eta >= 0.f)) return CESM_EINVAL;
  if (eta == 0.f) z = nullptr;
  const bool vec = HW % 4 == 0 && (((uintptr_t)x | (uintptr_t)eps | (uintptr_t)z | (uintptr_t)out) & 15) == 0;
  // about 4096 blocks over the batch: grid-stride inside a sample
  const int64_t per = std::max<int64_t>(1, 4096 / B);
  const dim3 grid((unsigned)std::min<int64_t>(cdiv(vec ? HW / 4 : HW, 256), per), (unsigned)B);
  if (vec)
    ddim_step_kernel<true><<<grid, 256, 0, stream>>>(x, eps, z, t, t_prev, alphas_cumprod, eta, out, HW);
  else
    ddim_step_kernel<false><<<grid, 256, 0, stream>>>(x, eps, z, t, t_prev, alphas_cumprod, eta, out, HW);
  return cesm_launch_status();
}

int cesm_dpmpp_step(const float* x, const float* eps, const float* x0_last, const int64_t* t, const int64_t* t_prev,
                    const int64_t* t_last, const float* alphas_cumprod, float* out, float* x0_out, int B, int64_t HW,
                    int T, hipStream_t stream) {
  if (!x || !eps || !t || !t_prev || !t_last || !alphas_cumprod || !out || !x0_out) return CESM_EINVAL;
  if (B < 1 || B > 65535 || HW < 1 || T < 1) return CESM_EINVAL;
  const bool vec = HW % 4 == 0 && (((uintptr_t)x | (uintptr_t)eps | (uintptr_t)x0_last | (uintptr_t)out |
                                    (uintptr_t)x0_out) & 15) == 0;
  // the grid of cesm_ddim_step: about 4096 blocks over the batch, grid-stride inside a sample
  const int64_t per = std::max<int64_t>(1, 4096 / B);
  const dim3 grid((unsigned)std::min<int64_t>(cdiv(vec ? HW / 4 : HW, 256), per), (unsigned)B);
  if (vec)
    dpmpp_step_kernel<true><<<grid, 256, 0, stream>>>(x, eps, x0_last, t, t_prev, t_last, alphas_cumprod, out, x0_out,
                                                      HW, T);
  else
    dpmpp_step_kernel<false><<<grid, 256, 0, stream>>>(x, eps, x0_last, t, t_prev, t_last, alphas_cumprod, out, x0_out,
                                                       HW, T);
  return cesm_launch_status();
}

// The three guided updates: the grids of their unguided entries over B samples; x, eps, out hold 2 B rows.
int cesm_ddpm_step_cfg(const float* x, const float* eps, const float* z, const int64_t* t,
                       const float* sqrt_recip_alphas, const float* betas, const float* sqrt_one_minus_ac,
                       const float* posterior_variance, float* out, int B, int64_t HW, float scale,
                       hipStream_t stream) {
  if (!x || !eps || !t || !sqrt_recip_alphas || !betas || !sqrt_one_minus_ac || !posterior_variance || !out)
    return CESM_EINVAL;
  if (B < 1 || HW < 1 || !(scale >= 0.f && std::isfinite(scale))) return CESM_EINVAL;
  const unsigned grid = (unsigned)std::min<int64_t>(cdiv((int64_t)B * HW, 256), 4096);
  ddpm_step_kernel<float><<<grid, 256, 0, stream>>>(x, eps, z, t, sqrt_recip_alphas, betas, sqrt_one_minus_ac,
                                                 posterior_variance, out, B, HW, scale);
  return cesm_launch_status();
}

int cesm_ddim_step_cfg(const float* x, const float* eps, const float* z, const int64_t* t, const int64_t* t_prev,
                       const float* alphas_cumprod, float eta, float* out, int B, int64_t HW, int T, float scale,
                       hipStream_t stream) {
  if (!x || !eps || !t || !t_prev || !alphas_cumprod || !out) return CESM_EINVAL;
  if (B < 1 || B > 65535 || HW < 1 || T < 1 || !(eta >= 0.f) || !(scale >= 0.f && std::isfinite(scale)))
    return CESM_EINVAL;
  if (eta == 0.f) z = nullptr;
  const bool vec = HW % 4 == 0 && (((uintptr_t)x | (uintptr_t)eps | (uintptr_t)z | (uintptr_t)out) & 15) == 0;
  const int64_t per = std::max<int64_t>(1, 4096 / B);
  const dim3 grid((unsigned)std::min<int64_t>(cdiv(vec ? HW / 4 : HW, 256), per), (unsigned)B);
  if (vec)
    ddim_step_kernel<true, float><<<grid, 256, 0, stream>>>(x, eps, z, t, t_prev, alphas_cumprod, eta, out, HW, scale);
  else
    ddim_step_kernel<false, float><<<grid, 256, 0, stream>>>(x, eps, z, t, t_prev, alphas_cumprod, eta, out, HW, scale);
  return cesm_launch_status();
}

int cesm_dpmpp_step_cfg(const float* x, const float* eps, const float* x0_last, const int64_t* t,
                        const int64_t* t_prev, const int64_t* t_last, const float* alphas_cumprod, float* out,
                        float* x0_out, int B, int64_t HW, int T, float scale, hipStream_t stream) {
  if (!x || !eps || !t || !t_prev || !t_last || !alphas_cumprod || !out || !x0_out) return CESM_EINVAL;
  if (B < 1 || B > 65535 || HW < 1 || T < 1 || !(scale >= 0.f && std::isfinite(scale))) return CESM_EINVAL;
  const bool vec = HW % 4 == 0 && (((uintptr_t)x | (uintptr_t)eps | (uintptr_t)x0_last | (uintptr_t)out |
                                    (uintptr_t)x0_out) & 15) == 0;
  const int64_t per = std::max<int64_t>(1, 4096 / B);
  const dim3 grid((unsigned)std::min<int64_t>(cdiv(vec ? HW / 4 : HW, 256), per), (unsigned)B);
  if (vec)
    dpmpp_step_kernel<true, float><<<grid, 256, 0, stream>>>(x, eps, x0_last, t, t_prev, t_last, alphas_cumprod, out,
                                                          x0_out, HW, T, scale);
  else
    dpmpp_step_kernel<false, float><<<grid, 256, 0, stream>>>(x, eps, x0_last, t, t_prev, t_last, alphas_cumprod, out,
                                                           x0_out, HW, T, scale);
  return cesm_launch_status();
}

int cesm_cond_mask(const float* cond, const unsigned char* keep, float* out, int B, int64_t n, hipStream_t stream) {
  if (!cond || !keep || !out || B < 1 || B > 65535 || n < 1) return CESM_EINVAL;
  const bool vec = n % 4 == 0 && (((uintptr_t)cond | (uintptr_t)out) & 15) == 0;
  const int64_t per = std::max<int64_t>(1, 4096 / B);
  const dim3 grid((unsigned)std::min<int64_t>(cdiv(vec ? n / 4 : n, 256), per), (unsigned)B);
  if (vec)
    cond_mask_kernel<true><<<grid, 256, 0, stream>>>(cond, keep, out, n);
  else
    cond_mask_kernel<false><<<grid, 256, 0, stream>>>(cond, keep, out, n);
  return cesm_launch_status();
}

// loss[0] = mean((pred-tgt)^2); part: 512 floats
int cesm_mse(const float* pred, const float* tgt, float* loss, float* part, int64_t n, hipStream_t stream) {
  const int nblk = 512;
  mse_partial_kernel<<<nblk, 256, 0, stream>>>(pred, tgt, part, n);
  mse_final_kernel<<<1, 64, 0, stream>>>(part, loss, nblk, n);
  return cesm_launch_status();
}

int cesm_mse_bwd(const float* pred, const float* tgt, const float* gscale, float* dpred, int64_t n,
                 hipStream_t stream) {
  const unsigned grid = (unsigned)std::min<int64_t>(cdiv(n, 256), 4096);
  mse_bwd_kernel<<<grid, 256, 0, stream>>>(pred, tgt, gscale, dpred, n);
  return cesm_launch_status();
}

// out[3] = {mse_raw, mse_lat, total}; part: 512 * 3 floats
int cesm_wloss(const float* pred, const float* noise, const float* w, const int64_t* row0, const float* a, float lam,
               float* out, float* part, int B, int V, int H, int W, int Hg, hipStream_t stream) {
  WLossGeom g;
  if (!pred || !noise || !w || !out || !part) return CESM_EINVAL;
  if (!wloss_geom(B, V, H, W, Hg, lam, (uintptr_t)pred | (uintptr_t)noise, &g)) return CESM_EINVAL;
  const int64_t R = (int64_t)B * V * H;
  if (g.vec)
    wloss_partial_kernel<true><<<g.grid, 256, 0, stream>>>(pred, noise, w, row0, a, lam, part, R, V, H, W, Hg, g.L);
  else
    wloss_partial_kernel<false><<<g.grid, 256, 0, stream>>>(pred, noise, w, row0, a, lam, part, R, V, H, W, Hg, g.L);
  wloss_final_kernel<<<1, 64, 0, stream>>>(part, out, (int)g.grid, R * W);
  return cesm_launch_status();
}

int cesm_wloss_bwd(const float* pred, const float* noise, const float* w, const int64_t* row0, const float* a,
                   float lam, const float* gscale, float* dpred, int B, int V, int H, int W, int Hg,
                   hipStream_t stream) {
  WLossGeom g;
  if (!pred || !noise || !w || !gscale || !dpred) return CESM_EINVAL;
  if (!wloss_geom(B, V, H, W, Hg, lam, (uintptr_t)pred | (uintptr_t)noise | (uintptr_t)dpred, &g)) return CESM_EINVAL;
  const int64_t R = (int64_t)B * V * H;
  if (g.vec)
    wloss_bwd_kernel<true><<<g.grid, 256, 0, stream>>>(pred, noise, w, row0, a, lam, gscale, dpred, R, V, H, W, Hg,
                                                       g.L);
  else
    wloss_bwd_kernel<false><<<g.grid, 256, 0, stream>>>(pred, noise, w, row0, a, lam, gscale, dpred, R, V, H, W, Hg,
                                                        g.L);
  return cesm_launch_status();
}

// info[3] (device): norm, clip coef, finite flag.  part: 1024 doubles.
int cesm_grad_norm(const float* g, int64_t n, float max_norm, const float* loss, double* part, float* info,
                   hipStream_t stream) {
  const int nblk = 1024;
  sumsq_partial_kernel<<<nblk, 256, 0, stream>>>(g, part, n);
  clip_coef_kernel<<<1, 64, 0, stream>>>(part, nblk, max_norm, loss, info);
  return cesm_launch_status();
}

int cesm_adamw(float* p, float* g, float* m, float* v, float* info, int* step, int64_t n, float lr, float b1,
               float b2, float eps, float wd, int use_clip, hipStream_t stream) {
  if (!info || !step) return CESM_EINVAL;
  adamw_step_kernel<<<1, 64, 0, stream>>>(info, step);
  const unsigned grid = (unsigned)std::min<int64_t>(cdiv(n, 256), 8192);
  adamw_kernel<<<grid, 256, 0, stream>>>(p, g, m, v, info, n, lr, b1, b2, eps, wd, use_clip);
  return cesm_launch_status();
}

int cesm_adamw_ema(float* p, float* g, float* m, float* v, float* info, int* step, int64_t n, float lr, float b1,
                   float b2, float eps, float wd, int use_clip, float* ema, int* ema_n, float* ema_omd, float beta,
                   int warmup, hipStream_t stream) {
  if (!p || !g || !m || !v || !info || !step || !ema || !ema_n || !ema_omd || n < 1) return CESM_EINVAL;
  adamw_ema_step_kernel<<<1, 64, 0, stream>>>(info, step, ema_n, ema_omd, beta, warmup);
  const bool vec = n >= 4 && (((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v | (uintptr_t)ema) & 15) == 0;
  if (vec) {
    const unsigned grid = (unsigned)std::min<int64_t>(cdiv(n / 4, 256), 8192);
    adamw_ema_kernel<true><<<grid, 256, 0, stream>>>(p, g, m, v, ema, info, ema_omd, n, lr, b1, b2, eps, wd, use_clip);
  } else {
    const unsigned grid = (unsigned)std::min<int64_t>(cdiv(n, 256), 8192);
    adamw_ema_kernel<false><<<grid, 256, 0, stream>>>(p, g, m, v, ema, info, ema_omd, n, lr, b1, b2, eps, wd,
                                                      use_clip);
  }
  return cesm_launch_status();
}

int cesm_add(int dtype, const void* a, const void* b, void* out, int64_t n, hipStream_t stream) {
  if (n % 8) return CESM_EINVAL;
  const unsigned grid = (unsigned)std::min<int64_t>(cdiv(n / 8, 256), 8192);
  if (dtype == CESM_DT_BF16)
    add_kernel<bf16><<<grid, 256, 0, stream>>>((const bf16*)a, (const bf16*)b, (bf16*)out, n / 8);
  else if (dtype == CESM_DT_F32)
    add_kernel<float><<<grid, 256, 0, stream>>>((const float*)a, (const float*)b, (float*)out, n / 8);
  else
    return CESM_EINVAL;
  return cesm_launch_status();
}

// rows [row_lo, row_lo + row_n) of every sample of a [B][rows_b][C] tensor <-> compact [B][row_n][C]: per sample one
// contiguous run of row_n * C elements, copied 16 bytes per lane
static int rows_copy(int dtype, const void* src, void* dst, int B, int64_t rows_b, int64_t row_lo, int64_t row_n, int C,
                     bool gather, hipStream_t stream) {
  const int64_t es = dtype == CESM_DT_BF16 ? 2 : dtype == CESM_DT_F32 ? 4 : 0;
  if (!es || B <= 0 || B > 65535 || C <= 0 || (C * es) % 16 || row_lo < 0 || row_n <= 0 || row_lo > rows_b - row_n ||
      (((uintptr_t)src | (uintptr_t)dst) & 15))
    return CESM_EINVAL;
  const int64_t u = C * es / 16;  // 16-byte units per row
  const int64_t n16 = row_n * u, full = rows_b * u, lo = row_lo * u;
  const unsigned grid = (unsigned)std::min<int64_t>(cdiv(n16, 256), 4096);
  const uint4* s = (const uint4*)src + (gather ? lo : 0);
  uint4* d = (uint4*)dst + (gather ? 0 : lo);
  rows_copy_kernel<<<dim3(grid, B), 256, 0, stream>>>(s, d, n16, gather ? full : n16, gather ? n16 : full);
  return cesm_launch_status();
}

int cesm_rows_gather(int dtype, const void* src, void* dst, int B, int64_t rows_b, int64_t row_lo, int64_t row_n, int C,
                     hipStream_t stream) {
  return rows_copy(dtype, src, dst, B, rows_b, row_lo, row_n, C, true, stream);
}

int cesm_rows_scatter(int dtype, const void* src, void* dst, int B, int64_t rows_b, int64_t row_lo, int64_t row_n, int C,
                      hipStream_t stream) {
  return rows_copy(dtype, src, dst, B, rows_b, row_lo, row_n, C, false, stream);
}

int cesm_cast(int dtype_in, int dtype_out, const void* x, void* y, int64_t n, hipStream_t stream) {
  const unsigned grid = (unsigned)std::min<int64_t>(cdiv(n, 256), 8192);
  if (dtype_in == CESM_DT_F32 && dtype_out == CESM_DT_BF16)
    cast_kernel<float, bf16><<<grid, 256, 0, stream>>>((const float*)x, (bf16*)y, n);
  else if (dtype_in == CESM_DT_BF16 && dtype_out == CESM_DT_F32)
    cast_kernel<bf16, float><<<grid, 256, 0, stream>>>((const bf16*)x, (float*)y, n);
  else if (dtype_in == CESM_DT_F32 && dtype_out == CESM_DT_F32)
    cast_kernel<float, float><<<grid, 256, 0, stream>>>((const float*)x, (float*)y, n);
  else
    return CESM_EINVAL;
  return cesm_launch_status();
}

int cesm_window_gather(const float* cond, const float* tgt, const int64_t* items, float* cwin, float* x0,
                       int nitems, int K, int M, int H, int W, int h, int w, int center, hipStream_t stream) {
  const int64_t total = (int64_t)(K + 1) * h * w * nitems;
  const unsigned grid = (unsigned)std::min<int64_t>(cdiv(total, 256), 8192);
  window_gather_kernel<<<grid, 256, 0, stream>>>(cond, tgt, items, cwin, x0, nitems, K, M, H, W, h, w, center);
  return cesm_launch_status();
}

int cesm_window_gather_mv(const float* cond, const float* tgt, const int64_t* times, const int64_t* meta, float* cwin,
                          float* x0, int nitems, int K, int V, int Vc, int csel0, int csel1, int csel2, int csel3,
                          int T, int M, int H, int W, int h, int w, hipStream_t stream) {
  if (!cond || !tgt || !times || !meta || !cwin || !x0) return CESM_EINVAL;
  if (nitems < 1 || T < 1 || M < 1 || Vc < 1 || h < 1 || w < 1) return CESM_EINVAL;
  if (V < 1 || V > 4 || K < 1 || h > H || w > W) return CESM_EUNSUPPORTED;
  const int cs[4] = {csel0, csel1, csel2, csel3};
  for (int v = 0; v < V; ++v)
    if (cs[v] < 0 || cs[v] >= Vc) return CESM_EUNSUPPORTED;
  const bool vec = w % 4 == 0 && (((uintptr_t)cwin | (uintptr_t)x0) & 15) == 0;
  const int units = vec ? w / 4 : w;          // accesses per row
  const int passes = (int)cdiv(units, 256);   // a row longer than the block takes several, evenly filled
  const int L = (int)cdiv(units, passes);
  const int64_t R = (int64_t)nitems * (V * K + V) * h;
  // two rows per slot before the grid grows (a short row is one 16-byte store per thread), at most 2048 blocks
  const unsigned grid = (unsigned)std::min<int64_t>(cdiv(R, 2 * (256 / L)), 2048);
  const GatherSel sel = {csel0, csel1, csel2, csel3};
  if (vec)
    window_gather_mv_kernel<true><<<grid, 256, 0, stream>>>(cond, tgt, times, meta, cwin, x0, sel, R, K, V, Vc, T, M, H,
                                                            W, h, w, L);
  else
    window_gather_mv_kernel<false><<<grid, 256, 0, stream>>>(cond, tgt, times, meta, cwin, x0, sel, R, K, V, Vc, T, M,
                                                             H, W, h, w, L);
  return cesm_launch_status();
}

int cesm_window_gather_mc(const float* cond, const float* tgt, const int64_t* times, const int64_t* meta, float* cwin,
                          float* x0, int nitems, int K, int V, int Cc, int Vc, int csel0, int csel1, int csel2,
                          int csel3, int T, int M, int H, int W, int h, int w, hipStream_t stream) {
  if (Cc == V)
    return cesm_window_gather_mv(cond, tgt, times, meta, cwin, x0, nitems, K, V, Vc, csel0, csel1, csel2, csel3, T, M,
                                 H, W, h, w, stream);
  if (!cond || !tgt || !times || !meta || !cwin || !x0) return CESM_EINVAL;
  if (nitems < 1 || T < 1 || M < 1 || Vc < 1 || h < 1 || w < 1) return CESM_EINVAL;
  if (V < 1 || V > 4 || Cc < 1 || Cc > 4 || K < 1 || h > H || w > W) return CESM_EUNSUPPORTED;
  const int cs[4] = {csel0, csel1, csel2, csel3};
  for (int c = 0; c < Cc; ++c)
    if (cs[c] < 0 || cs[c] >= Vc) return CESM_EUNSUPPORTED;
  const bool vec = w % 4 == 0 && (((uintptr_t)cwin | (uintptr_t)x0) & 15) == 0;
  const int units = vec ? w / 4 : w;
  const int passes = (int)cdiv(units, 256);
  const int L = (int)cdiv(units, passes);
  const int64_t R = (int64_t)nitems * (Cc * K + V) * h;
  const unsigned grid = (unsigned)std::min<int64_t>(cdiv(R, 2 * (256 / L)), 2048);
  const GatherSel sel = {csel0, csel1, csel2, csel3};
  if (vec)
    window_gather_mc_kernel<true><<<grid, 256, 0, stream>>>(cond, tgt, times, meta, cwin, x0, sel, R, K, V, Cc, Vc, T,
                                                            M, H, W, h, w, L);
  else
    window_gather_mc_kernel<false><<<grid, 256, 0, stream>>>(cond, tgt, times, meta, cwin, x0, sel, R, K, V, Cc, Vc, T,
                                                             M, H, W, h, w, L);
  return cesm_launch_status();
}

}  // extern "C"
