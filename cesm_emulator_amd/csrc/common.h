// Shared device helpers for the CESM-emulator gfx950 kernels.
// Storage types: float (fp32 parity mode) and __bf16 (perf mode); all arithmetic and
// all reductions are fp32 (fp64 where a cross-workgroup statistic needs it).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>

#define CESM_OK 0
#define CESM_EINVAL -1
#define CESM_EUNSUPPORTED -2
#define CESM_ELAUNCH -3

#define CESM_DT_F32 0
#define CESM_DT_BF16 1

typedef __bf16 bf16;
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

#define LDS_PTR(T) __attribute__((address_space(3))) T*

// compute units of the current device (cached; 256 on MI355X)
static inline int cesm_num_cus() {
  static int n = 0;
  if (!n) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess ||
        n <= 0)
      n = 256;
  }
  return n;
}

static inline int cesm_launch_status() {
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? CESM_OK : CESM_ELAUNCH;
}

__device__ __forceinline__ float to_f(float x) { return x; }
__device__ __forceinline__ float to_f(bf16 x) { return (float)x; }
template <typename T> __device__ __forceinline__ T from_f(float x);
template <> __device__ __forceinline__ float from_f<float>(float x) { return x; }
template <> __device__ __forceinline__ bf16 from_f<bf16>(float x) { return (bf16)x; }

// 8 consecutive elements <-> 8 floats (16 B for bf16, 32 B for fp32)
__device__ __forceinline__ void load8(const float* p, float* v) {
  const f32x4 a = *reinterpret_cast<const f32x4*>(p);
  const f32x4 b = *reinterpret_cast<const f32x4*>(p + 4);
  v[0] = a[0]; v[1] = a[1]; v[2] = a[2]; v[3] = a[3];
  v[4] = b[0]; v[5] = b[1]; v[6] = b[2]; v[7] = b[3];
}
__device__ __forceinline__ void load8(const bf16* p, float* v) {
  const bf16x8 a = *reinterpret_cast<const bf16x8*>(p);
#pragma unroll
  for (int i = 0; i < 8; ++i) v[i] = (float)a[i];
}
__device__ __forceinline__ void store8(float* p, const float* v) {
  f32x4 a = {v[0], v[1], v[2], v[3]};
  f32x4 b = {v[4], v[5], v[6], v[7]};
  *reinterpret_cast<f32x4*>(p) = a;
  *reinterpret_cast<f32x4*>(p + 4) = b;
}
__device__ __forceinline__ void store8(bf16* p, const float* v) {
  bf16x8 a;
#pragma unroll
  for (int i = 0; i < 8; ++i) a[i] = (bf16)v[i];
  *reinterpret_cast<bf16x8*>(p) = a;
}
__device__ __forceinline__ void load4(const float* p, float* v) {
  const f32x4 a = *reinterpret_cast<const f32x4*>(p);
  v[0] = a[0]; v[1] = a[1]; v[2] = a[2]; v[3] = a[3];
}
__device__ __forceinline__ void load4(const bf16* p, float* v) {
  const bf16x4 a = *reinterpret_cast<const bf16x4*>(p);
  v[0] = (float)a[0]; v[1] = (float)a[1]; v[2] = (float)a[2]; v[3] = (float)a[3];
}
__device__ __forceinline__ void store4(float* p, const float* v) {
  f32x4 a = {v[0], v[1], v[2], v[3]};
  *reinterpret_cast<f32x4*>(p) = a;
}
__device__ __forceinline__ void store4(bf16* p, const float* v) {
  bf16x4 a = {(bf16)v[0], (bf16)v[1], (bf16)v[2], (bf16)v[3]};
  *reinterpret_cast<bf16x4*>(p) = a;
}

// streaming (non-temporal) accesses for per-voxel traffic that is touched once, so the weight
// fragments the fused attention kernels re-read every head stay cache-resident (round 5: plain stores instead,
// whole step 130.3 / 130.4 -> 130.9 / 130.6 ms, profiles/r5f_nt_stores_ab.txt)
__device__ __forceinline__ bf16x8 ldnt16(const bf16* p) {
  return __builtin_nontemporal_load(reinterpret_cast<const bf16x8*>(p));
}
__device__ __forceinline__ void stnt16(bf16* p, bf16x8 v) {
  __builtin_nontemporal_store(v, reinterpret_cast<bf16x8*>(p));
}
__device__ __forceinline__ void ldnt4(const bf16* p, float* v) {
  const bf16x4 a = __builtin_nontemporal_load(reinterpret_cast<const bf16x4*>(p));
  v[0] = (float)a[0]; v[1] = (float)a[1]; v[2] = (float)a[2]; v[3] = (float)a[3];
}
__device__ __forceinline__ void stnt4(bf16* p, const float* v) {
  bf16x4 a = {(bf16)v[0], (bf16)v[1], (bf16)v[2], (bf16)v[3]};
  __builtin_nontemporal_store(a, reinterpret_cast<bf16x4*>(p));
}

__device__ __forceinline__ float silu_f(float x) { return x / (1.f + __expf(-x)); }
// exact-ish silu for parity: expf (not the fast intrinsic)
__device__ __forceinline__ float silu_p(float x) { return x / (1.f + expf(-x)); }
__device__ __forceinline__ float dsilu_p(float x) {
  const float s = 1.f / (1.f + expf(-x));
  return s * (1.f + x * (1.f - s));
}

// storage-dtype dispatch: fp32 (parity mode) keeps expf + IEEE division, bf16 uses v_exp/v_rcp
__device__ __forceinline__ float fast_sigmoid(float x) { return __builtin_amdgcn_rcpf(1.f + __expf(-x)); }
template <typename T>
__device__ __forceinline__ float silu_t(float x) {
  if constexpr (std::is_same<T, float>::value) return silu_p(x);
  else return x * fast_sigmoid(x);
}
template <typename T>
__device__ __forceinline__ float dsilu_t(float x) {
  if constexpr (std::is_same<T, float>::value) return dsilu_p(x);
  else {
    const float s = fast_sigmoid(x);
    return s * (1.f + x * (1.f - s));
  }
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}
// sum over each row of 16 lanes (lanes 16r..16r+15), every lane of the row gets the total; DPP adds in a
// fixed order (quad swaps, half-row mirror, row mirror), so the result is bit-reproducible
#define CESM_DPP_ADD(v, ctrl) \
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), ctrl, 0xF, 0xF, false))
__device__ __forceinline__ float row16_sum(float v) {
  CESM_DPP_ADD(v, 0xB1);   // quad_perm [1,0,3,2]
  CESM_DPP_ADD(v, 0x4E);   // quad_perm [2,3,0,1]
  CESM_DPP_ADD(v, 0x141);  // row_half_mirror
  CESM_DPP_ADD(v, 0x140);  // row_mirror
  return v;
}
// sum over aligned groups of `width` lanes (width power of two <= 64)
__device__ __forceinline__ float group_sum(float v, int width) {
  for (int o = width >> 1; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

static inline int64_t cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }

namespace {
// a lane's fragment from an A-operand fragment image (layout and builders: attn_helpers.h)
__device__ __forceinline__ bf16x8 ld_img(const bf16* img, int mt, int KT, int kt, int lane) {
  return *reinterpret_cast<const bf16x8*>(img + (((int64_t)mt * KT + kt) * 64 + lane) * 8);
}

// lane (g, i) <- tile[r0 + 4g + e][c0 + i], e = 0..3 (hardware transpose read; EXEC all ones)
__device__ __forceinline__ s16x4 tr4(const bf16* tile, int ld, int r0, int c0, int lane) {
  const int g = lane >> 4, q = (lane >> 2) & 3, p = lane & 3;
  return __builtin_amdgcn_ds_read_tr16_b64_v4i16((LDS_PTR(s16x4))(tile + (r0 + 4 * g + q) * ld + c0 + 4 * p));
}

// ---- "region" LDS tiles of the fused attention kernels (round 3) ----
// A bf16 tile of R rows x 16*G columns is stored as G regions of [R][16] (32-B rows, region stride rs, a multiple of
// 16), and in every row the two 16-B chunks swap when bit 2 of the row is set (SW = 1) or bit 2 ^ bit 3 (SW = 2).
// The access sites of these kernels -- 16-B fragment reads of 16 rows (ds_read_b128), 8-B transposed / k-slot
// reads of 8 consecutive rows (ds_read_b64_tr_b16), 8-B per-row reads of 16 rows (ds_read_b64) and 8-B column
// stores of 16 rows (ds_write_b64) -- are then bank-conflict free, except the stores, which are 2-way (SW = 1 for
// rows read from multiple-of-4 bases, SW = 2 where 16-row 8-B reads occur; tools/lds_banks.py enumerates every
// site, tools/lds_probe.hip measures them: SQ_LDS_BANK_CONFLICT 0 on the reads, 50 % of the store cycles).  A
// conflict-free store needs the 8-B slot XORed with (r >> 2) & 3, which splits the 16-B read pairs of odd row
// groups and is not XOR-separable for reads at 4-aligned row bases: measured free stores, not adopted (§6b).  Column constants (the head dim half, the q/k/v kind) only
// select a region -- an immediate offset -- so every site needs one per-lane offset register, which the
// register-bound backward kernels depend on (an XOR-swizzled 64-B row needs one per column constant).
// Round 2's padded rows (80 / 144 / 272 B) were 2-way on the fragment and transposed reads: 42-49 % of the LDS
// cycles of tw_fwd / twh_bwd / slah_dx were bank conflicts (profiles/r2_v14_pmc_sq.txt).
template <int SW = 1>
__device__ __forceinline__ int rg_off(int r, int c, int rs) {
  const int sw = SW == 1 ? (r >> 2) : ((r >> 2) ^ (r >> 3));
  return (c >> 4) * rs + r * 16 + ((((c >> 3) ^ sw) & 1) << 3) + (c & 7);
}
// rg_off<1>(rb + i, c, rs) for rb % 4 == 0: bit 2 of rb + i is bit 2 of rb XOR bit 2 of i, so the offset is the
// per-lane rg_off<1>(i, c, rs) XOR a uniform term, plus the uniform row base
__device__ __forceinline__ int rg_at(int rb, int lane_off) { return rb * 16 + (lane_off ^ ((rb & 4) << 1)); }
// hardware-transpose read of a region tile: lane (g, i) <- tile[r0 + 4g + e][c0 + i], e = 0..3 (EXEC all ones)
template <int SW = 1>
__device__ __forceinline__ s16x4 tr4_rg(const bf16* tile, int r0, int c0, int rs, int lane) {
  const int g = lane >> 4, q = (lane >> 2) & 3, p = lane & 3;
  return __builtin_amdgcn_ds_read_tr16_b64_v4i16((LDS_PTR(s16x4))(tile + rg_off<SW>(r0 + 4 * g + q, c0 + 4 * p, rs)));
}
// xhat / dy tiles of the head-parallel backwards: 4 regions, region stride R*16 + 16 (the 32-B stagger keeps the
// LN role's 8-lane row writes conflict-free)
__host__ __device__ constexpr int xt_rs(int R) { return R * 16 + 16; }
__host__ __device__ constexpr int xt_elems(int R) { return 4 * xt_rs(R); }
// fp32 partial dxn rows (written over a wave's own slices): 256-B rows, 16-B unit u at u ^ (r & 7) (conflict-free)
constexpr int TH_PLD = 64;
__device__ __forceinline__ int pl_off(int r, int c) { return r * TH_PLD + (((c >> 2) ^ (r & 7)) << 2) + (c & 3); }
// an SGPR zero the compiler cannot see through: added to the weight-image pointers inside the group loop so
// the (loop-invariant, per-head) fragment loads are not hoisted out of it and kept live across the loop
__device__ __forceinline__ int opaque_zero() {
  int z;
  asm volatile("s_mov_b32 %0, 0" : "=s"(z));
  return z;
}

// a VGPR copy the compiler cannot see through: a lane index re-derived from it inside a loop keeps the lane-
// dependent LDS offsets of that loop from being hoisted out of it as loop-invariant registers (they are
// recomputed per iteration at a few VALU each instead), for kernels at the 256-VGPR limit
__device__ __forceinline__ int opaque_v(int v) {
  int r;
  asm volatile("v_mov_b32 %0, %1" : "=v"(r) : "v"(v));
  return r;
}

}  // namespace

// host-side switch for A/B runs of kernel variants (read once per process)
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
static inline bool getenv_flag(const char* name) {
  static std::map<std::string, bool> cache;
  auto it = cache.find(name);
  if (it != cache.end()) return it->second;
  const char* v = std::getenv(name);
  const bool on = v && v[0] && std::strcmp(v, "0") != 0;
  cache[name] = on;
  return on;
}
