/*
 * cesm_hip.h — C ABI of libcesm_hip.so, the gfx950 (MI355X) kernels behind the
 * cesm_emulator_amd drop-in for the reference's video_net training/inference hot path.
 *
 * The reference (kallenordling/cesm_emulator @ 2025-09-05) is pure Python: every entry point
 * below replaces one or more PyTorch-dispatched ATen/NCCL ops at the cited reference lines
 * (SURVEY.md §2.2).  Conventions:
 *   - all pointers are device pointers (hipMalloc / PyTorch caching allocator); kernels never
 *     allocate or free — workspaces are passed in by the caller;
 *   - activations are channels-last [N][H][W][C] with N = batch*frames, dtype = CESM_DT_F32
 *     (parity mode) or CESM_DT_BF16 (perf mode); parameters, statistics and grads are fp32;
 *   - every call is stream-ordered on `stream` and enqueue-only (no host sync, graph-capturable);
 *   - return 0 on success, negative CESM_E* on bad arguments or launch failure; the Python
 *     layer raises RuntimeError (mirroring model.py:99-132 / train.py:842-843 errors);
 *   - `accumulate` = 1 adds into the destination gradient (grad accumulation), 0 overwrites.
 */
#ifndef CESM_HIP_H
#define CESM_HIP_H
#include <hip/hip_runtime.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CESM_DT_F32 0
#define CESM_DT_BF16 1

/* ABI version of this header.  Bumped whenever an entry point's argument list changes; a host binding compares it
 * with cesm_abi_version() before the first call (cesm_emulator_amd/_lib.py does), so an old header cannot silently
 * mis-call a newer library.  History:
 *   4 (round 4): cesm_ln_fwd / cesm_ln_bwd gained (perm_f, perm_hw), cesm_tflash_fwd / cesm_tflash_bwd gained
 *     qkv_pixel_major — each before the hipStream_t;
 *   5 (round 5): cesm_abi_version() itself; cesm_conv_fwd / cesm_conv_fwd_gn gained `queue` and cesm_tblock_bwd_dw
 *     gained `dwout`, each before the hipStream_t / after dgamma;
 *   6 (round 6): cesm_tblock_bwd_dw lost `dwout` again (the in-kernel to_out weight gradient measured slower than the
 *     forward's O write and was removed) and gained `o` after dx (O emitted by the backward); cesm_conv_pack_batch's
 *     job table gained per-job block starts and its fourth argument is the grid size;
 *     cesm_qkv_bwd / cesm_qkv_bwd_streams added;
 *   7: cesm_conv_wgrad_sq_bn removed; cesm_conv_wgrad_nsplit, cesm_conv_wgrad_bias_rides and cesm_conv_pack_blocks
 *     added (host-only queries: the weight-gradient split count and the pack tiling now come from the library);
 *   8: cesm_tconv_fwd / cesm_tconv_bwd and their host-only queries added (temporal-convolution blocks). */
#define CESM_ABI_VERSION 8
int cesm_abi_version(void);
/* Measurement aid, not a training op: nblk blocks that each occupy one whole CU (full LDS) for `usec` microseconds on
 * `stream` -- the one-GPU stand-in for the RCCL kernels of an overlapped gradient all-reduce (tools/overlap_sim.py,
 * distributed.XgmiModelReducer). */
int cesm_hold_cus(int nblk, float usec, hipStream_t stream);

/* ---- convolutions (csrc/conv_fwd.hip with conv_halo.hip and conv_level0.hip; conv_wgrad.hip; conv_pack.hip) ------
 * Generic implicit-GEMM conv on MFMA. Replaces nn.Conv3d (1,k,k) at video_net.py:215 (Block.proj),
 * :246 (res_conv), :61-62 (Downsample), nn.ConvTranspose3d at :65-66 (Upsample), the attention
 * projections nn.Linear :380-381 and 1x1 nn.Conv2d :322-323, and all their data gradients.
 *   out[n,oy,ox,co] = bias[co] + res[..] + sum W[co][ky*KW+kx][ci] * X[n,(oy*S-P+ky)/U,(ox*S-P+kx)/U,ci]
 * Input may be the channel-concat of x1 (C1 ch) and x2 (C2 ch) (video_net.py:857, :868 torch.cat);
 * output channels [0,Co1) go to y1 and [Co1,Cout) to y2. */
int cesm_conv_fwd(int dtype, const void* x1, const void* x2, const void* wp, const float* bias, const void* res,
                  const void* res2, void* y1, void* y2, int Nb, int Hi, int Wi, int C1, int C2, int Ho, int Wo, int Cout, int Co1,
                  int KH, int KW, int S, int P, int U, int* queue, hipStream_t stream);
/* cesm_conv_fwd (Co1 = Cout, no residual) that also writes the GroupNorm statistics partials of its output
 * y (the Block conv feeding GroupNorm, video_net.py:215-217): gnpart [B][nslot][Cout/4] float2 (sum, sum of
 * squares per channel quad over the pixels of one partial slot), every entry written once, no atomics;
 * nslot from cesm_conv_gn_nslot (0: the kernel for this shape has no partials -> CESM_EUNSUPPORTED here,
 * use cesm_gn_stats).  Nb = B * frames. */
int64_t cesm_conv_gn_nslot(int dtype, int Nb, int Hi, int Wi, int C1, int C2, int Ho, int Wo, int Cout, int KH, int KW,
                           int S, int P, int U, int B);
int cesm_conv_fwd_gn(int dtype, const void* x1, const void* x2, const void* wp, const float* bias, void* y, float* gnpart,
                     int B, int Nb, int Hi, int Wi, int C1, int C2, int Ho, int Wo, int Cout, int KH, int KW, int S,
                     int P, int U, int* queue, hipStream_t stream);
/* name of the kernel cesm_conv_fwd launches for these arguments (host-only query, no GPU work; the
 * launcher itself selects through the same function).  "invalid" if cesm_conv_fwd would return EINVAL. */
const char* cesm_conv_fwd_variant(int dtype, int Nb, int Hi, int Wi, int C1, int C2, int Ho, int Wo, int Cout,
                                  int Co1, int KH, int KW, int S, int P, int U);
/* Host-only queries on cesm_conv_wgrad's launch plan (no GPU work; the launcher decides through the same function;
 * with_bias: db != NULL).  _variant: name of the kernel it launches.  _nsplit: the pixel-split count to size slab and
 * bslab for -- it fixes the summation order of dW, so callers take it from here instead of a formula of their own.
 * _bias_rides: 1 if the kernel chosen without a bias request can produce db in the same pass -- then pass db (and ask
 * _nsplit / _variant with with_bias = 1); 0: leave db NULL and take the bias gradient from cesm_colsum. */
const char* cesm_conv_wgrad_variant(int dtype, int Nb, int Hi, int Wi, int C1, int C2, int Ho, int Wo, int Cout,
                                    int Co1, int KH, int KW, int S, int P, int U, int with_bias);
int cesm_conv_wgrad_nsplit(int dtype, int Nb, int Hi, int Wi, int C1, int C2, int Ho, int Wo, int Cout, int Co1, int KH,
                           int KW, int S, int P, int U, int with_bias);
int cesm_conv_wgrad_bias_rides(int dtype, int Nb, int Hi, int Wi, int C1, int C2, int Ho, int Wo, int Cout, int Co1,
                               int KH, int KW, int S, int P, int U);
/* weight gradient of a cesm_conv_fwd launch; written in PyTorch layout [D0][D1][1][KH][KW] with the
 * (swap, flip) mapping of cesm_conv_pack.  slab: nsplit*Cout*KH*KW*(C1+C2) floats; any nsplit >= 1 is accepted
 * (cesm_conv_wgrad_nsplit gives the tuned one).
 * db (nullable): the conv bias gradient sum_px dY (+=), computed in the same pass (bslab: nsplit*Cout
 * floats); only on the bf16 wide / square-tile kernels — CESM_EUNSUPPORTED otherwise, before anything is launched.
 * cesm_conv_wgrad_bias_rides is narrower on purpose: it also answers 0 for a split destination (Co1 != Cout), where
 * a db passed here would still be computed by the wide kernel; the product path takes that bias gradient from
 * cesm_colsum, as it always has, so db's summation order stays what it was. */
int cesm_conv_wgrad(int dtype, const void* x1, const void* x2, const void* dy1, const void* dy2, float* dw,
                    float* slab, float* db, float* bslab, int nsplit, int Nb, int Hi, int Wi, int C1, int C2, int Ho,
                    int Wo, int Cout, int Co1, int KH, int KW, int S, int P, int U, int swap, int flip, int accumulate,
                    hipStream_t stream);
/* PyTorch conv weight (fp32) -> GEMM layout Wp[co][tap][ci] in dtype.  swap: GEMM co is dim 1 of
 * the torch tensor (transposed conv forward / conv dgrad); flip: taps reversed.  bf16 3x3 and 4x4 weights with
 * Cout % 64 == 0 and Cin % 32 == 0 are written "chunked" instead: element (co, tap, ci) at
 * (((co/64 * Cin/32 + ci/32) * KH*KW + tap) * 64 + co%64) * 32 + ci%32 -- one contiguous block per (64-co block,
 * 32-channel chunk), the tile the halo convs stage.  The pack is opaque to callers: cesm_conv_fwd reads either
 * layout by the same rule (same argument lists; round 6). */
int cesm_conv_pack(int dtype, const float* w, void* wp, int Cout, int Cin, int KH, int KW, int swap, int flip,
                   hipStream_t stream);
/* every cached pack of one dtype redone in ONE launch after an optimizer step: jobs = device
 * int64[njobs][8] {src fp32 ptr, dst ptr, Cout, Cin, KH, KW, swap, flip} (cesm_conv_pack semantics) followed by
 * int64[njobs + 1] block starts, the exclusive prefix sum of the per-job tile counts (cesm_conv_pack_blocks, host
 * only: cdiv(Cout, cot) * cdiv(Cin, 64) with cot = clamp(4096 / (KH * KW * 64), 1, 64); CESM_EINVAL if KH * KW > 64 --
 * a tile's taps x 64 channels must fit the kernel's 4096-float LDS tile, so such a job cannot be in the table), then
 * int64[starts[njobs]] the job index of every block; nblocks = the grid (the last start is the work; any nblocks >= 1
 * is correct).  ABI 6: the table gained the starts, the fourth argument was blocks_per_job. */
int cesm_conv_pack_blocks(int Cout, int Cin, int KH, int KW);
int cesm_conv_pack_batch(int dtype, const int64_t* jobs, int njobs, int nblocks, hipStream_t stream);
/* dst[c] (+)= sum over rows of x[r][c]  (conv bias gradients) ; part: nsplit*C floats */
int cesm_colsum(int dtype, const void* x, float* dst, float* part, int nsplit, int64_t rows, int C, int accumulate,
                hipStream_t stream);
/* ---- stem and head (csrc/stem_head.hip with stem_dgrad.h and multivar.h) --------------------------
 * stem Conv3d(2->Co,(1,KS,KS),pad KS/2) on cat([x_t, cond]) read straight from the NCDHW fp32 boundary
 * tensors (video_net.py:595-600, :808-815; model.py:111-121 frame broadcast). */
int cesm_stem_fwd(int dtype, const float* xt, const float* cond, const float* w, const float* bias, void* y, int B,
                  int F, int Fx, int Fc, int H, int W, int Co, int KS, hipStream_t stream);
int cesm_stem_wgrad(int dtype, const float* xt, const float* cond, const void* dy, float* dw, float* part, int nblk,
                    int B, int F, int Fx, int Fc, int H, int W, int Co, int KS, int accumulate, hipStream_t stream);
/* Data gradient of the stem (input gradients: d/d x_t and d/d cond).  dy [B*F][H][W][Co] in the compute dtype (the
 * tensor cesm_stem_wgrad reads), w the fp32 master weight [Co][2][KS][KS]; dxt [B][Fx][H][W] and dcond [B][Fc][H][W]
 * fp32 are overwritten, each nullable (then not written; its sum rides in the same MFMA rows).  An input the forward broadcast over frames
 * (Fx or Fc == 1 with F > 1) receives the sum over all F frames.  Deterministic (no atomics).  CESM_EUNSUPPORTED
 * unless KS is odd and <= 7, Co % 64 == 0 and Fx, Fc are 1 or F.  (Added without a CESM_ABI_VERSION bump: no existing
 * argument list changed.) */
int cesm_stem_dgrad(int dtype, const void* dy, const float* w, float* dxt, float* dcond,
                    int B, int F, int Fx, int Fc, int H, int W, int Co, int KS, hipStream_t stream);
/* head Conv3d(C->1,1) (video_net.py:763) evaluated on frame F//2 only (model.py:124-130). */
int cesm_head_fwd(int dtype, const void* x, const float* w, const float* bias, float* out, int B, int F, int HW, int C,
                  hipStream_t stream);
int cesm_head_bwd(int dtype, const float* dout, const void* x, const float* w, void* dx, float* dw, float* db,
                  float* part, int nblk, int B, int F, int HW, int C, int accumulate, hipStream_t stream);
/* The stem and head for V target variables, 1 <= V <= 4 (csrc/multivar.h).  Tensors are the reference's:
 * xt [B][V][Fx][H][W], cond [B][V][Fc][H][W], stem w [Co][2V][KS][KS] with input channels 0..V-1 = x_t and V..2V-1 =
 * cond, dw the same shape, part nblk*Co*2V*KS*KS floats, dxt / dcond shaped like xt / cond (each nullable); head w
 * [V][C], bias / db [V], out / dout [B][V][HW], dw [V][C], part nblk*V*(C+1) floats.  Everything else is as in the
 * five entry points above, and V == 1 IS those entry points (same kernels, same grids).  CESM_EUNSUPPORTED for V
 * outside 1..4 and for the stem shapes cesm_stem_dgrad refuses.  Deterministic.  (Added entry points: the ABI version
 * stays.) */
int cesm_stem_fwd_mv(int dtype, const float* xt, const float* cond, const float* w, const float* bias, void* y, int B,
                     int V, int F, int Fx, int Fc, int H, int W, int Co, int KS, hipStream_t stream);
int cesm_stem_wgrad_mv(int dtype, const float* xt, const float* cond, const void* dy, float* dw, float* part, int nblk,
                       int B, int V, int F, int Fx, int Fc, int H, int W, int Co, int KS, int accumulate,
                       hipStream_t stream);
int cesm_stem_dgrad_mv(int dtype, const void* dy, const float* w, float* dxt, float* dcond, int B, int V, int F, int Fx,
                       int Fc, int H, int W, int Co, int KS, hipStream_t stream);
int cesm_head_fwd_mv(int dtype, const void* x, const float* w, const float* bias, float* out, int B, int V, int F,
                     int HW, int C, hipStream_t stream);
int cesm_head_bwd_mv(int dtype, const float* dout, const void* x, const float* w, void* dx, float* dw, float* db,
                     float* part, int nblk, int B, int V, int F, int HW, int C, int accumulate, hipStream_t stream);
/* The stem with the number of conditioning maps Cc separated from the number of target variables V (multi-forcing
 * conditioning; csrc/multivar.h), 1 <= V <= 4 and 1 <= Cc <= 4: Conv3d(P -> Co), P = V + Cc, on cat([x_t, cond]).
 * xt [B][V][Fx][H][W], cond [B][Cc][Fc][H][W], w / dw [Co][P][KS][KS] with input channels 0..V-1 = x_t and V..P-1 =
 * cond, part nblk*Co*P*KS*KS floats, dxt shaped like xt and dcond like cond (each nullable).  Every other argument is
 * that of the *_mv entry, and Cc == V IS the *_mv entry (same kernels, same grids; V = Cc = 1 the single-variable
 * one).  CESM_EUNSUPPORTED for V or Cc outside 1..4 and for the stem shapes cesm_stem_dgrad refuses.  Deterministic.
 * (Added entry points: the ABI version stays.) */
int cesm_stem_fwd_mc(int dtype, const float* xt, const float* cond, const float* w, const float* bias, void* y, int B,
                     int V, int Cc, int F, int Fx, int Fc, int H, int W, int Co, int KS, hipStream_t stream);
int cesm_stem_wgrad_mc(int dtype, const float* xt, const float* cond, const void* dy, float* dw, float* part, int nblk,
                       int B, int V, int Cc, int F, int Fx, int Fc, int H, int W, int Co, int KS, int accumulate,
                       hipStream_t stream);
int cesm_stem_dgrad_mc(int dtype, const void* dy, const float* w, float* dxt, float* dcond, int B, int V, int Cc, int F,
                       int Fx, int Fc, int H, int W, int Co, int KS, hipStream_t stream);

/* ---- normalisation (csrc/norm.hip) -------------------------------------------------------
 * GroupNorm(G,C) eps, affine, then x*(scale+1)+shift, SiLU, + residual: video_net.py:216-227, :265. */
/* ws >= max(B*256, 1024)*G*2 doubles */
int cesm_gn_stats(int dtype, const void* y, float* stats, double* ws, int B, int64_t rows_b, int C, int G, float eps,
                  hipStream_t stream);
/* stats [B][G] (mean, rstd) from cesm_conv_fwd_gn's partials (replaces cesm_gn_stats' pass over y):
 * fixed-order double reduction, rows_b = voxels per sample.  part is scratch: for large nslot (>= 8192) the
 * two-stage reduction overwrites it with its block sums */
int cesm_gn_stats_part(float* part, float* stats, int B, int64_t nslot, int C, int G, int64_t rows_b, float eps,
                       hipStream_t stream);
int cesm_gn_apply(int dtype, const void* y, const float* stats, const float* gamma, const float* beta,
                  const float* ss, const void* res, void* out, float* ws, int B, int64_t rows_b, int C, int G,
                  hipStream_t stream);
/* Host-only queries of the launch plan (no GPU work): the row chunks per sample of the reduction kernels
 * (cesm_gn_stats, and cesm_gn_bwd's reduction; chunk k covers rows [k r, min(rows_b, (k + 1) r)) with
 * r = ceil(rows_b / chunks), so a trailing chunk can be ragged or empty) and of the streaming kernels (cesm_gn_apply,
 * cesm_gn_bwd's apply pass; `rows` = rows_b, or the window's row_n for cesm_gn_apply_rows).  These are what the
 * launchers themselves call.  -1 for a size < 1 or a C the forward refuses.  Added entry points (no existing argument
 * list changed): the ABI version stays, as for cesm_stem_dgrad. */
int cesm_gn_nchunk(int64_t rows_b, int C, int B);
int cesm_gn_apply_nchunk(int64_t rows, int C);
/* backward; also writes the producing conv's bias gradient dbias (+)= sum dy (nullable) without another
 * pass over dy.  ws >= max(B*1024, 1024)*C*3 + B*C*3 + B*C*5 floats (max(B*256, 1024) suffices in the default
 * build; builds with -DGN_BIGB_CAP=512/1024 or -DGN_PER_SAMPLE=1 use up to 1024 chunk partials per sample).
 * Width rule: C / 8 must be a power of two and <= 128 (the reduction adds the lanes that share a channel vector with
 * xor shuffles), C / G one of 8, 16, 32, 64 and G <= 64; any other width returns CESM_EINVAL.  The forward
 * (cesm_gn_stats, cesm_gn_apply) is wider: any C % 8 == 0 up to 2048 with (C / G) % 8 == 0, C = 192 included.
 * dss, dgamma, dbeta and dbias are each nullable (then not written); accumulate = 0 overwrites the three parameter
 * gradients, 1 adds to them; dss is always overwritten.  The workspace need not be initialised. */
int cesm_gn_bwd(int dtype, const void* dout, const void* y, const float* stats, const float* gamma,
                const float* beta, const float* ss, void* dy, float* dss, float* dgamma, float* dbeta, float* dbias,
                float* ws, int B, int64_t rows_b, int C, int G, int accumulate, hipStream_t stream);
/* Row-window forms for the tail of the network, where only the centre frame reaches the head: the window is rows
 * [row_lo, row_lo + row_n) of every sample's rows_b (frame f: row_lo = f*H*W, row_n = H*W).  y (and dy) are the full
 * [B][rows_b][C] tensors with the statistics of all rows; the tensors that matter only inside the window are compact
 * [B][row_n][C].  cesm_gn_apply_rows reads only the window rows of y and writes only out_c (res_c nullable), with
 * cesm_gn_apply's arithmetic.  cesm_gn_bwd_rows takes the compact dout_c of a dout that is zero outside the window
 * and writes the dense dy and the same dss / dgamma / dbeta / dbias (each nullable) as cesm_gn_bwd would on the
 * zero-padded dout, bit for bit up to the sign of a zero: rows outside the window read y, never dout_c.  ws as for the dense
 * calls.  (Added without a CESM_ABI_VERSION bump: no existing argument list changed.) */
int cesm_gn_apply_rows(int dtype, const void* y, const float* stats, const float* gamma, const float* beta,
                       const float* ss, const void* res_c, void* out_c, float* ws, int B, int64_t rows_b, int C, int G,
                       int64_t row_lo, int64_t row_n, hipStream_t stream);
int cesm_gn_bwd_rows(int dtype, const void* dout_c, const void* y, const float* stats, const float* gamma,
                     const float* beta, const float* ss, void* dy, float* dss, float* dgamma, float* dbeta,
                     float* dbias, float* ws, int B, int64_t rows_b, int C, int G, int64_t row_lo, int64_t row_n,
                     int accumulate, hipStream_t stream);
/* channel LayerNorm (biased var, gamma only): video_net.py:78-87.  perm_f > 0: x is [B][perm_f][perm_hw] voxels and
 * out is written pixel-major ([B][perm_hw][perm_f], the long-window qkv order); 0: same order as x */
int cesm_ln_fwd(int dtype, const void* x, const float* gamma, void* out, float* mr, int64_t V, int C, float eps,
                int perm_f, int perm_hw, hipStream_t stream);
/* dx = LN backward + dres (the Residual wrapper's pass-through gradient, video_net.py:75); perm_f > 0: dy is
 * pixel-major (as cesm_ln_fwd's permuted out) */
int cesm_ln_bwd(int dtype, const void* dy, const void* x, const float* mr, const float* gamma, const void* dres,
                void* dx, float* dgamma, float* part, int nblk, int64_t V, int C, int accumulate, int perm_f, int perm_hw,
                hipStream_t stream);

/* ---- temporal-convolution blocks (csrc/tconv.h, included from norm.hip) ---------------------
 * Residual(PreNorm(TemporalCNN)) of UNet(use_temp_attn=False): n = LN_C(x) * gamma (biased variance),
 *   y[b,f,p,:] = x[b,f,p,:] + bias + sum_k W[:,:,k] n[b,f+k-1,p,:]      (n = 0 for frames outside 0 .. F-1)
 * x, y, dy, dx [B*F][HW][C] of `dtype`, C in {64, 128, 256} (cesm_tconv_supported; else CESM_EUNSUPPORTED), any
 * F >= 1 and HW >= 1.  wp / wpt: the Conv1d weight [C][C][3] packed by cesm_conv_pack(dtype, w, out, C, C, 1, 3, s, s)
 * with s = 0 (wp, forward) and s = 1 (wpt, swapped and flipped: backward).  mr [B*F*HW][2] (mean, rstd): written by
 * the forward when non-null, read by the backward.  ws / ws_n / ws_dn: [B*F*HW][C] of dtype, fp32 path only (bf16:
 * ignored, may be null).
 * Backward: dx = LN backward of dn = sum_k W[:,:,k]^T dy[b,f-k+1,p,:], + dy; dgamma [C], dw [C][C][3] (the Conv1d
 * weight's layout), db [C] fp32, each (+)= and each nullable (then not computed, nothing written for it).  part /
 * slab: fp32 workspaces of cesm_tconv_part_floats / cesm_tconv_slab_floats elements (0 = unsupported shape); part is
 * needed when dgamma or db is asked for (fp32 path: always), slab when dw is.  Every reduction is over fixed-order
 * partial sums (no atomics): results are bit-repeatable.  bf16 runs MFMA kernels (one read of x and one write of y in
 * the forward); fp32 is the parity path (LayerNorm kernels + plain FMA). */
int cesm_tconv_supported(int C);
int64_t cesm_tconv_part_floats(int dtype, int B, int F, int HW, int C);
int64_t cesm_tconv_slab_floats(int dtype, int B, int F, int HW, int C);
int cesm_tconv_fwd(int dtype, const void* x, const float* gamma, const void* wp, const float* bias, void* y, float* mr,
                   void* ws, int B, int F, int HW, int C, float eps, hipStream_t stream);
int cesm_tconv_bwd(int dtype, const void* x, const void* dy, const float* mr, const float* gamma, const void* wpt, void* dx,
                   float* dgamma, float* dw, float* db, float* part, float* slab, void* ws_n, void* ws_dn, int B, int F,
                   int HW, int C, float eps, int accumulate, hipStream_t stream);

/* ---- attention (csrc/attn.hip) -----------------------------------------------------------
 * RoPE angle table (rotary_embedding.py:143-144, :275-278): rot[f][i] = (cos, sin)(f*freqs[i]). */
int cesm_rope_table(const float* freqs, float* rot, int F, hipStream_t stream);
/* RelativePositionBias (video_net.py:268-310): bias[h][i][j] = table[bucket(j-i)][h] and backward. */
int cesm_relpos_fwd(const float* table, float* bias, int F, int heads, int num_buckets, int max_distance,
                    hipStream_t stream);
int cesm_relpos_bwd(const float* part, int nparts_per_h, int B, float* dtable, float* ws, int F, int heads,
                    int num_buckets, int max_distance, int accumulate, hipStream_t stream);
/* temporal attention core (video_net.py:401-453 between to_qkv and to_out), qkv [V][768] -> out [V][256] */
int cesm_tattn_nblk(int F, int HW);
int cesm_tattn_fwd(int dtype, const void* qkv, const float* bias, const float* rot, void* out, float* lse, int B,
                   int F, int HW, float scale, hipStream_t stream);
int cesm_tattn_bwd(int dtype, const void* qkv, const void* o, const void* dout, const float* lse, const float* bias,
                   const float* rot, void* dqkv, float* dbias_part, int B, int F, int HW, float scale,
                   hipStream_t stream);
/* Temporal-attention core on MFMA (bf16, csrc/tflash.hip; F <= 128): same contract as cesm_tattn_fwd /
 * cesm_tattn_bwd (video_net.py:403-454) for the unfused path (long windows, C >= 256 levels).  fwd: qkv
 * [B*F*HW][768] -> out [..][256], lse [B][8][HW][F] (log2 units, nullable); bias [8][F][F], rot [F][16][2].
 * bwd: dqkv [..][768] from qkv, o (the forward's out), lse, dout [..][256]; dtable (+)= the rel-pos table
 * gradient (nullable).  Workspaces: dbuf B*8*HW*F, part B*8*cesm_tflash_nblk(HW)*(2F-1), off 8*(2F-1) floats.
 * Round 5 (same argument lists, CESM_ABI_VERSION unchanged): F >= 8 runs the one-pass fused backward (dbuf then
 * unused; CESM_TF_FUSED=0 in the environment restores the dq + dk / dv kernels), and cesm_tflash_nblk returns 128
 * for every HW (the fused kernel's pixel streams per (sample, head)) -- size part from it, not from a formula. */
int cesm_tflash_supported(int F);
int cesm_tflash_nblk(int HW);
/* name of the backward kernel (the fused one, or the dq kernel of the two-kernel form) cesm_tflash_bwd runs for
 * (F, HW) (host-only query) */
const char* cesm_tflash_bwd_variant(int F, int HW);
/* ND of the tflash_bwd_fused_kernel<NT, ND> cesm_tflash_bwd instantiates (NT = ceil(F / 16)): NT - 1 exact
 * bias-gradient diagonals per side, or 2 (saturated accumulators) for NT >= 4 when every offset beyond two diagonals
 * falls into the bucket of +-(F - 1); -1 when no fused kernel runs (F < 8, or F unsupported).  Host-only query. */
int cesm_tflash_bwd_nd(int F, int num_buckets, int max_distance);
/* qkv_pixel_major (F > 16): qkv / dqkv rows ordered [B][HW][F] (a pixel's frames adjacent: the long-window path's
 * LN writes its output in that order, so the to_qkv GEMM produces it); out / dout / lse keep their layouts */
int cesm_tflash_fwd(const void* qkv, const float* bias, const float* rot, void* out, float* lse, int B, int F, int HW,
                    float scale, int qkv_pixel_major, hipStream_t stream);
int cesm_tflash_bwd(const void* qkv, const void* o, const void* dout, const float* lse, const float* bias,
                    const float* rot, void* dqkv, float* dtable, float* dbuf, float* part, float* off, int B, int F,
                    int HW, float scale, int num_buckets, int max_distance, int accumulate, int qkv_pixel_major,
                    hipStream_t stream);
/* Fused temporal-attention block forward, bf16 (csrc/tblock.hip): y = x + Residual(PreNorm(Attention))
 * (video_net.py:69-98, :350-454) with LN, QKV GEMM, RoPE, MFMA core, out-proj in one kernel; x,y
 * [B*F*HW][C], wqkv [768][C], wout [C][256] packed bf16; saves mr [B*F*HW][2] and lse [B][8][HW][F].
 * F <= 16, C in {64,128,256,512}. */
int cesm_tblock_fwd(const void* x, const float* gamma, const void* wqkv, const void* wout, const float* bias,
                    const float* rot, void* y, float* mr, float* lse, void* o, void* wimg, int B, int F, int HW, int C,
                    float scale, float eps, hipStream_t stream);
/* Fused temporal-attention block backward, dx path (bf16): recomputes LN/QKV/RoPE/softmax from mr and
 * lse, dO = dy.W_out, MFMA core backward, dxn = dqkv.W_qkv, LN backward + residual -> dx.  Emits
 * (nullable) dqkv [..][768], o [..][256], xn [..][C] bf16 for the to_qkv/to_out weight gradients,
 * dbias_part [B][8][nblk][F][F] (cesm_relpos_bwd layout) and dgamma (+)= sum dxn*xhat.
 * wqkv_t [C][768] and wout_t [256][C] are the swap-packed weights; nblk from cesm_tblock_bwd_nblk. */
int cesm_tblock_bwd_nblk(int B, int F, int HW, int C);
/* (cesm_tblock_fwd's o, nullable, C <= 256: the attention output O [..][256] bf16 before to_out, written
 * by the forward for the to_out weight gradient; the backward's o is then passed null.) */
int cesm_tblock_bwd(const void* x, const void* dy, const float* gamma, const float* mr, const float* lse,
                    const void* wqkv, const void* wqkv_t, const void* wout_t, const float* bias, const float* rot,
                    void* dx, void* dqkv, void* o, void* xn, float* dbias_part, float* dgamma, float* dgamma_part, void* wimg,
                    int nblk, int B, int F, int HW, int C, float scale, int accumulate, hipStream_t stream);
/* Fused temporal-attention block with in-kernel weight gradients (C = 64, 4F <= 48; csrc/tblock.hip):
 * cesm_tblock_fwd_fold is cesm_tblock_fwd with LN gamma folded into the QKV weights (wqkv_f32: the fp32
 * master weight [768][C]; wimg (768 + 256) * C bf16); cesm_tblock_bwd_dw is its backward: dx, and
 * dwqkv (+)= dW_qkv, dgamma (+)= the LN gamma gradient (nullable) without the 768-channel dqkv / xn
 * intermediates; dbias_part [8][nblk][F][F] (cesm_relpos_bwd, B = 1); slab nblk*768*C and tmp 768*C floats,
 * wimg (2*768 + 256) * C bf16; nblk from cesm_tblock_bwd_dw_nblk (0 = unsupported shape).  o (nullable) receives the
 * attention output O [..][256] bf16 recomputed from the backward's P (round 6: the forward then writes no O), the input
 * of the to_out weight gradient's wide GEMM.
 * Replaces video_net.py:368-454 (Attention) + :90-98 (PreNorm LN) + :69-75 (Residual) and the
 * to_qkv / to_out weight gradients of its backward. */
int cesm_tblock_bwd_dw_nblk(int B, int F, int HW, int C);
int cesm_tblock_fwd_fold(const void* x, const float* gamma, const float* wqkv_f32, const void* wout,
                         const float* bias, const float* rot, void* y, float* mr, float* lse, void* o, void* wimg,
                         int B, int F, int HW, int C, float scale, float eps, hipStream_t stream);
int cesm_tblock_bwd_dw(const void* x, const void* dy, const float* mr, const float* lse, const float* wqkv_f32,
                       const float* gamma, const void* wout_t, const float* bias, const float* rot, void* dx, void* o,
                       float* dwqkv, float* dgamma, float* dbias_part, float* slab, float* tmp, void* wimg,
                       int nblk, int B, int F, int HW, int C, float scale, int accumulate, hipStream_t stream);
/* Backward of the 768-channel qkv projection with dqkv read once (csrc/qkvbwd.hip, round 6): dx = dy . W (the LN
 * output's gradient, written) and dw (+)= dy^T . x in one pass -- replaces the dgrad GEMM + wide weight-gradient GEMM
 * pair of video_net.py:380-381 / :322-323 (to_qkv) on the unfused attention paths (long windows F > 16, C >= 256).
 * dy [M][768] bf16, x [M][C] bf16 (C = 64 .. 512, C % 64 == 0), wt [C][768] bf16 (wt[c][n] = W[n][c]), dx [M][C] bf16,
 * dw [768][C] fp32 (nullable), slab (C / 64) * streams * 768 * 64 floats with streams = cesm_qkv_bwd_streams (0 =
 * unsupported shape).  Rows may be in any order (pixel- or frame-major) as long as dy, x and dx agree. */
int cesm_qkv_bwd_streams(int64_t M, int N, int C);
int cesm_qkv_bwd(const void* dy, const void* x, const void* wt, void* dx, float* dw, float* slab, int64_t M, int N,
                 int C, int accumulate, hipStream_t stream);
/* spatial linear attention core (video_net.py:335-345 between to_qkv and to_out) */
int cesm_sla_nchunk(int HW);
int cesm_sla_fwd(int dtype, const void* qkv, void* out, float* ctx, float* ml, float* ws, int Nf, int HW, float scale,
                 hipStream_t stream);
int cesm_sla_bwd(int dtype, const void* qkv, const void* dout, const float* ctx, const float* ml, void* dqkv,
                 float* ws, int Nf, int HW, float scale, hipStream_t stream);

/* Fused spatial-linear-attention block (bf16, C = 64; csrc/sla_fused.hip): y = x + Residual(PreNorm(
 * SpatialLinearAttention)) (video_net.py:313-347) without per-pixel intermediates in HBM: online-softmax
 * context partials -> combine -> output.  Saves mz [Nf][8][32][2] (max, normaliser of k over pixels),
 * ctx32 [Nf][8][32][32] and the context as MFMA A fragments actT/actx [Nf][8][2][64][8] bf16.
 * o (nullable): the attention output before to_out [Nf][HW][256] bf16, for the to_out weight gradient
 * (training; the backward then need not emit it).
 * ws: cesm_slaf_nblk(Nf, HW) * Nf * 8 * 1088 floats. */
int cesm_slaf_nblk(int Nf, int HW);
int cesm_slaf_fwd(const void* x, const float* gamma, const void* wqkv, const void* wout, const float* bout, void* y,
                  void* o, float* mz, float* ctx32, void* actT, void* actx, float* ws, int Nf, int HW, int C,
                  float scale, float eps, hipStream_t stream);

/* Fused SLA block backward, dx path (bf16, C = 64): dctx partials -> combine (G_d = sum_e dctx ctx, dctx as
 * A fragments adc/adcT) -> dx (+ dy residual), dgamma (+)=; emits (nullable) dqkv [..][768], o [..][256],
 * xn [..][C] for the to_qkv / to_out weight gradients.  part: nblk*Nf*8*1024 floats, G: Nf*8*64*16 floats,
 * adc/adcT: Nf*8*2*64*8 bf16, dgp: cesm_slaf_bwd_nblk(Nf, HW, C)*C floats;
 * wimg: (2*768 + 256)*C bf16 (fragment images of the three weights, rebuilt per call). */
int cesm_slaf_bwd(const void* x, const void* dy, const float* gamma, const void* wqkv, const void* wqkv_t,
                  const void* wout_t, const float* mz, const float* ctx32, const void* actT, const void* actx,
                  void* dx, void* dqkv, void* o, void* xn, float* dgamma, float* part, float* G, void* adc, void* adcT,
                  float* dgp, void* wimg, int Nf, int HW, int C, float scale, float eps, int accumulate,
                  hipStream_t stream);
/* Fused SLA block backward with in-kernel weight gradients (C = 64): the forward runs cesm_slaf_fwd with
 * gamma_one (unit LN gamma) and wq_fold = bf16 W_qkv diag(gamma) (cesm_pack_scaled); this backward returns
 * dx and accumulates dwqkv (+)= dW_qkv [768][C], dgamma (+)= the LN gamma gradient (nullable) without the
 * 768-channel dqkv / xn intermediates of cesm_slaf_bwd.  nblk_dx from cesm_slaf_bwd_dw_nblk (0 = unsupported);
 * slab nblk_dx*768*C, tmp 768*C floats; wimg (2*768 + 256)*C bf16.  dwout [C][256] / dbout [C] (+)= the to_out
 * weight / bias gradients (both or neither; nullable) from the recomputed q~ and the forward's context, so the
 * forward need not write O: partm (cesm_slaf_nblk + 1) * Nf * 8 * 2048 floats, partb cesm_slaf_nblk * Nf * C.
 * Replaces video_net.py:313-347 (SLA) + :90-98 + :69-75 and the to_qkv / to_out weight gradients of its
 * backward. */
int cesm_slaf_bwd_dw_nblk(int Nf, int HW, int C);
int cesm_slaf_bwd_dw(const void* x, const void* dy, const float* gamma_one, const void* wq_fold, const float* wqkv_f32,
                     const float* gamma, const void* wout_t, const float* mz, const float* ctx32, const void* actT,
                     const void* actx, void* dx, float* dwqkv, float* dgamma, float* dwout, float* dbout, float* part,
                     float* G, void* adc, void* adcT, float* slab, float* tmp, float* partm, float* partb, void* wimg,
                     int nblk_dx, int Nf, int HW, int C, float scale, float eps, int accumulate, hipStream_t stream);
/* out = bf16(w diag(colscale)) for an fp32 row-major w [M][K] (trans = 1: written transposed, [K][M]) */
int cesm_pack_scaled(const float* w, const float* colscale, void* out, int M, int K, int trans, hipStream_t stream);
int cesm_slaf_bwd_nblk(int Nf, int HW, int C);

/* ---- small ops, loss, optimizer, data (csrc/misc.hip) ------------------------------------- */
/* SinusoidalPosEmb (video_net.py:101-113) */
int cesm_sinusoidal(const int64_t* t, float* emb, int B, int dim, hipStream_t stream);
/* y = bias + act(x) W^T, act = SiLU when silu_in (time_mlp video_net.py:651-656, ResnetBlock.mlp :238-242) */
int cesm_linear_small_fwd(const float* x, const float* w, const float* bias, float* y, int R, int I, int O,
                          int silu_in, hipStream_t stream);
int cesm_linear_small_bwd(const float* x, const float* w, const float* dy, float* dx, float* dw, float* db, int R,
                          int I, int O, int silu_in, int accumulate_dx, int accumulate_w, hipStream_t stream);
/* Diffusion.q_sample (model.py:196-201) and F.mse_loss (model.py:208) */
int cesm_q_sample(const float* x0, const float* noise, const int64_t* t, const float* sa, const float* s1a,
                  float* xt, int B, int64_t HW, hipStream_t stream);
/* Diffusion.p_sample DDPM update (model.py:168-183), fused: out = r_t (x - b_t/s1_t eps) + sqrt(pv_t) z,
 * coefficients gathered on device from the schedule buffers by t[B]; z may be null (no noise term);
 * out may alias x.  x, eps, z, out: [B][HW] fp32. */
int cesm_ddpm_step(const float* x, const float* eps, const float* z, const int64_t* t, const float* sqrt_recip_alphas,
                   const float* betas, const float* sqrt_one_minus_ac, const float* posterior_variance, float* out,
                   int B, int64_t HW, hipStream_t stream);
/* Diffusion.ddim_step update (generalized DDIM step of Song et al. 2021, eq. 12; few-step sampling), fused:
 * out = a x + b eps + sigma z, with (a, b, sigma) formed per sample on the device, in double, from
 * alphas_cumprod[t] and alphas_cumprod[t_prev] (t_prev < 0: 1, the step returns the x0 estimate) -- the arithmetic of
 * Diffusion.ddim_coefs.  t, t_prev: [B] device tensors, t_prev[b] < t[b] < T (checked by the caller, not here), t may
 * differ across the batch; eta >= 0 (0: deterministic; 1 with t_prev = t - 1: the DDPM step).  z == NULL or eta == 0:
 * no noise term, z is not read.  out may alias x.  x, eps, z, out: [B][HW] fp32; alphas_cumprod: [T] fp32.
 * An added entry point (no existing argument list changed): the ABI version stays, as for cesm_stem_dgrad. */
int cesm_ddim_step(const float* x, const float* eps, const float* z, const int64_t* t, const int64_t* t_prev,
                   const float* alphas_cumprod, float eta, float* out, int B, int64_t HW, int T, hipStream_t stream);
/* Diffusion.dpmpp_step update: one DPM-Solver++(2M) step (Lu et al. 2022) from t to t_prev < t, with the x0 estimate
 * of the previous executed step (at t_last > t) as history, fused:
 *   out = a x + b eps + c x0_last,   x0_out = c1 x + c2 eps.
 * With ac_u = alphas_cumprod[u], alpha_u = sqrt(ac_u), sigma_u = sqrt(1 - ac_u), lambda_u = log(ac_u / (1 - ac_u)) / 2,
 * formed per sample on the device in double (log and expm1 too) and rounded to fp32 once each -- the arithmetic of
 * Diffusion.dpmpp_coefs:
 *   c1 = 1 / alpha_t,  c2 = -sigma_t / alpha_t                        (the x0 estimate)
 *   t_prev >= 0:  h = lambda_prev - lambda_t,  G = -alpha_prev expm1(-h),
 *                 t_last < 0 (no history):  w_c = 1, w_p = 0          (the DDIM step at eta = 0)
 *                 t_last >= 0:  r = (lambda_t - lambda_last) / h,  w_c = 1 + 1/(2r),  w_p = -1/(2r)
 *                 a = sigma_prev / sigma_t + G w_c / alpha_t,  b = -G w_c sigma_t / alpha_t,  c = G w_p
 *   t_prev < 0 (last step, returns the x0 estimate, never extrapolates):  a = c1, b = c2, c = 0.
 * t, t_prev, t_last: [B] device tensors, -1 <= t_prev[b] < t[b] < T and t_last[b] = -1 or t[b] < t_last[b] < T (the
 * caller's check); every table index formed from them is clamped into 0 ... T-1 here, so a wrong index gives a wrong
 * number, not a read outside the table.  x0_last is read only for samples with t_prev >= 0 and t_last >= 0 and may be
 * NULL when no sample has history.  out may alias x and x0_out may alias x0_last.  x, eps, x0_last, out, x0_out:
 * [B][HW] fp32; alphas_cumprod: [T] fp32.  16-byte accesses where HW % 4 == 0 and all five are 16-byte aligned, else
 * one element per access.  CESM_EINVAL on a null pointer (x0_last apart), B < 1, B > 65535, HW < 1 or T < 1.
 * An added entry point (no existing argument list changed): the ABI version stays, as for cesm_ddim_step. */
int cesm_dpmpp_step(const float* x, const float* eps, const float* x0_last, const int64_t* t, const int64_t* t_prev,
                    const int64_t* t_last, const float* alphas_cumprod, float* out, float* x0_out, int B, int64_t HW,
                    int T, hipStream_t stream);
/* Classifier-free guidance (Ho & Salimans 2022): the three updates above with the combine of a conditional and an
 * unconditional network evaluation fused in,
 *   g = eps_u + scale (eps_c - eps_u),  formed as fma(scale, eps_c - eps_u, eps_u): one rounded subtraction, one FMA;
 * everything after it is the unguided kernel's own code with g in the place of eps (equal halves, eps_u == eps_c, give
 * the unguided result bit for bit at every scale).  Arguments are those of the unguided entry plus `scale`, a finite
 * number >= 0 (1: the conditional model, 0: the unconditional one).  B counts SAMPLES; x, eps and out have 2 B rows:
 * rows [0, B) of eps are eps_c (evaluated on cond), rows [B, 2B) eps_u (evaluated on the null condition, an all-zero
 * cond); x is read from rows [0, B) only, and x_prev is written to row b and to row b + B, so the next network
 * evaluation finds both halves equal without a copy.  z, x0_last, x0_out, t, t_prev and t_last have B rows / entries.
 * Aliasing, null z / x0_last, index clamps, the 16-byte path and the B / HW / T checks: as the unguided entries.
 * CESM_EINVAL also on a scale that is negative or not finite and on a null pointer (z and x0_last apart).
 * Added entry points (no existing argument list changed): the ABI version stays, as for cesm_ddim_step. */
int cesm_ddpm_step_cfg(const float* x, const float* eps, const float* z, const int64_t* t,
                       const float* sqrt_recip_alphas, const float* betas, const float* sqrt_one_minus_ac,
                       const float* posterior_variance, float* out, int B, int64_t HW, float scale,
                       hipStream_t stream);
int cesm_ddim_step_cfg(const float* x, const float* eps, const float* z, const int64_t* t, const int64_t* t_prev,
                       const float* alphas_cumprod, float eta, float* out, int B, int64_t HW, int T, float scale,
                       hipStream_t stream);
int cesm_dpmpp_step_cfg(const float* x, const float* eps, const float* x0_last, const int64_t* t,
                        const int64_t* t_prev, const int64_t* t_last, const float* alphas_cumprod, float* out,
                        float* x0_out, int B, int64_t HW, int T, float scale, hipStream_t stream);
/* Condition dropout of guidance training: out[b][:] = keep[b] ? cond[b][:] : 0 for b < B.  cond, out: [B][n] fp32, n
 * the elements of one sample ([V][H][W] or a window [V][Fc][H][W]); keep: [B] bytes (a torch.bool tensor), non-zero
 * keeps.  A select, not a multiply: a dropped sample's cond is not read, so a NaN or Inf there does not reach out, and
 * its out is +0.  out may alias cond.  16-byte accesses where n % 4 == 0 and both are 16-byte aligned, else one element
 * per access.  CESM_EINVAL on a null pointer, B < 1, B > 65535 or n < 1. */
int cesm_cond_mask(const float* cond, const unsigned char* keep, float* out, int B, int64_t n, hipStream_t stream);
int cesm_mse(const float* pred, const float* tgt, float* loss, float* part, int64_t n, hipStream_t stream);
int cesm_mse_bwd(const float* pred, const float* tgt, const float* gscale, float* dpred, int64_t n,
                 hipStream_t stream);
/* Weighted loss: latitude (row) weights and per-sample weights on the one squared-error sum.  pred, noise: [B][V][H][W]
 * fp32, d = pred - noise, n = B V H W; w: [Hg] fp32 row weights of the full grid, Hg >= H; row0: [B] int64, the grid
 * row of each sample's row 0 (NULL: all 0); a: [B] fp32 per-sample weights (NULL: all 1); lam in [0, 1].
 * With c(b, h) = (1 - lam) + lam w[row0[b] + h], formed once per row in fp32:
 *   out[0] = mse_raw = (1/n) sum d^2,  out[1] = mse_lat = (1/n) sum w[row0[b] + h] d^2,
 *   out[2] = total = (1/n) sum a[b] c(b, h) d^2;   cesm_wloss_bwd: dpred = gscale[0] (2/n) a[b] c(b, h) d.
 * The row index row0[b] + h is clamped into [0, Hg - 1] before w is read: a wrong offset gives a wrong number, not a
 * read outside w.  Deterministic: no atomics; part (512 * 3 floats) takes three fp32 partials per block, which a
 * second kernel (one wave) adds in double in a fixed order.  Two launches forward, one backward.  16-byte accesses where
 * W % 4 == 0 and pred, noise (and dpred) are 16-byte aligned, else one element per access.  CESM_EINVAL on a null
 * pointer (row0 and a excepted), a size < 1, Hg < H or lam outside [0, 1].
 * Added entry points (no existing argument list changed): the ABI version stays, as for cesm_stem_dgrad. */
int cesm_wloss(const float* pred, const float* noise, const float* w, const int64_t* row0, const float* a, float lam,
               float* out, float* part, int B, int V, int H, int W, int Hg, hipStream_t stream);
int cesm_wloss_bwd(const float* pred, const float* noise, const float* w, const int64_t* row0, const float* a,
                   float lam, const float* gscale, float* dpred, int B, int V, int H, int W, int Hg,
                   hipStream_t stream);
/* Ensemble verification statistics in one pass over the ensemble (csrc/ensemble.hip).
 * ens: [B][M][V][H][W] fp32, contiguous, member m of
 * condition b = row b M + m of a sampler batch, 2 <= M <= 128; obs: [B][V][H][W] fp32 or NULL; w: [Hg] fp32 row weights,
 * Hg >= H; row0: [B] int64 grid row of each condition's row 0 (NULL: all 0).  Per pixel, evaluated in fp32 in this form
 * (the order of summation within a pixel is fixed but unspecified):
 *   s = sum_m x_m,  mean = s / M;   q = sum_m (x_m - mean)^2,  var = q / (M - 1)   (two passes, never sum x^2 - s^2 / M)
 *   A = sum_m |x_m - y|,  P = sum_{i<j} |x_i - x_j|,  crps = A / M - P / (M (M - 1))   (fair CRPS, Ferro 2014)
 *   rank = #{m : x_m < y} in [0, M], ties count as not-less.
 * Outputs, each nullable: maps mean, var, crps (fp32) and rank (int32), [B][V][H][W]; crps and rank need obs.  acc:
 * double [V][4 + M + 1]; row v = sums over that variable's b, h, w, with w_r = w[clamp(row0[b] + h, 0, Hg - 1)], of
 *   w_r,  w_r (mean - y)^2,  w_r var,  w_r crps,  w_r [rank = r] for r = 0 .. M;
 * without obs only columns 0 and 2 are written, the rest of the row is left as found.  accumulate != 0: acc += the
 * sums, else acc = the sums.  part: workspace of 2048 (4 + M + 1) floats, needed with acc.
 * The row index is clamped before w is read: a wrong offset gives a wrong number, never a read outside w.
 * Deterministic: no float atomics; per block fp32 partials in which a row's weight meets that row's sum once and rank
 * counts are integers until then; the blocks' partials are added in double in a fixed order by a second kernel (one
 * wave per accumulator entry).  ens is read once, 16 bytes per lane where W % 4 == 0 and ens is 16-byte aligned, else
 * 4; any W.  P is formed pairwise from LDS (the source has the layout); M is a run-time value and nothing is
 * padded.  Non-finite inputs may give non-finite outputs; rank stays in [0, M].
 * CESM_EINVAL: ens or w null, M outside 2 .. 128, a size < 1, Hg < H, crps or rank without obs, acc without part, or
 * no output at all.  An added entry point (no existing argument list changed): the ABI version stays. */
int cesm_ens_stats(const float* ens, const float* obs, const float* w, const int64_t* row0, float* mean, float* var,
                   float* crps, int* rank, double* acc, float* part, int B, int M, int V, int H, int W, int Hg,
                   int accumulate, hipStream_t stream);
/* clip_grad_norm_ (train.py:865; torch/nn/utils/clip_grad.py:165-180) over a flat grad buffer;
 * info = {norm, clamped clip coef, finite(loss & norm)} stays on device (no host sync). */
int cesm_grad_norm(const float* g, int64_t n, float max_norm, const float* loss, double* part, float* info,
                   hipStream_t stream);
/* AdamW step (train.py:1077-1083, torch/optim/adam.py:417-547) over flat buffers; skipped on device
 * when info[2] == 0 (non-finite), applies the clip coefficient info[1] when use_clip.  step: device int
 * step counter, advanced on device only for a finite step (info[3] <- the step number used for the bias
 * corrections), so a skipped step leaves the count consistent with exp_avg / exp_avg_sq. */
int cesm_adamw(float* p, float* g, float* m, float* v, float* info, int* step, int64_t n, float lr, float b1,
               float b2, float eps, float wd, int use_clip, hipStream_t stream);
/* cesm_adamw plus an exponential moving average of the weights in the same pass over the flat buffers: p, g, m, v
 * and step come out bit-identical to cesm_adamw's, and ema[i] <- ema[i] + omd (p_new[i] - ema[i]) in fp32 from the
 * parameter value just written (no second read of p, no further launch).  For a finite step (info[2] != 0) the
 * single-thread pre-kernel advances step / info[3] as cesm_adamw does, sets n = ++ema_n[0] (device count of EMA
 * updates) and stores ema_omd[0] = (float)(1 - d), d = warmup ? min(beta, (1 + n) / (10 + n)) : beta in double; a
 * skipped step leaves p, m, v, step, ema and ema_n untouched.  ema: [n] fp32; ema_n: device int; ema_omd: device
 * scratch for one float; 0 <= beta < 1 (checked by the caller).  Any n >= 1 and any 4-byte alignment (128-bit
 * accesses only where all five buffers are 16-byte aligned).  CESM_EINVAL on a null pointer or n < 1.
 * An added entry point (no existing argument list changed): the ABI version stays, as for cesm_stem_dgrad. */
int cesm_adamw_ema(float* p, float* g, float* m, float* v, float* info, int* step, int64_t n, float lr, float b1,
                   float b2, float eps, float wd, int use_clip, float* ema, int* ema_n, float* ema_omd, float beta,
                   int warmup, hipStream_t stream);
/* out = a + b (gradient sums at residual / skip fan-outs) */
int cesm_add(int dtype, const void* a, const void* b, void* out, int64_t n, hipStream_t stream);
/* Strided frame copy (csrc/misc.hip): gather copies rows [row_lo, row_lo + row_n) of every sample of src
 * [B][rows_b][C] into the compact dst [B][row_n][C]; scatter copies the compact src over those rows of the full dst
 * and touches no other row.  No host synchronisation (capture-safe).  C * element size must be a multiple of 16
 * bytes and both pointers 16-byte aligned, else CESM_EINVAL.  (Added without a CESM_ABI_VERSION bump.) */
int cesm_rows_gather(int dtype, const void* src, void* dst, int B, int64_t rows_b, int64_t row_lo, int64_t row_n, int C,
                     hipStream_t stream);
int cesm_rows_scatter(int dtype, const void* src, void* dst, int B, int64_t rows_b, int64_t row_lo, int64_t row_n, int C,
                      hipStream_t stream);
int cesm_cast(int dtype_in, int dtype_out, const void* x, void* y, int64_t n, hipStream_t stream);
/* WindowedAllMembersDataset_random.__getitem__ gather (dataset_single_member.py:168-196);
 * items: nitems x {t0, m, anchor, reverse, crop_i, crop_j} int64 */
int cesm_window_gather(const float* cond, const float* tgt, const int64_t* items, float* cwin, float* x0,
                       int nitems, int K, int M, int H, int W, int h, int w, int center, hipStream_t stream);
/* The same gather for V target variables and explicit frame indices (dataset_single_member.py:104-196: _choose_times,
 * the crop and __getitem__; csrc/misc.hip), 1 <= V <= 4:
 *   cond [T][M][Vc][H][W], tgt [T][M][V][H][W] fp32 (the reference's (T, M, C, H, W));
 *   csel0 .. csel3: csel[v] in [0, Vc), by value, names the forcing plane that feeds cond channel v (entries >= V are
 *   ignored; one forcing and two targets: Vc = 1, csel = (0, 0));
 *   times int64 [nitems][K]: the frame indices of each item, in output order; meta int64 [nitems][4]: (member m,
 *   anchor, crop i, crop j); both device pointers.
 *   cwin[n][v][k][y][x] = cond[times[n][k]][m][csel[v]][i + y][j + x]     cwin [nitems][V][K][h][w]
 *   x0[n][v][y][x]      = tgt[anchor][m][v][i + y][j + x]                 x0   [nitems][V][h][w]
 * Time reversal and the random sample modes are a different `times` row (the host permutes it): there is no reverse or
 * centre argument.  times and anchor are clamped into [0, T - 1], m into [0, M - 1], i into [0, H - h] and j into
 * [0, W - w] before any address is formed, all offsets 64-bit: a bad index gives a wrong number, never a read outside
 * the arrays.  One launch writes both outputs, one writer per element, no atomics.  16-byte stores where w % 4 == 0 and
 * cwin, x0 are 16-byte aligned (the source start j is arbitrary: 16-byte loads only for a row that is aligned), else
 * one element per access.  CESM_EUNSUPPORTED for V outside 1 .. 4, a csel[v] outside [0, Vc), h > H, w > W or K < 1;
 * CESM_EINVAL on a null pointer or another size < 1.  (Added without a CESM_ABI_VERSION bump: no existing argument
 * list changed.) */
int cesm_window_gather_mv(const float* cond, const float* tgt, const int64_t* times, const int64_t* meta, float* cwin,
                          float* x0, int nitems, int K, int V, int Vc, int csel0, int csel1, int csel2, int csel3,
                          int T, int M, int H, int W, int h, int w, hipStream_t stream);
/* cesm_window_gather_mv with the cond plane count Cc separated from V (multi-forcing conditioning), 1 <= V, Cc <= 4:
 *   csel0 .. csel3: csel[c] in [0, Vc) names the forcing plane that feeds cond channel c < Cc (entries >= Cc ignored);
 *   cwin[n][c][k][y][x] = cond[times[n][k]][m][csel[c]][i + y][j + x]     cwin [nitems][Cc][K][h][w]
 *   x0[n][v][y][x]      = tgt[anchor][m][v][i + y][j + x]                 x0   [nitems][V][h][w]
 * Work units are (n, plane in Cc K + V, y).  Clamping, 64-bit offsets, the vector / element paths and the return codes
 * are those of cesm_window_gather_mv (CESM_EUNSUPPORTED also for Cc outside 1 .. 4).  (Added entry point: the ABI
 * version stays.) */
int cesm_window_gather_mc(const float* cond, const float* tgt, const int64_t* times, const int64_t* meta, float* cwin,
                          float* x0, int nitems, int K, int V, int Cc, int Vc, int csel0, int csel1, int csel2,
                          int csel3, int T, int M, int H, int W, int h, int w, hipStream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* CESM_HIP_H */
