"""Thin tensor-level wrappers over libcesm_hip.so (one C call each, no torch compute).

Every wrapper takes torch tensors living on the current HIP device, allocates its outputs and
workspaces through the PyTorch caching allocator (plumbing) and enqueues the kernel on
torch's current stream.  Shapes are asserted on the host before launch so a bad call raises
instead of faulting on the GPU.
"""
from __future__ import annotations

import math
import numbers
import os

import torch

from ._lib import KernelError, call, lib

F32, BF16 = 0, 1
_DT = {torch.float32: F32, torch.bfloat16: BF16}


def dtcode(t: torch.Tensor) -> int:
    try:
        return _DT[t.dtype]
    except KeyError:
        raise TypeError(f"unsupported dtype {t.dtype}") from None


def S():
    return torch.cuda.current_stream().cuda_stream


def P(t):
    return 0 if t is None else t.data_ptr()


def _chk(t, shape=None, dtype=None):
    if t is None:
        return
    if not t.is_cuda:
        raise RuntimeError("cesm_emulator_amd kernels need device tensors (no CPU fallback)")
    if not t.is_contiguous():
        raise RuntimeError("expected a contiguous tensor")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise RuntimeError(f"shape mismatch: got {tuple(t.shape)}, expected {tuple(shape)}")
    if dtype is not None and t.dtype != dtype:
        raise RuntimeError(f"dtype mismatch: got {t.dtype}, expected {dtype}")


def empty(shape, dtype, device):
    return torch.empty(shape, dtype=dtype, device=device)


# ------------------------------------------------------------------------------------ conv
def conv_pack(w: torch.Tensor, dtype, cout, cin, kh, kw, swap, flip):
    _chk(w, dtype=torch.float32)
    out = empty((cout, kh * kw * cin), dtype, w.device)
    call("cesm_conv_pack", _DT[dtype], P(w), P(out), cout, cin, kh, kw, int(swap), int(flip), S())
    return out


def conv_pack_into(w, out, cout, cin, kh, kw, swap, flip):
    """re-pack into an existing GEMM-layout buffer"""
    _chk(w, dtype=torch.float32)
    call("cesm_conv_pack", _DT[out.dtype], P(w), P(out), cout, cin, kh, kw, int(swap), int(flip), S())
    return out


def pack_blocks(cout, cin, kh, kw):
    """blocks cesm_conv_pack_batch gives one job (host-only query; the kernel's own tiling, csrc/conv_pack.hip)"""
    n = lib().cesm_conv_pack_blocks(int(cout), int(cin), int(kh), int(kw))
    if n < 0:
        raise ValueError(f"conv pack job {cout} x {cin} x {kh} x {kw}: more than 64 taps (or an empty weight) does not "
                         "fit cesm_conv_pack_batch's tile")
    return n


def conv_pack_table(rows, device):
    """device job table of cesm_conv_pack_batch: rows [src ptr, dst ptr, Cout, Cin, KH, KW, swap, flip], then the
    per-job block starts (exclusive prefix of pack_blocks), then the job index of every block; returns (table, nblocks)"""
    if not rows:
        raise ValueError("conv_pack_table: no jobs")
    starts, bjob = [0], []
    for j, r in enumerate(rows):
        n = pack_blocks(r[2], r[3], r[4], r[5])
        starts.append(starts[-1] + n)
        bjob += [j] * n
    flat = [v for r in rows for v in r] + starts + bjob
    return torch.tensor(flat, dtype=torch.int64).to(device), starts[-1]


def conv_pack_batch(jobs_dev, njobs, dtype, nblocks):
    """one launch re-packing every job of a conv_pack_table (see cesm_conv_pack_batch)"""
    call("cesm_conv_pack_batch", _DT[dtype], P(jobs_dev), int(njobs), int(nblocks), S())


_QUEUES = {}


def work_queue():
    """the caller-owned int32[2] work counter of the persistent convs' dynamic item claiming (cesm_conv_fwd's queue):
    one per (device, stream) -- launches on one stream run in order, so they share it.  cesm_conv_fwd zeroes it with a
    stream-ordered memset before every launch that uses it (round 6, ADVICE r5: a launch cut short can no longer leave
    a stale count that makes the next one skip its items).  Not allocated during graph capture (the allocation would
    belong to the graph's private pool): a capture that finds no counter for its stream gets the static item split, as
    does CESM_CONV_STATIC=1."""
    if STATIC_CONV:
        return 0
    st = torch.cuda.current_stream()
    key = (st.device.index, st.cuda_stream)
    q = _QUEUES.get(key)
    if q is None:
        if torch.cuda.is_current_stream_capturing():
            return 0
        q = _QUEUES[key] = torch.zeros(4, dtype=torch.int32, device=st.device)
    return q.data_ptr()


STATIC_CONV = os.environ.get("CESM_CONV_STATIC", "0") == "1"


def conv_fwd(x1, x2, wp, bias, geom, res=None, res2=None, out_split=None):
    """geom = (Ho, Wo, Cout, KH, KW, S, P, U).  Returns y (or (y1, y2) when out_split=Co1)."""
    Ho, Wo, Cout, KH, KW, St, Pd, U = geom
    Nb, Hi, Wi, C1 = x1.shape
    C2 = 0 if x2 is None else x2.shape[3]
    _chk(x1)
    if x2 is not None:
        _chk(x2, (Nb, Hi, Wi, C2), x1.dtype)
    _chk(wp, (Cout, KH * KW * (C1 + C2)), x1.dtype)
    if bias is not None:
        _chk(bias, (Cout,), torch.float32)
    Co1 = Cout if out_split is None else out_split
    y1 = empty((Nb, Ho, Wo, Co1), x1.dtype, x1.device)
    y2 = empty((Nb, Ho, Wo, Cout - Co1), x1.dtype, x1.device) if Co1 != Cout else None
    _chk(res, (Nb, Ho, Wo, Co1), x1.dtype)
    _chk(res2, (Nb, Ho, Wo, Cout - Co1), x1.dtype)
    call("cesm_conv_fwd", dtcode(x1), P(x1), P(x2), P(wp), P(bias), P(res), P(res2), P(y1), P(y2), Nb, Hi, Wi, C1,
         C2, Ho, Wo, Cout, Co1, KH, KW, St, Pd, U, work_queue(), S())
    if CONV_TRACE is not None:
        CONV_TRACE.append(("fwd", Nb, Hi, Wi, C1 + C2, Ho, Wo, Cout, KH, KW, St, Pd, U))
    return y1 if y2 is None else (y1, y2)


def conv_gn_nslot(x1, x2, geom, B):
    """GroupNorm partial slots per sample cesm_conv_fwd_gn writes for this conv (0: the kernel has none)"""
    Ho, Wo, Cout, KH, KW, St, Pd, U = geom
    Nb, Hi, Wi, C1 = x1.shape
    C2 = 0 if x2 is None else x2.shape[3]
    return int(lib().cesm_conv_gn_nslot(dtcode(x1), Nb, Hi, Wi, C1, C2, Ho, Wo, Cout, KH, KW, St, Pd, U, B))


def conv_fwd_gn(x1, x2, wp, bias, geom, B, nslot):
    """conv_fwd of a Block conv (video_net.py:215) that also writes the GroupNorm statistics partials of its
    output (per sample, slot and channel quad: sum, sum of squares); returns (y, part) for gn_stats_part"""
    Ho, Wo, Cout, KH, KW, St, Pd, U = geom
    Nb, Hi, Wi, C1 = x1.shape
    C2 = 0 if x2 is None else x2.shape[3]
    _chk(x1)
    if x2 is not None:
        _chk(x2, (Nb, Hi, Wi, C2), x1.dtype)
    _chk(wp, (Cout, KH * KW * (C1 + C2)), x1.dtype)
    if bias is not None:
        _chk(bias, (Cout,), torch.float32)
    y = empty((Nb, Ho, Wo, Cout), x1.dtype, x1.device)
    part = empty((B, nslot, Cout // 4, 2), torch.float32, x1.device)
    call("cesm_conv_fwd_gn", dtcode(x1), P(x1), P(x2), P(wp), P(bias), P(y), P(part), B, Nb, Hi, Wi, C1, C2, Ho, Wo,
         Cout, KH, KW, St, Pd, U, work_queue(), S())
    if CONV_TRACE is not None:
        CONV_TRACE.append(("fwd", Nb, Hi, Wi, C1 + C2, Ho, Wo, Cout, KH, KW, St, Pd, U))
    return y, part


def qkv_bwd_supported(M, C):
    return lib().cesm_qkv_bwd_streams(int(M), 768, int(C)) > 0


def qkv_bwd(dy, x, wt, dw, accumulate=True):
    """backward of the 768-channel qkv projection, dqkv read once (csrc/qkvbwd.hip): returns dx [..., C] (the LN
    output's gradient); dw [768, C] fp32 (+)= dy^T x (nullable).  dy [..., 768], x [..., C] bf16 with the same rows;
    wt [C, 768] bf16 = the weight transposed (conv_pack(w, bf16, C, 768, 1, 1, 1, 1))."""
    C = x.shape[-1]
    M = x.numel() // C
    _chk(x, dtype=torch.bfloat16)
    _chk(dy, dtype=torch.bfloat16)
    _chk(wt, (C, 768), torch.bfloat16)
    if dy.numel() != M * 768:
        raise RuntimeError(f"qkv_bwd: dy has {dy.numel()} elements, expected {M} x 768")
    ns = lib().cesm_qkv_bwd_streams(M, 768, C)
    if ns <= 0:
        raise ValueError(f"qkv_bwd: unsupported shape M={M} C={C}")
    dev = x.device
    dx = empty(x.shape, torch.bfloat16, dev)
    slab = None
    if dw is not None:
        _chk(dw, dtype=torch.float32)
        if dw.numel() != 768 * C:
            raise RuntimeError("qkv_bwd: dw must hold 768 x C floats")
        slab = empty(((C // 64) * ns * 768 * 64,), torch.float32, dev)
    call("cesm_qkv_bwd", P(dy), P(x), P(wt), P(dx), P(dw), P(slab), M, 768, C, int(accumulate), S())
    return dx


# shape log of conv launches (set CESM_TRACE_CONV=1; tools/conv_shapes.py prints it)
CONV_TRACE = [] if os.environ.get("CESM_TRACE_CONV") else None


def conv_wgrad(x1, x2, dy1, dy2, dw, geom, swap, flip, accumulate=True, db=None):
    """dW of a conv (split-K over pixels + reduce).  db: also the bias gradient (+=) in the same pass when the kernel
    for this shape carries it (cesm_conv_wgrad_bias_rides); returns True if db was produced (else the caller runs
    colsum).  The split count, and with it dW's summation order, is the library's (cesm_conv_wgrad_nsplit)."""
    Ho, Wo, Cout, KH, KW, St, Pd, U = geom
    Nb, Hi, Wi, C1 = x1.shape
    C2 = 0 if x2 is None else x2.shape[3]
    Co1 = dy1.shape[3]
    _chk(dy1, (Nb, Ho, Wo, Co1), x1.dtype)
    _chk(dy2, None if dy2 is None else (Nb, Ho, Wo, Cout - Co1), x1.dtype)
    _chk(dw, dtype=torch.float32)
    geo = (dtcode(x1), Nb, Hi, Wi, C1, C2, Ho, Wo, Cout, Co1, KH, KW, St, Pd, U)
    if db is not None and not lib().cesm_conv_wgrad_bias_rides(*geo):
        db = None
    nsplit = lib().cesm_conv_wgrad_nsplit(*geo, int(db is not None))
    slab = empty((nsplit, Cout, KH * KW * (C1 + C2)), torch.float32, x1.device)
    bslab = None
    if db is not None:
        _chk(db, (Cout,), torch.float32)
        bslab = empty((nsplit, Cout), torch.float32, x1.device)
    if CONV_TRACE is not None:
        CONV_TRACE.append(("wgrad", Nb, Hi, Wi, C1 + C2, Ho, Wo, Cout, KH, KW, St, Pd, U))
    call("cesm_conv_wgrad", dtcode(x1), P(x1), P(x2), P(dy1), P(dy2), P(dw), P(slab), P(db), P(bslab), nsplit, Nb,
         Hi, Wi, C1, C2, Ho, Wo, Cout, Co1, KH, KW, St, Pd, U, int(swap), int(flip), int(accumulate), S())
    return db is not None


def colsum(x, dst, accumulate=True):
    C = x.shape[-1]
    rows = x.numel() // C
    nsplit = int(max(1, min(1024, rows // 512)))
    part = empty((nsplit, C), torch.float32, x.device)
    call("cesm_colsum", dtcode(x), P(x), P(dst), P(part), nsplit, rows, C, int(accumulate), S())


def _mv_call(name, what, *args):
    """a cesm_*_mv entry: CESM_EUNSUPPORTED (-2) is a ValueError that names the shape, any other failure a KernelError"""
    rc = getattr(lib(), name)(*args)
    if rc == -2:
        raise ValueError(f"{name}: unsupported shape {what}")
    if rc != 0:
        raise KernelError(f"{name} failed with code {rc}")


def _stem_io(xt, cond, cin, F):
    """(B, V, Fx, Fc, H, W) of the stem's inputs, checked against the weight's input channels cin = 2V and the frame
    count F.  xt [B, V, Fx, H, W], cond [B, V, Fc, H, W] fp32; at V = 1 the variable axis may be left out."""
    if cin < 2 or cin % 2:
        raise ValueError(f"stem weight with {cin} input channels: expected 2V (x_t and cond of V variables)")
    V = cin // 2
    if xt.ndim == 4 and cond.ndim == 4 and V == 1:
        (B, Fx, H, W), Fc = xt.shape, cond.shape[1]
        _chk(xt, dtype=torch.float32)
        _chk(cond, (B, Fc, H, W), torch.float32)
    else:
        if xt.ndim != 5 or cond.ndim != 5:
            raise ValueError(f"stem inputs must be [B, V, F, H, W], got {tuple(xt.shape)} and {tuple(cond.shape)}")
        B, _, Fx, H, W = xt.shape
        Fc = cond.shape[2]
        _chk(xt, (B, V, Fx, H, W), torch.float32)
        _chk(cond, (B, V, Fc, H, W), torch.float32)
    if Fx not in (1, F) or Fc not in (1, F):
        raise ValueError(f"stem: x_t has {Fx} frames and cond {Fc}; each must be 1 or F = {F}")
    return B, V, Fx, Fc, H, W


def stem_fwd(xt, cond, w, b, F, dtype):
    """stem Conv3d(2V -> Co, (1,KS,KS)) on cat([x_t, cond]): w [Co, 2V, 1, KS, KS] gives V (1 <= V <= 4)"""
    Co, cin, _, KS, _ = w.shape
    B, V, Fx, Fc, H, W = _stem_io(xt, cond, cin, F)
    _chk(w, (Co, cin, 1, KS, KS), torch.float32)
    _chk(b, (Co,), torch.float32)
    y = empty((B * F, H, W, Co), dtype, xt.device)
    _mv_call("cesm_stem_fwd_mv", f"V={V} KS={KS} Co={Co} F={F} Fx={Fx} Fc={Fc}", _DT[dtype], P(xt), P(cond), P(w), P(b),
             P(y), B, V, F, Fx, Fc, H, W, Co, KS, S())
    return y


def stem_wgrad(xt, cond, dy, dw, F, accumulate=True):
    Co, cin, _, KS, _ = dw.shape
    B, V, Fx, Fc, H, W = _stem_io(xt, cond, cin, F)
    _chk(dy, (B * F, H, W, Co))
    _chk(dw, (Co, cin, 1, KS, KS), torch.float32)
    nblk = 512
    part = empty((nblk, Co * cin * KS * KS), torch.float32, xt.device)
    _mv_call("cesm_stem_wgrad_mv", f"V={V} KS={KS} Co={Co} F={F} Fx={Fx} Fc={Fc}", dtcode(dy), P(xt), P(cond), P(dy),
             P(dw), P(part), nblk, B, V, F, Fx, Fc, H, W, Co, KS, int(accumulate), S())


def stem_dgrad(dy, w, B, F, Fx, Fc, want_xt=True, want_cond=True):
    """data gradient of the stem (csrc/stem_head.hip: stem_dgrad.h, multivar.h): dy [B*F, H, W, Co] (what stem_wgrad reads),
    w the fp32 stem weight [Co, 2V, 1, KS, KS].  Returns (dxt [B, V, Fx, H, W], dcond [B, V, Fc, H, W]) fp32 ([B, Fx, H,
    W] and [B, Fc, H, W] at V = 1), None where not wanted; an input that was broadcast over frames (Fx or Fc == 1 < F)
    gets the sum over the F frames."""
    Nb, H, W, Co = dy.shape
    KS = w.shape[-1]
    cin = w.shape[1]
    if cin < 2 or cin % 2:
        raise ValueError(f"stem weight with {cin} input channels: expected 2V (x_t and cond of V variables)")
    V = cin // 2
    _chk(dy, (B * F, H, W, Co))
    _chk(w, (Co, cin, 1, KS, KS), torch.float32)
    var = () if V == 1 else (V,)
    dxt = empty((B, *var, Fx, H, W), torch.float32, dy.device) if want_xt else None
    dcond = empty((B, *var, Fc, H, W), torch.float32, dy.device) if want_cond else None
    _mv_call("cesm_stem_dgrad_mv", f"V={V} KS={KS} Co={Co} F={F} Fx={Fx} Fc={Fc}", dtcode(dy), P(dy), P(w), P(dxt),
             P(dcond), B, V, F, Fx, Fc, H, W, Co, KS, S())
    return dxt, dcond


STEM_MAX_COND = 4  # conditioning maps of the stem (cesm_stem_*_mc): 1 .. 4, like the target variables


def _stem_io_mc(xt, cond, cin, F):
    """(B, V, Cc, Fx, Fc, H, W) of the multi-forcing stem's inputs: xt [B, V, Fx, H, W], cond [B, Cc, Fc, H, W] fp32,
    V + Cc = the weight's input channels cin (V and Cc are read from the inputs, always 5-D here)"""
    if xt.ndim != 5 or cond.ndim != 5:
        raise ValueError(f"stem inputs must be [B, V, F, H, W] and [B, Cc, F, H, W], got {tuple(xt.shape)} and "
                         f"{tuple(cond.shape)}")
    B, V, Fx, H, W = xt.shape
    Cc, Fc = cond.shape[1], cond.shape[2]
    if V + Cc != cin:
        raise RuntimeError(f"shape mismatch: stem weight with {cin} input channels, x_t has {V} and cond {Cc}")
    _chk(xt, (B, V, Fx, H, W), torch.float32)
    _chk(cond, (B, Cc, Fc, H, W), torch.float32)
    if Fx not in (1, F) or Fc not in (1, F):
        raise ValueError(f"stem: x_t has {Fx} frames and cond {Fc}; each must be 1 or F = {F}")
    return B, V, Cc, Fx, Fc, H, W


def stem_fwd_mc(xt, cond, w, b, F, dtype):
    """stem Conv3d(V + Cc -> Co, (1,KS,KS)) on cat([x_t, cond]) with Cc conditioning maps (cesm_stem_fwd_mc): xt [B, V,
    Fx, H, W], cond [B, Cc, Fc, H, W], w [Co, V + Cc, 1, KS, KS]; 1 <= V, Cc <= 4.  Cc == V runs what stem_fwd runs."""
    Co, cin, _, KS, _ = w.shape
    B, V, Cc, Fx, Fc, H, W = _stem_io_mc(xt, cond, cin, F)
    _chk(w, (Co, cin, 1, KS, KS), torch.float32)
    _chk(b, (Co,), torch.float32)
    y = empty((B * F, H, W, Co), dtype, xt.device)
    _mv_call("cesm_stem_fwd_mc", f"V={V} Cc={Cc} KS={KS} Co={Co} F={F} Fx={Fx} Fc={Fc}", _DT[dtype], P(xt), P(cond),
             P(w), P(b), P(y), B, V, Cc, F, Fx, Fc, H, W, Co, KS, S())
    return y


def stem_wgrad_mc(xt, cond, dy, dw, F, accumulate=True):
    """weight gradient of stem_fwd_mc: dw [Co, V + Cc, 1, KS, KS] fp32 (+)= ..."""
    Co, cin, _, KS, _ = dw.shape
    B, V, Cc, Fx, Fc, H, W = _stem_io_mc(xt, cond, cin, F)
    _chk(dy, (B * F, H, W, Co))
    _chk(dw, (Co, cin, 1, KS, KS), torch.float32)
    nblk = 512
    part = empty((nblk, Co * cin * KS * KS), torch.float32, xt.device)
    _mv_call("cesm_stem_wgrad_mc", f"V={V} Cc={Cc} KS={KS} Co={Co} F={F} Fx={Fx} Fc={Fc}", dtcode(dy), P(xt), P(cond),
             P(dy), P(dw), P(part), nblk, B, V, Cc, F, Fx, Fc, H, W, Co, KS, int(accumulate), S())


def stem_dgrad_mc(dy, w, B, V, F, Fx, Fc, want_xt=True, want_cond=True):
    """data gradient of stem_fwd_mc: w [Co, V + Cc, 1, KS, KS] and V give Cc.  Returns (dxt [B, V, Fx, H, W], dcond [B,
    Cc, Fc, H, W]) fp32, None where not wanted; a frame-broadcast input gets the sum over the F frames."""
    Nb, H, W, Co = dy.shape
    KS = w.shape[-1]
    cin = w.shape[1]
    V = int(V)
    Cc = cin - V
    if V < 1 or Cc < 1:
        raise ValueError(f"stem weight with {cin} input channels and V = {V}: no conditioning maps left")
    _chk(dy, (B * F, H, W, Co))
    _chk(w, (Co, cin, 1, KS, KS), torch.float32)
    dxt = empty((B, V, Fx, H, W), torch.float32, dy.device) if want_xt else None
    dcond = empty((B, Cc, Fc, H, W), torch.float32, dy.device) if want_cond else None
    _mv_call("cesm_stem_dgrad_mc", f"V={V} Cc={Cc} KS={KS} Co={Co} F={F} Fx={Fx} Fc={Fc}", dtcode(dy), P(dy), P(w),
             P(dxt), P(dcond), B, V, Cc, F, Fx, Fc, H, W, Co, KS, S())
    return dxt, dcond


def _head_v(w, C):
    if w.numel() == 0 or w.numel() % C:
        raise ValueError(f"head weight of shape {tuple(w.shape)} on {C} channels: expected [V, {C}]")
    return w.numel() // C


def head_fwd(x, w, b, B, F):
    """head Conv3d(C -> V, 1) on frame F // 2: x [B*F, H, W, C], w [V, C] (any shape with V*C elements, e.g. the module's
    [V, C, 1, 1, 1]), b [V]; returns [B, V, H, W] fp32"""
    Nb, H, W, C = x.shape
    V = _head_v(w, C)
    _chk(x, (B * F, H, W, C))
    _chk(w, dtype=torch.float32)
    _chk(b, (V,), torch.float32)
    out = empty((B, V, H, W), torch.float32, x.device)
    _mv_call("cesm_head_fwd_mv", f"V={V} C={C}", dtcode(x), P(x), P(w), P(b), P(out), B, V, F, H * W, C, S())
    return out


def head_bwd(dout, x, w, dw, db, B, F, need_dx=True, accumulate=True):
    """dout [B, V, H, W] fp32; dw shaped like w ([V, C]), db [V] (both None: no parameter gradients)"""
    Nb, H, W, C = x.shape
    V = _head_v(w, C)
    _chk(x, (B * F, H, W, C))
    _chk(dout, (B, V, H, W), torch.float32)
    _chk(w, dtype=torch.float32)
    if dw is not None:
        _chk(dw, dtype=torch.float32)
        _chk(db, (V,), torch.float32)
        if dw.numel() != V * C or db is None:
            raise RuntimeError(f"head_bwd: dw needs {V * C} elements and db [{V}]")
    dx = empty(x.shape, x.dtype, x.device) if need_dx else None
    nblk = 256
    part = empty((nblk, V * (C + 1)), torch.float32, x.device)
    _mv_call("cesm_head_bwd_mv", f"V={V} C={C}", dtcode(x), P(dout), P(x), P(w), P(dx), P(dw), P(db), P(part), nblk, B,
             V, F, H * W, C, int(accumulate), S())
    return dx


# ------------------------------------------------------------------------------------ norms
def gn_stats(y, B, G, eps=1e-5):
    C = y.shape[-1]
    rows_b = y.numel() // (C * B)
    stats = empty((B, G, 2), torch.float32, y.device)
    ws = empty((max(B * 256, 1024) * G * 2,), torch.float64, y.device)
    call("cesm_gn_stats", dtcode(y), P(y), P(stats), P(ws), B, rows_b, C, G, float(eps), S())
    return stats


def gn_stats_part(part, rows_b, G, eps=1e-5):
    """GroupNorm (mean, rstd) [B][G][2] from conv_fwd_gn's partials (replaces gn_stats' pass over y)"""
    B, nslot, nq, _ = part.shape
    stats = empty((B, G, 2), torch.float32, part.device)
    call("cesm_gn_stats_part", P(part), P(stats), B, nslot, nq * 4, G, rows_b, float(eps), S())
    return stats


def gn_apply(y, stats, gamma, beta, ss, res, B, G):
    C = y.shape[-1]
    rows_b = y.numel() // (C * B)
    out = empty(y.shape, y.dtype, y.device)
    _chk(res, y.shape, y.dtype)
    ws = empty((2 * B * C,), torch.float32, y.device)
    call("cesm_gn_apply", dtcode(y), P(y), P(stats), P(gamma), P(beta), P(ss), P(res), P(out), P(ws), B, rows_b, C,
         G, S())
    return out


def gn_bwd(dout, y, stats, gamma, beta, ss, dgamma, dbeta, B, G, want_dss, dbias=None):
    """GroupNorm(+scale/shift, SiLU) backward; dbias (+)= sum of dy over rows (the producing conv's bias)"""
    C = y.shape[-1]
    rows_b = y.numel() // (C * B)
    dy = empty(y.shape, y.dtype, y.device)
    dss = empty((B, 2 * C), torch.float32, y.device) if want_dss else None
    ws = empty((max(B * 1024, 1024) * C * 3 + B * C * 3 + B * C * 5,), torch.float32, y.device)  # <= 1024 chunks/sample
    call("cesm_gn_bwd", dtcode(y), P(dout), P(y), P(stats), P(gamma), P(beta), P(ss), P(dy), P(dss), P(dgamma),
         P(dbeta), P(dbias), P(ws), B, rows_b, C, G, 1, S())
    return dy, dss


def _row_window(t, B, row_lo, row_n):
    """(C, rows_b) of the full tensor t [B * frames, H, W, C] after checking the window [row_lo, row_lo + row_n)"""
    _chk(t)
    C = t.shape[-1]
    rows_b = t.numel() // (C * B)
    if t.numel() != B * rows_b * C or row_lo < 0 or row_n <= 0 or row_lo + row_n > rows_b:
        raise RuntimeError(f"row window [{row_lo}, {row_lo + row_n}) outside the {rows_b} rows of a sample")
    return C, rows_b


def gn_apply_rows(y, stats, gamma, beta, ss, res_c, B, G, row_lo, row_n):
    """gn_apply on rows [row_lo, row_lo + row_n) of every sample: y full, res_c (or None) and the result compact
    [B, row_n, C]"""
    C, rows_b = _row_window(y, B, row_lo, row_n)
    out = empty((B, row_n, C), y.dtype, y.device)
    if res_c is not None:
        _chk(res_c, dtype=y.dtype)
        if res_c.numel() != out.numel():
            raise RuntimeError(f"gn_apply_rows: res_c has {res_c.numel()} elements, expected {out.numel()}")
    ws = empty((2 * B * C,), torch.float32, y.device)
    call("cesm_gn_apply_rows", dtcode(y), P(y), P(stats), P(gamma), P(beta), P(ss), P(res_c), P(out), P(ws), B, rows_b,
         C, G, row_lo, row_n, S())
    return out


def gn_bwd_rows(dout_c, y, stats, gamma, beta, ss, dgamma, dbeta, B, G, want_dss, row_lo, row_n, dbias=None):
    """gn_bwd for a dout that is zero outside rows [row_lo, row_lo + row_n) of every sample, given compact as dout_c
    [B, row_n, C]; returns the dense dy (y's shape) and dss"""
    C, rows_b = _row_window(y, B, row_lo, row_n)
    _chk(dout_c, dtype=y.dtype)
    if dout_c.numel() != B * row_n * C:
        raise RuntimeError(f"gn_bwd_rows: dout_c has {dout_c.numel()} elements, expected {B * row_n * C}")
    dy = empty(y.shape, y.dtype, y.device)
    dss = empty((B, 2 * C), torch.float32, y.device) if want_dss else None
    ws = empty((max(B * 1024, 1024) * C * 3 + B * C * 3 + B * C * 5,), torch.float32, y.device)
    call("cesm_gn_bwd_rows", dtcode(y), P(dout_c), P(y), P(stats), P(gamma), P(beta), P(ss), P(dy), P(dss), P(dgamma),
         P(dbeta), P(dbias), P(ws), B, rows_b, C, G, row_lo, row_n, 1, S())
    return dy, dss


def rows_gather(x, B, row_lo, row_n, out_shape=None):
    """rows [row_lo, row_lo + row_n) of every sample of x [B * frames, H, W, C] as a compact tensor [B, row_n, C]
    (or out_shape with as many elements)"""
    C, rows_b = _row_window(x, B, row_lo, row_n)
    out = empty((B, row_n, C) if out_shape is None else out_shape, x.dtype, x.device)
    if out.numel() != B * row_n * C:
        raise RuntimeError(f"rows_gather: out_shape {tuple(out.shape)} does not hold {B} x {row_n} x {C} elements")
    call("cesm_rows_gather", dtcode(x), P(x), P(out), B, rows_b, row_lo, row_n, C, S())
    return out


def rows_scatter(src_c, dst, B, row_lo, row_n):
    """overwrite rows [row_lo, row_lo + row_n) of every sample of dst with the compact src_c; other rows untouched"""
    C, rows_b = _row_window(dst, B, row_lo, row_n)
    _chk(src_c, dtype=dst.dtype)
    if src_c.numel() != B * row_n * C:
        raise RuntimeError(f"rows_scatter: src_c has {src_c.numel()} elements, expected {B * row_n * C}")
    call("cesm_rows_scatter", dtcode(dst), P(src_c), P(dst), B, rows_b, row_lo, row_n, C, S())
    return dst


def ln_fwd(x, gamma, save=True, eps=1e-5, perm=None):
    """perm = (F, HW): write the output rows of voxel (b, f, p) at (b, p, f) -- pixel-major, a pixel's frames
    adjacent (mr stays in x's order)"""
    if not (x.is_cuda and gamma.is_cuda):  # checked here, not left to the stream query: host pointers must not launch
        raise RuntimeError("cesm_emulator_amd kernels need device tensors (no CPU fallback)")
    C = x.shape[-1]
    V = x.numel() // C
    out = empty(x.shape, x.dtype, x.device)
    mr = empty((V, 2), torch.float32, x.device) if save else None
    pf, phw = perm if perm else (0, 0)
    call("cesm_ln_fwd", dtcode(x), P(x), P(gamma), P(out), P(mr), V, C, float(eps), pf, phw, S())
    return out, mr


def ln_bwd(dy, x, mr, gamma, dgamma, dres=None, perm=None):
    """perm = (F, HW): dy rows are pixel-major (as ln_fwd(perm=...) wrote the output); x, dres, dx in x's order"""
    C = x.shape[-1]
    V = x.numel() // C
    dx = empty(x.shape, x.dtype, x.device)
    nblk = 1024
    part = empty((nblk, C), torch.float32, x.device)
    _chk(dres, x.shape, x.dtype)
    pf, phw = perm if perm else (0, 0)
    call("cesm_ln_bwd", dtcode(x), P(dy), P(x), P(mr), P(gamma), P(dres), P(dx), P(dgamma), P(part), nblk, V, C, 1,
         pf, phw, S())
    return dx


TCONV_C = (64, 128, 256)  # widths of the temporal-convolution kernels (csrc/tconv.h)


def tconv_fwd(x, gamma, wp, bias, B, F, save=True, eps=1e-5):
    """Residual(PreNorm(TemporalCNN)) forward (csrc/tconv.h): x [B*F, H, W, C]; wp = conv_pack(w, x.dtype, C, C, 1, 3, 0, 0)
    of the Conv1d weight [C, C, 3]; returns (y, mr) with mr [V, 2] = (mean, rstd) per voxel when save, else None."""
    Nb, H, W, C = x.shape
    if C not in TCONV_C:
        raise ValueError(f"tconv_fwd: C = {C} is not one of {TCONV_C}")
    if Nb != B * F:
        raise RuntimeError(f"tconv_fwd: {Nb} images are not B x F = {B} x {F}")
    _chk(x)
    _chk(wp, (C, 3 * C), x.dtype)
    _chk(gamma, (C,), torch.float32)
    _chk(bias, (C,), torch.float32)
    V = Nb * H * W
    y = empty(x.shape, x.dtype, x.device)
    mr = empty((V, 2), torch.float32, x.device) if save else None
    ws = empty(x.shape, x.dtype, x.device) if x.dtype == torch.float32 else None
    call("cesm_tconv_fwd", dtcode(x), P(x), P(gamma), P(wp), P(bias), P(y), P(mr), P(ws), B, F, H * W, C, float(eps), S())
    return y, mr


def tconv_bwd(x, dy, mr, gamma, wpt, dgamma, dw, db, B, F, eps=1e-5, accumulate=True):
    """backward of tconv_fwd: returns dx; dgamma [C], dw [C, C, 3], db [C] fp32 (+)= their gradients, each nullable (then
    not computed).  wpt = conv_pack(w, x.dtype, C, C, 1, 3, 1, 1)."""
    Nb, H, W, C = x.shape
    if C not in TCONV_C:
        raise ValueError(f"tconv_bwd: C = {C} is not one of {TCONV_C}")
    if Nb != B * F:
        raise RuntimeError(f"tconv_bwd: {Nb} images are not B x F = {B} x {F}")
    V = Nb * H * W
    _chk(x)
    _chk(dy, x.shape, x.dtype)
    _chk(mr, (V, 2), torch.float32)
    _chk(wpt, (C, 3 * C), x.dtype)
    _chk(gamma, (C,), torch.float32)
    _chk(dgamma, (C,), torch.float32)
    _chk(dw, (C, C, 3), torch.float32)
    _chk(db, (C,), torch.float32)
    dev, f32 = x.device, x.dtype == torch.float32
    dt = dtcode(x)
    dx = empty(x.shape, x.dtype, dev)
    part = slab = ws_n = ws_dn = None
    if f32 or dgamma is not None or db is not None:
        part = empty((lib().cesm_tconv_part_floats(dt, B, F, H * W, C),), torch.float32, dev)
    if dw is not None:
        slab = empty((lib().cesm_tconv_slab_floats(dt, B, F, H * W, C),), torch.float32, dev)
    if f32:
        ws_dn = empty(x.shape, x.dtype, dev)
        if dw is not None or db is not None:
            ws_n = empty(x.shape, x.dtype, dev)
    call("cesm_tconv_bwd", dt, P(x), P(dy), P(mr), P(gamma), P(wpt), P(dx), P(dgamma), P(dw), P(db), P(part), P(slab),
         P(ws_n), P(ws_dn), B, F, H * W, C, float(eps), int(accumulate), S())
    return dx


def add(a, b):
    out = empty(a.shape, a.dtype, a.device)
    _chk(b, a.shape, a.dtype)
    call("cesm_add", dtcode(a), P(a), P(b), P(out), a.numel(), S())
    return out


# ------------------------------------------------------------------------------------ attention
def rope_table(freqs, F):
    rot = empty((F, 16, 2), torch.float32, freqs.device)
    call("cesm_rope_table", P(freqs), P(rot), F, S())
    return rot


def relpos_fwd(table, F, num_buckets=32, max_distance=32):
    nb, heads = table.shape
    bias = empty((heads, F, F), torch.float32, table.device)
    call("cesm_relpos_fwd", P(table), P(bias), F, heads, num_buckets, max_distance, S())
    return bias


# bf16 temporal-attention core on MFMA (csrc/tflash.hip) for F <= 128; fp32 (parity mode): the VALU kernels
def _tflash(qkv, F):
    return qkv.dtype == torch.bfloat16 and lib().cesm_tflash_supported(F) == 1


def tattn_fwd(qkv, bias, rot, B, F, HW, scale, save=True, pixel_major=False):
    """pixel_major (MFMA core, F > 16): qkv rows ordered [B][HW][F]; out stays [B][F][HW]"""
    V = qkv.shape[0]
    _chk(qkv, (B * F * HW, 768))
    out = empty((V, 256), qkv.dtype, qkv.device)
    lse = empty((B, 8, HW, F), torch.float32, qkv.device) if save else None
    if _tflash(qkv, F):
        call("cesm_tflash_fwd", P(qkv), P(bias), P(rot), P(out), P(lse), B, F, HW, float(scale), int(pixel_major), S())
        return out, lse
    if pixel_major:
        raise ValueError("pixel-major qkv needs the MFMA temporal core (bf16, F <= 128)")
    call("cesm_tattn_fwd", dtcode(qkv), P(qkv), P(bias), P(rot), P(out), P(lse), B, F, HW, float(scale), S())
    return out, lse


def tattn_bwd(qkv, o, dout, lse, bias, rot, dtable, B, F, HW, scale, num_buckets=32, max_distance=32,
              pixel_major=False):
    """pixel_major: qkv and the returned dqkv in [B][HW][F] row order (o, dout frame-major)"""
    dqkv = empty(qkv.shape, qkv.dtype, qkv.device)
    if _tflash(qkv, F):
        _chk(o, (qkv.shape[0], 256), qkv.dtype)
        _chk(dout, (qkv.shape[0], 256), qkv.dtype)
        dev = qkv.device
        nblk = lib().cesm_tflash_nblk(HW)
        dbuf = empty((B, 8, HW, F), torch.float32, dev)
        part = empty((B * 8 * nblk * (2 * F - 1),), torch.float32, dev)
        off = empty((8 * (2 * F - 1),), torch.float32, dev)
        call("cesm_tflash_bwd", P(qkv), P(o), P(dout), P(lse), P(bias), P(rot), P(dqkv), P(dtable), P(dbuf), P(part),
             P(off), B, F, HW, float(scale), num_buckets, max_distance, 1, int(pixel_major), S())
        return dqkv
    if pixel_major:
        raise ValueError("pixel-major qkv needs the MFMA temporal core (bf16, F <= 128)")
    nblk = lib().cesm_tattn_nblk(F, HW)
    part = empty((B * 8 * nblk, F, F), torch.float32, qkv.device)
    call("cesm_tattn_bwd", dtcode(qkv), P(qkv), P(o), P(dout), P(lse), P(bias), P(rot), P(dqkv), P(part), B, F, HW,
         float(scale), S())
    if dtable is not None:
        ws = empty((8, F, F), torch.float32, qkv.device)
        call("cesm_relpos_bwd", P(part), nblk, B, P(dtable), P(ws), F, 8, num_buckets, max_distance, 1, S())
    return dqkv


TBLOCK_C = (64, 128, 256, 512)


def tblock_fwd(x, gamma, wqkv, wout, bias, rot, B, F, scale, save=True, eps=1e-5, save_o=False):
    """fused temporal-attention block forward (bf16); x [B*F, H, W, C].  Returns (y, mr, lse, o); o (the
    attention output before to_out, [B*F, H, W, 256]) only with save_o (C <= 256), for the to_out weight
    gradient, so the backward need not emit it."""
    Nb, H, W, C = x.shape
    _chk(x, dtype=torch.bfloat16)
    _chk(wqkv, (768, C), torch.bfloat16)
    _chk(wout, (C, 256), torch.bfloat16)
    y = empty(x.shape, x.dtype, x.device)
    mr = empty((Nb * H * W, 2), torch.float32, x.device) if save else None
    lse = empty((B, 8, H * W, F), torch.float32, x.device) if save else None
    o = empty((Nb, H, W, 256), x.dtype, x.device) if save_o else None
    wimg = empty(((768 + 256) * C,), torch.bfloat16, x.device)  # weight fragment images (rebuilt per call)
    call("cesm_tblock_fwd", P(x), P(gamma), P(wqkv), P(wout), P(bias), P(rot), P(y), P(mr), P(lse), P(o), P(wimg),
         B, F, H * W, C, float(scale), float(eps), S())
    return y, mr, lse, o


def tblock_bwd(x, dy, gamma, mr, lse, wqkv, wqkv_t, wout_t, bias, rot, dgamma, dtable, B, F, scale,
               want_wgrad_inputs=True, num_buckets=32, max_distance=32, emit_o=True):
    """fused temporal-attention block backward, dx path (bf16).  Returns (dx, dqkv, o, xn); the last
    three ([.., 768], [.., 256], [.., C] bf16) feed the to_qkv / to_out weight-gradient GEMMs."""
    Nb, H, W, C = x.shape
    HW = H * W
    _chk(x, dtype=torch.bfloat16)
    _chk(dy, x.shape, torch.bfloat16)
    _chk(wqkv, (768, C), torch.bfloat16)
    _chk(wqkv_t, (C, 768), torch.bfloat16)
    _chk(wout_t, (256, C), torch.bfloat16)
    if Nb != B * F or mr.shape != (Nb * HW, 2) or lse.shape != (B, 8, HW, F):
        raise ValueError("tblock_bwd: saved statistics do not match x")
    dev = x.device
    dx = empty(x.shape, x.dtype, dev)
    if want_wgrad_inputs:
        dqkv = empty((Nb, H, W, 768), x.dtype, dev)
        o = empty((Nb, H, W, 256), x.dtype, dev) if emit_o else None
        xn = empty(x.shape, x.dtype, dev)
    else:
        dqkv = o = xn = None
    nblk = lib().cesm_tblock_bwd_nblk(B, F, HW, C)
    dbp = empty((B, 8, nblk, F, F), torch.float32, dev)
    dgp = empty((B * nblk, C), torch.float32, dev)
    wimg = empty(((2 * 768 + 256) * C,), torch.bfloat16, dev)  # weight fragment images (rebuilt per call)
    call("cesm_tblock_bwd", P(x), P(dy), P(gamma), P(mr), P(lse), P(wqkv), P(wqkv_t), P(wout_t), P(bias), P(rot),
         P(dx), P(dqkv), P(o), P(xn), P(dbp), P(dgamma), P(dgp), P(wimg), nblk, B, F, HW, C, float(scale), 1, S())
    if dtable is not None:
        ws = empty((8, F, F), torch.float32, dev)
        call("cesm_relpos_bwd", P(dbp), nblk, B, P(dtable), P(ws), F, 8, num_buckets, max_distance, 1, S())
    return dx, dqkv, o, xn


def tblock_bwd_dw_supported(B, F, HW, C):
    """shapes the head-parallel fused backward with in-kernel weight gradients handles (C = 64, 4F <= 48)"""
    return lib().cesm_tblock_bwd_dw_nblk(B, F, HW, C) > 0


def tblock_fwd_fold(x, gamma, wqkv_f32, wout, bias, rot, B, F, scale, save=True, eps=1e-5, save_o=False):
    """tblock_fwd with the LN gamma folded into the QKV weights (the forward of tblock_bwd_dw); wqkv_f32 is
    the fp32 master to_qkv weight [768, C].  Returns (y, mr, lse, o) as tblock_fwd."""
    Nb, H, W, C = x.shape
    _chk(x, dtype=torch.bfloat16)
    _chk(wqkv_f32, (768, C), torch.float32)
    _chk(wout, (C, 256), torch.bfloat16)
    _chk(gamma, (C,), torch.float32)
    y = empty(x.shape, x.dtype, x.device)
    mr = empty((Nb * H * W, 2), torch.float32, x.device) if save else None
    lse = empty((B, 8, H * W, F), torch.float32, x.device) if save else None
    o = empty((Nb, H, W, 256), x.dtype, x.device) if save_o else None
    wimg = empty(((768 + 256) * C,), torch.bfloat16, x.device)
    call("cesm_tblock_fwd_fold", P(x), P(gamma), P(wqkv_f32), P(wout), P(bias), P(rot), P(y), P(mr), P(lse), P(o),
         P(wimg), B, F, H * W, C, float(scale), float(eps), S())
    return y, mr, lse, o


def tblock_bwd_dw(x, dy, mr, lse, wqkv_f32, gamma, wout_t, bias, rot, dwqkv, dgamma, dtable, B, F, scale,
                  num_buckets=32, max_distance=32, emit_o=False):
    """head-parallel fused temporal-block backward with in-kernel weight gradients (C = 64, 4F <= 48):
    returns dx, or (dx, o) with emit_o -- o [Nb, H, W, 256] the attention output recomputed from the backward's P,
    the to_out weight gradient's input (the forward then writes none); dwqkv (+)= the to_qkv weight gradient,
    dgamma (+)= the LN gamma gradient, dtable (+)= the rel-pos table gradient (each nullable).  The forward must
    be tblock_fwd_fold's."""
    Nb, H, W, C = x.shape
    HW = H * W
    _chk(x, dtype=torch.bfloat16)
    _chk(dy, x.shape, torch.bfloat16)
    _chk(wqkv_f32, (768, C), torch.float32)
    _chk(gamma, (C,), torch.float32)
    _chk(wout_t, (256, C), torch.bfloat16)
    _chk(dwqkv, (768, C), torch.float32)
    _chk(dgamma, (C,), torch.float32)
    if Nb != B * F or mr.shape != (Nb * HW, 2) or lse.shape != (B, 8, HW, F):
        raise ValueError("tblock_bwd_dw: saved statistics do not match x")
    nblk = lib().cesm_tblock_bwd_dw_nblk(B, F, HW, C)
    if nblk <= 0:
        raise ValueError(f"tblock_bwd_dw: unsupported shape C={C} F={F}")
    dev = x.device
    dx = empty(x.shape, x.dtype, dev)
    o = empty((Nb, H, W, 256), x.dtype, dev) if emit_o else None
    dbp = empty((8, nblk, F, F), torch.float32, dev)
    slab = empty((nblk * 768 * C,), torch.float32, dev)
    tmp = empty((768, C), torch.float32, dev)
    wimg = empty(((2 * 768 + 256) * C,), torch.bfloat16, dev)
    call("cesm_tblock_bwd_dw", P(x), P(dy), P(mr), P(lse), P(wqkv_f32), P(gamma), P(wout_t), P(bias), P(rot), P(dx),
         P(o), P(dwqkv), P(dgamma), P(dbp), P(slab), P(tmp), P(wimg), nblk, B, F, HW, C, float(scale), 1, S())
    if dtable is not None:
        ws = empty((8, F, F), torch.float32, dev)
        call("cesm_relpos_bwd", P(dbp), nblk, 1, P(dtable), P(ws), F, 8, num_buckets, max_distance, 1, S())
    return (dx, o) if emit_o else dx


# fused SLA at C = 64 and 128 (measured +0.8 % step throughput for C = 128 with the parallel context
# combine)
SLAF_C = (64, 128)


def slaf_fwd(x, gamma, wqkv, wout, bout, scale, eps=1e-5, save_o=False):
    """fused spatial-linear-attention block forward (bf16, C=64/128); x [Nf, H, W, C].
    Returns y and the saved state (mz, ctx32, actT, actx, o) for slaf_bwd; o (the attention output before
    to_out, [Nf, H, W, 256]) only with save_o, for the to_out weight gradient."""
    Nf, H, W, C = x.shape
    HW = H * W
    _chk(x, dtype=torch.bfloat16)
    _chk(wqkv, (768, C), torch.bfloat16)
    _chk(wout, (C, 256), torch.bfloat16)
    dev = x.device
    y = empty(x.shape, x.dtype, dev)
    mz = empty((Nf, 8, 32, 2), torch.float32, dev)
    ctx32 = empty((Nf, 8, 32, 32), torch.float32, dev)
    actT = empty((Nf, 8, 2, 64, 8), torch.bfloat16, dev)
    actx = empty((Nf, 8, 2, 64, 8), torch.bfloat16, dev)
    nblk = lib().cesm_slaf_nblk(Nf, HW)
    ws = empty((nblk * Nf * 8 * 1088,), torch.float32, dev)
    o = empty((Nf, H, W, 256), x.dtype, dev) if save_o else None
    call("cesm_slaf_fwd", P(x), P(gamma), P(wqkv), P(wout), P(bout), P(y), P(o), P(mz), P(ctx32), P(actT), P(actx),
         P(ws), Nf, HW, C, float(scale), float(eps), S())
    return y, (mz, ctx32, actT, actx, o)


def slaf_bwd(x, dy, gamma, wqkv, wqkv_t, wout_t, state, dgamma, scale, want_wgrad_inputs=True, eps=1e-5):
    """fused SLA block backward, dx path (bf16, C=64).  Returns (dx, dqkv, o, xn); the last three feed the
    to_qkv / to_out weight-gradient GEMMs.  When the forward saved o (slaf_fwd save_o), that o is returned
    and the backward does not emit it."""
    Nf, H, W, C = x.shape
    HW = H * W
    mz, ctx32, actT, actx, o_fwd = state
    _chk(dy, x.shape, torch.bfloat16)
    _chk(wqkv_t, (C, 768), torch.bfloat16)
    _chk(wout_t, (256, C), torch.bfloat16)
    dev = x.device
    dx = empty(x.shape, x.dtype, dev)
    if want_wgrad_inputs:
        dqkv = empty((Nf, H, W, 768), x.dtype, dev)
        o = empty((Nf, H, W, 256), x.dtype, dev) if o_fwd is None else None
        xn = empty(x.shape, x.dtype, dev)
    else:
        dqkv = o = xn = None
    nblk = lib().cesm_slaf_nblk(Nf, HW)
    part = empty((nblk * Nf * 8 * 1024,), torch.float32, dev)
    G = empty((Nf, 8, 64, 16), torch.float32, dev)  # per-lane k-softmax offsets + G image
    adc = empty((Nf, 8, 2, 64, 8), torch.bfloat16, dev)
    adcT = empty((Nf, 8, 2, 64, 8), torch.bfloat16, dev)
    dgp = empty((lib().cesm_slaf_bwd_nblk(Nf, HW, C), C), torch.float32, dev)
    wimg = empty(((2 * 768 + 256) * C,), torch.bfloat16, dev)
    call("cesm_slaf_bwd", P(x), P(dy), P(gamma), P(wqkv), P(wqkv_t), P(wout_t), P(mz), P(ctx32), P(actT), P(actx),
         P(dx), P(dqkv), P(o), P(xn), P(dgamma), P(part), P(G), P(adc), P(adcT), P(dgp), P(wimg), Nf, HW, C,
         float(scale), float(eps), 1, S())
    if want_wgrad_inputs and o_fwd is not None:
        o = o_fwd
    return dx, dqkv, o, xn


def pack_scaled(w, colscale, trans=False):
    """bf16 copy of w diag(colscale) (w fp32 [M, K]); trans: the transposed [K, M] layout"""
    M, K = w.shape
    _chk(w, dtype=torch.float32)
    _chk(colscale, (K,), torch.float32)
    out = empty((K, M) if trans else (M, K), torch.bfloat16, w.device)
    call("cesm_pack_scaled", P(w), P(colscale), P(out), M, K, int(trans), S())
    return out


def slaf_bwd_dw_supported(Nf, HW, C):
    return lib().cesm_slaf_bwd_dw_nblk(Nf, HW, C) > 0


def slaf_bwd_dw(x, dy, gamma_one, wq_fold, wqkv_f32, gamma, wout_t, state, dwqkv, dgamma, scale, eps=1e-5,
                dwout=None, dbout=None):
    """fused SLA block backward with in-kernel weight gradients (C = 64); the forward must have been
    slaf_fwd(x, gamma_one, wq_fold, ...) with wq_fold = pack_scaled(wqkv_f32, gamma).  Returns dx; dwqkv /
    dgamma (+)= the to_qkv / LN gamma gradients, dwout [C, 256] / dbout [C] (+)= the to_out weight / bias
    gradients (both or neither; computed from the recomputed q~ and the saved context: no O needed)."""
    Nf, H, W, C = x.shape
    HW = H * W
    mz, ctx32, actT, actx, _o = state
    _chk(x, dtype=torch.bfloat16)
    _chk(dy, x.shape, torch.bfloat16)
    _chk(wq_fold, (768, C), torch.bfloat16)
    _chk(wqkv_f32, (768, C), torch.float32)
    _chk(gamma, (C,), torch.float32)
    _chk(gamma_one, (C,), torch.float32)
    _chk(wout_t, (256, C), torch.bfloat16)
    _chk(dwqkv, (768, C), torch.float32)
    _chk(dgamma, (C,), torch.float32)
    nblk_dx = lib().cesm_slaf_bwd_dw_nblk(Nf, HW, C)
    if nblk_dx <= 0:
        raise ValueError(f"slaf_bwd_dw: unsupported shape C={C}")
    dev = x.device
    dx = empty(x.shape, x.dtype, dev)
    nblk = lib().cesm_slaf_nblk(Nf, HW)
    part = empty((nblk * Nf * 8 * 1024,), torch.float32, dev)
    G = empty((Nf, 8, 64, 16), torch.float32, dev)
    adc = empty((Nf, 8, 2, 64, 8), torch.bfloat16, dev)
    adcT = empty((Nf, 8, 2, 64, 8), torch.bfloat16, dev)
    slab = empty((nblk_dx, 768, C), torch.float32, dev)
    tmp = empty((768, C), torch.float32, dev)
    wimg = empty(((2 * 768 + 256) * C,), torch.bfloat16, dev)
    if (dwout is None) != (dbout is None):
        raise ValueError("slaf_bwd_dw: dwout and dbout go together")
    partm = partb = None
    if dwout is not None:
        _chk(dwout, (C, 256), torch.float32)
        _chk(dbout, (C,), torch.float32)
        partm = empty(((nblk + 1) * Nf * 8 * 2048,), torch.float32, dev)
        partb = empty((nblk * Nf * C,), torch.float32, dev)
    call("cesm_slaf_bwd_dw", P(x), P(dy), P(gamma_one), P(wq_fold), P(wqkv_f32), P(gamma), P(wout_t), P(mz), P(ctx32),
         P(actT), P(actx), P(dx), P(dwqkv), P(dgamma), P(dwout), P(dbout), P(part), P(G), P(adc), P(adcT), P(slab),
         P(tmp), P(partm), P(partb), P(wimg), nblk_dx, Nf, HW, C, float(scale), float(eps), 1, S())
    return dx


def sla_fwd(qkv, Nf, HW, scale):
    nchunk = lib().cesm_sla_nchunk(HW)
    out = empty((qkv.shape[0], 256), qkv.dtype, qkv.device)
    ctx = empty((Nf, 8, 32, 32), torch.float32, qkv.device)
    ml = empty((Nf, 8, 32, 2), torch.float32, qkv.device)
    ws = empty((Nf * 8 * nchunk * (32 + 32 + 1024),), torch.float32, qkv.device)
    call("cesm_sla_fwd", dtcode(qkv), P(qkv), P(out), P(ctx), P(ml), P(ws), Nf, HW, float(scale), S())
    return out, ctx, ml


def sla_bwd(qkv, dout, ctx, ml, Nf, HW, scale):
    nchunk = lib().cesm_sla_nchunk(HW)
    dqkv = empty(qkv.shape, qkv.dtype, qkv.device)
    ws = empty((Nf * 8 * nchunk * 1024 + Nf * 8 * (1024 + 32),), torch.float32, qkv.device)
    call("cesm_sla_bwd", dtcode(qkv), P(qkv), P(dout), P(ctx), P(ml), P(dqkv), P(ws), Nf, HW, float(scale), S())
    return dqkv


# ------------------------------------------------------------------------------------ misc
def sinusoidal(t, dim):
    emb = empty((t.shape[0], dim), torch.float32, t.device)
    call("cesm_sinusoidal", P(t), P(emb), t.shape[0], dim, S())
    return emb


def linear_small(x, w, b, silu_in):
    R, I = x.shape
    O = w.shape[0]
    y = empty((R, O), torch.float32, x.device)
    call("cesm_linear_small_fwd", P(x), P(w), P(b), P(y), R, I, O, int(silu_in), S())
    return y


def linear_small_bwd(x, w, dy, dx, dw, db, silu_in, accumulate_dx):
    R, I = x.shape
    O = w.shape[0]
    call("cesm_linear_small_bwd", P(x), P(w), P(dy), P(dx), P(dw), P(db), R, I, O, int(silu_in), int(accumulate_dx),
         1, S())


def q_sample(x0, noise, t, sa, s1a):
    B = x0.shape[0]
    xt = empty(x0.shape, torch.float32, x0.device)
    call("cesm_q_sample", P(x0), P(noise), P(t), P(sa), P(s1a), P(xt), B, x0.numel() // B, S())
    return xt


def ddpm_step(x, eps, z, t, sra, betas, s1a, pv, out=None):
    """Fused DDPM ancestral update (model.py:168-183); z=None drops the noise term; out may be x."""
    B = x.shape[0]
    _chk(x, dtype=torch.float32)
    _chk(eps, x.shape, torch.float32)
    if z is not None:
        _chk(z, x.shape, torch.float32)
    if out is None:
        out = empty(x.shape, torch.float32, x.device)
    call("cesm_ddpm_step", P(x), P(eps), P(z), P(t), P(sra), P(betas), P(s1a), P(pv), P(out), B, x.numel() // B, S())
    return out


def ddim_step(x, eps, z, t, t_prev, alphas_cumprod, eta, out=None):
    """Fused generalized DDIM update (cesm_ddim_step; coefficients: Diffusion.ddim_coefs): t, t_prev [B] int64 device
    tensors with t_prev < t < T (the caller's range check, the kernel has none); z=None or eta=0 drops the noise term;
    out may be x."""
    B = x.shape[0]
    _chk(x, dtype=torch.float32)
    _chk(eps, x.shape, torch.float32)
    if z is not None:
        _chk(z, x.shape, torch.float32)
    _chk(t, (B,), torch.int64)
    _chk(t_prev, (B,), torch.int64)
    _chk(alphas_cumprod, dtype=torch.float32)
    if alphas_cumprod.ndim != 1:
        raise RuntimeError("alphas_cumprod must be 1-D")
    eta = float(eta)
    if not eta >= 0.0:
        raise ValueError(f"eta must be >= 0, got {eta}")
    if out is None:
        out = empty(x.shape, torch.float32, x.device)
    else:
        _chk(out, x.shape, torch.float32)
    call("cesm_ddim_step", P(x), P(eps), P(z), P(t), P(t_prev), P(alphas_cumprod), eta, P(out), B, x.numel() // B,
         alphas_cumprod.numel(), S())
    return out


def dpmpp_step(x, eps, x0_last, t, t_prev, t_last, alphas_cumprod, out=None, x0_out=None):
    """Fused DPM-Solver++(2M) update (cesm_dpmpp_step; coefficients: Diffusion.dpmpp_coefs): returns (x_prev, x0).
    t, t_prev, t_last [B] int64 device tensors with -1 <= t_prev < t < T and t_last = -1 (no history) or
    t < t_last < T (the caller's range check; the kernel only clamps its table indices).  x0_last=None: no sample has
    history; with it, only the samples with t_prev >= 0 and t_last >= 0 read it.  out may be x, x0_out may be x0_last."""
    B = x.shape[0]
    _chk(x, dtype=torch.float32)
    _chk(eps, x.shape, torch.float32)
    if x0_last is not None:
        _chk(x0_last, x.shape, torch.float32)
    _chk(t, (B,), torch.int64)
    _chk(t_prev, (B,), torch.int64)
    _chk(t_last, (B,), torch.int64)
    _chk(alphas_cumprod, dtype=torch.float32)
    if alphas_cumprod.ndim != 1:
        raise RuntimeError("alphas_cumprod must be 1-D")
    if out is None:
        out = empty(x.shape, torch.float32, x.device)
    else:
        _chk(out, x.shape, torch.float32)
    if x0_out is None:
        x0_out = empty(x.shape, torch.float32, x.device)
    else:
        _chk(x0_out, x.shape, torch.float32)
    call("cesm_dpmpp_step", P(x), P(eps), P(x0_last), P(t), P(t_prev), P(t_last), P(alphas_cumprod), P(out), P(x0_out),
         B, x.numel() // B, alphas_cumprod.numel(), S())
    return out, x0_out


def guidance_scale_arg(scale, name="scale"):
    """a classifier-free-guidance scale as a float: a finite number >= 0 (no bool), else ValueError"""
    if isinstance(scale, bool) or not isinstance(scale, numbers.Real):
        raise ValueError(f"{name} must be a finite number >= 0, got {scale!r}")
    s = float(scale)
    if not (math.isfinite(s) and s >= 0.0):
        raise ValueError(f"{name} must be a finite number >= 0, got {scale!r}")
    return s


def _cfg_rows(x, eps, out):
    """the guided updates' x / eps / out: [2 B, ...] fp32 (eps_c rows, then eps_u rows); returns (B, HW, out)"""
    _chk(x, dtype=torch.float32)
    if x.ndim < 1 or x.shape[0] < 2 or x.shape[0] % 2:
        raise RuntimeError(f"guided update: x needs 2 B rows (conditional half, unconditional half), got "
                           f"{tuple(x.shape)}")
    _chk(eps, x.shape, torch.float32)
    if out is None:
        out = empty(x.shape, torch.float32, x.device)
    else:
        _chk(out, x.shape, torch.float32)
    B = x.shape[0] // 2
    return B, x.numel() // (2 * B), out


def ddpm_step_cfg(x, eps, z, t, sra, betas, s1a, pv, scale, out=None):
    """ddpm_step with classifier-free guidance fused in (cesm_ddpm_step_cfg): x, eps, out [2 B, ...] -- eps rows
    [0, B) are eps_c, rows [B, 2B) eps_u; x is read from rows [0, B) and x_prev written to both halves; z, t: B rows.
    scale: a finite number >= 0.  out may be x."""
    scale = guidance_scale_arg(scale)
    B, HW, out = _cfg_rows(x, eps, out)
    if z is not None:
        _chk(z, (B, *x.shape[1:]), torch.float32)
    _chk(t, (B,), torch.int64)
    call("cesm_ddpm_step_cfg", P(x), P(eps), P(z), P(t), P(sra), P(betas), P(s1a), P(pv), P(out), B, HW, scale, S())
    return out


def ddim_step_cfg(x, eps, z, t, t_prev, alphas_cumprod, eta, scale, out=None):
    """ddim_step with classifier-free guidance fused in (cesm_ddim_step_cfg): x, eps, out [2 B, ...] as in
    ddpm_step_cfg; z, t, t_prev: B rows.  scale: a finite number >= 0.  out may be x."""
    scale = guidance_scale_arg(scale)
    B, HW, out = _cfg_rows(x, eps, out)
    if z is not None:
        _chk(z, (B, *x.shape[1:]), torch.float32)
    _chk(t, (B,), torch.int64)
    _chk(t_prev, (B,), torch.int64)
    _chk(alphas_cumprod, dtype=torch.float32)
    if alphas_cumprod.ndim != 1:
        raise RuntimeError("alphas_cumprod must be 1-D")
    eta = float(eta)
    if not eta >= 0.0:
        raise ValueError(f"eta must be >= 0, got {eta}")
    call("cesm_ddim_step_cfg", P(x), P(eps), P(z), P(t), P(t_prev), P(alphas_cumprod), eta, P(out), B, HW,
         alphas_cumprod.numel(), scale, S())
    return out


def dpmpp_step_cfg(x, eps, x0_last, t, t_prev, t_last, alphas_cumprod, scale, out=None, x0_out=None):
    """dpmpp_step with classifier-free guidance fused in (cesm_dpmpp_step_cfg): returns (x_prev [2 B, ...], x0
    [B, ...]).  x, eps, out [2 B, ...] as in ddpm_step_cfg; x0_last, x0_out, t, t_prev, t_last: B rows.  scale: a
    finite number >= 0.  out may be x, x0_out may be x0_last."""
    scale = guidance_scale_arg(scale)
    B, HW, out = _cfg_rows(x, eps, out)
    rows = (B, *x.shape[1:])
    if x0_last is not None:
        _chk(x0_last, rows, torch.float32)
    _chk(t, (B,), torch.int64)
    _chk(t_prev, (B,), torch.int64)
    _chk(t_last, (B,), torch.int64)
    _chk(alphas_cumprod, dtype=torch.float32)
    if alphas_cumprod.ndim != 1:
        raise RuntimeError("alphas_cumprod must be 1-D")
    if x0_out is None:
        x0_out = empty(rows, torch.float32, x.device)
    else:
        _chk(x0_out, rows, torch.float32)
    call("cesm_dpmpp_step_cfg", P(x), P(eps), P(x0_last), P(t), P(t_prev), P(t_last), P(alphas_cumprod), P(out),
         P(x0_out), B, HW, alphas_cumprod.numel(), scale, S())
    return out, x0_out


def cond_mask(cond, keep, out=None):
    """out[b] = cond[b] where keep[b], else 0 (cesm_cond_mask: a select, a dropped sample's cond is not read).  cond
    [B, ...] fp32, keep [B] bool on the device; out may be cond."""
    _chk(cond, dtype=torch.float32)
    if cond.ndim < 2 or cond.numel() < 1:
        raise RuntimeError(f"cond must be a non-empty [B, ...], got {tuple(cond.shape)}")
    B = cond.shape[0]
    _chk(keep, (B,), torch.bool)
    if out is None:
        out = empty(cond.shape, torch.float32, cond.device)
    else:
        _chk(out, cond.shape, torch.float32)
    call("cesm_cond_mask", P(cond), P(keep), P(out), B, cond.numel() // B, S())
    return out


def mse(pred, tgt):
    loss = empty((), torch.float32, pred.device)
    part = empty((512,), torch.float32, pred.device)
    call("cesm_mse", P(pred), P(tgt), P(loss), P(part), pred.numel(), S())
    return loss


def mse_bwd(pred, tgt, gscale):
    d = empty(pred.shape, torch.float32, pred.device)
    call("cesm_mse_bwd", P(pred), P(tgt), P(gscale), P(d), pred.numel(), S())
    return d


def _wloss_args(pred, noise, w, row0, a, lam):
    """checks shared by wloss / wloss_bwd; returns (B, V, H, W, Hg, lam)"""
    _chk(pred, dtype=torch.float32)
    if pred.ndim != 4:
        raise RuntimeError(f"shape mismatch: pred must be [B, V, H, W], got {tuple(pred.shape)}")
    B, V, H, W = pred.shape
    _chk(noise, pred.shape, torch.float32)
    _chk(w, dtype=torch.float32)
    if w is None or w.ndim != 1 or w.numel() < H:
        raise RuntimeError(f"shape mismatch: w must be [Hg] with Hg >= H = {H}")
    _chk(row0, (B,), torch.int64)
    _chk(a, (B,), torch.float32)
    lam = float(lam)
    if not 0.0 <= lam <= 1.0:
        raise ValueError(f"lam must be in [0, 1], got {lam}")
    return B, V, H, W, w.numel(), lam


def wloss(pred, noise, w, row0, a, lam):
    """Weighted squared-error loss (cesm_wloss): [3] device tensor {mse_raw, mse_lat, total} of d = pred - noise
    [B, V, H, W] with row weights w [Hg], crop row offsets row0 [B] int64 (None: 0), per-sample weights a [B]
    (None: 1) and blend lam; total = mean(a[b] ((1 - lam) + lam w[row0[b] + h]) d^2).  row0 is a device tensor and is
    not range-checked here (the kernel clamps the row index into w; the caller validates)."""
    B, V, H, W, Hg, lam = _wloss_args(pred, noise, w, row0, a, lam)
    out = empty((3,), torch.float32, pred.device)
    part = empty((512 * 3,), torch.float32, pred.device)
    call("cesm_wloss", P(pred), P(noise), P(w), P(row0), P(a), lam, P(out), P(part), B, V, H, W, Hg, S())
    return out


def wloss_bwd(pred, noise, w, row0, a, lam, gscale):
    """d total / d pred of wloss, times gscale[0] (device fp32 [1])"""
    B, V, H, W, Hg, lam = _wloss_args(pred, noise, w, row0, a, lam)
    _chk(gscale, (1,), torch.float32)
    d = empty(pred.shape, torch.float32, pred.device)
    call("cesm_wloss_bwd", P(pred), P(noise), P(w), P(row0), P(a), lam, P(gscale), P(d), B, V, H, W, Hg, S())
    return d


ENS_MIN_M, ENS_MAX_M = 2, 128   # csrc/ensemble.hip
ENS_PART_BLOCKS = 2048           # block partials cesm_ens_stats may write (its `part` workspace)


def ens_stats(ens, obs, w, row0=None, mean=True, var=True, crps=None, rank=None, acc=True, accumulate=False):
    """Ensemble verification statistics (cesm_ens_stats; the per-pixel contract is in include/cesm_hip.h): one pass over
    ens [B, M, V, H, W] fp32 (2 <= M <= 128; an [B * M, V, H, W] sampler batch viewed, member m of condition b = row
    b M + m) against obs [B, V, H, W] or None, with row weights w [Hg] and crop row offsets row0 [B] int64 (None: 0; a
    device tensor, not range-checked: the kernel clamps the row index into w).

    mean / var / crps / rank select the maps ([B, V, H, W]; fp32, rank int32); crps and rank default to `obs is not
    None` and need it.  acc: True allocates the float64 [V, 4 + M + 1] accumulator, False leaves it out, a tensor is
    used as given (accumulate=True adds to it, else it is overwritten).  Row v of acc holds the sums, weighted with
    w[row0[b] + h], of 1, (mean - obs)^2, var, crps and [rank = r] for r = 0 .. M; without obs only columns 0 and 2 are
    written.  Returns {"mean", "var", "crps", "rank", "acc"} with None for what was left out."""
    if not torch.is_tensor(ens) or ens.ndim != 5:
        raise RuntimeError("shape mismatch: ens must be [B, M, V, H, W], got "
                           f"{tuple(ens.shape) if torch.is_tensor(ens) else type(ens).__name__}")
    B, M, V, H, W = ens.shape
    if M < ENS_MIN_M:
        raise ValueError(f"an ensemble needs at least {ENS_MIN_M} members (M - 1 divides the variance), got M = {M}")
    if M > ENS_MAX_M:
        raise NotImplementedError(f"cesm_ens_stats handles at most {ENS_MAX_M} members, got M = {M}")
    if min(B, V, H, W) < 1:
        raise RuntimeError(f"shape mismatch: empty ensemble {tuple(ens.shape)}")
    crps = (obs is not None) if crps is None else bool(crps)
    rank = (obs is not None) if rank is None else bool(rank)
    if obs is None and (crps or rank):
        raise ValueError("the crps and rank maps need obs")
    if obs is not None and (not torch.is_tensor(obs) or tuple(obs.shape) != (B, V, H, W)):
        raise RuntimeError(f"shape mismatch: obs must be {(B, V, H, W)}, got "
                           f"{tuple(obs.shape) if torch.is_tensor(obs) else type(obs).__name__}")
    if not torch.is_tensor(w) or w.ndim != 1 or w.numel() < H:
        raise RuntimeError(f"shape mismatch: w must be [Hg] with Hg >= H = {H}")
    if row0 is not None and (not torch.is_tensor(row0) or tuple(row0.shape) != (B,)):
        raise RuntimeError(f"shape mismatch: row0 must be [{B}]")
    own_acc = torch.is_tensor(acc)
    if own_acc and tuple(acc.shape) != (V, 4 + M + 1):
        raise RuntimeError(f"shape mismatch: acc must be {(V, 4 + M + 1)}, got {tuple(acc.shape)}")
    want_acc = own_acc or bool(acc)
    if not (mean or var or crps or rank or want_acc):
        raise ValueError("ens_stats: no output selected")
    _chk(ens, dtype=torch.float32)
    _chk(obs, dtype=torch.float32)
    _chk(w, dtype=torch.float32)
    _chk(row0, dtype=torch.int64)
    if own_acc:
        _chk(acc, dtype=torch.float64)
    for t in (obs, w, row0, acc if own_acc else None):
        if t is not None and t.device != ens.device:
            raise RuntimeError(f"tensors on different devices: {t.device} and {ens.device}")
    dev = ens.device
    out = {"mean": empty((B, V, H, W), torch.float32, dev) if mean else None,
           "var": empty((B, V, H, W), torch.float32, dev) if var else None,
           "crps": empty((B, V, H, W), torch.float32, dev) if crps else None,
           "rank": empty((B, V, H, W), torch.int32, dev) if rank else None,
           "acc": None}
    part = None
    if want_acc:
        if not own_acc:
            acc = empty((V, 4 + M + 1), torch.float64, dev)
            if accumulate:
                acc.zero_()
        out["acc"] = acc
        part = empty((ENS_PART_BLOCKS * (4 + M + 1),), torch.float32, dev)
    call("cesm_ens_stats", P(ens), P(obs), P(w), P(row0), P(out["mean"]), P(out["var"]), P(out["crps"]),
         P(out["rank"]), P(out["acc"]), P(part), B, M, V, H, W, w.numel(), int(bool(accumulate)), S())
    return out


def grad_norm(flat_grad, max_norm, loss=None):
    info = empty((4,), torch.float32, flat_grad.device)
    part = empty((1024,), torch.float64, flat_grad.device)
    call("cesm_grad_norm", P(flat_grad), flat_grad.numel(), float(max_norm), P(loss), P(part), P(info), S())
    return info


def adamw(p, g, m, v, info, lr, b1, b2, eps, wd, step_dev, use_clip):
    """step_dev: device int32 [1] step counter (advanced on device when the step is finite)"""
    _chk(step_dev, (1,), torch.int32)
    call("cesm_adamw", P(p), P(g), P(m), P(v), P(info), P(step_dev), p.numel(), float(lr), float(b1), float(b2),
         float(eps), float(wd), int(use_clip), S())


def adamw_ema(p, g, m, v, info, lr, b1, b2, eps, wd, step_dev, use_clip, ema, ema_n, ema_omd, beta, warmup):
    """adamw() plus, in the same launch, ema <- ema + (1 - decay) (p_new - ema) for a finite step.
    ema: fp32 like p; ema_n: device int32 [1] count of EMA updates (advanced on device); ema_omd: device fp32 [1]
    scratch; decay = min(beta, (1 + n) / (10 + n)) with warmup, beta without (ema.ema_decay)."""
    beta = float(beta)
    if not 0.0 <= beta < 1.0:
        raise ValueError(f"beta must be in [0, 1), got {beta}")
    for t in (p, g, m, v, info, step_dev, ema, ema_n, ema_omd):
        if not torch.is_tensor(t):
            raise TypeError(f"adamw_ema needs tensors, got {type(t).__name__}")
    n = p.numel()
    if p.ndim != 1 or n < 1:
        raise ValueError(f"flat buffers must be 1-D and non-empty, got shape {tuple(p.shape)}")
    for t in (p, g, m, v, ema):
        _chk(t, (n,), torch.float32)
    _chk(info, (4,), torch.float32)
    _chk(step_dev, (1,), torch.int32)
    _chk(ema_n, (1,), torch.int32)
    _chk(ema_omd, (1,), torch.float32)
    for t in (g, m, v, ema, info, step_dev, ema_n, ema_omd):
        if t.device != p.device:
            raise RuntimeError(f"tensors on different devices: {t.device} and {p.device}")
    call("cesm_adamw_ema", P(p), P(g), P(m), P(v), P(info), P(step_dev), n, float(lr), float(b1), float(b2),
         float(eps), float(wd), int(use_clip), P(ema), P(ema_n), P(ema_omd), beta, int(bool(warmup)), S())


def cast(x, dtype):
    y = empty(x.shape, dtype, x.device)
    call("cesm_cast", dtcode(x), _DT[dtype], P(x), P(y), x.numel(), S())
    return y


def window_gather(cond, tgt, items, K, h, w, center):
    T, M, H, W = cond.shape
    n = items.shape[0]
    cwin = empty((n, 1, K, h, w), torch.float32, items.device)
    x0 = empty((n, 1, h, w), torch.float32, items.device)
    call("cesm_window_gather", P(cond), P(tgt), P(items), P(cwin), P(x0), n, K, M, H, W, h, w, int(center), S())
    return cwin, x0


GATHER_MAX_V = 4  # cesm_window_gather_mv takes csel by value


def _gather_range(name, a, lo, hi, fn="window_gather_mv"):
    """ValueError naming the field and the first value of the CPU int64 tensor a outside [lo, hi]"""
    bad = (a < lo) | (a > hi)
    if bool(bad.any()):
        raise ValueError(f"{fn}: {name} = {int(a[bad][0])} outside [{lo}, {hi}]")


def window_gather_mv(cond, tgt, times, meta, csel, h, w, out=None):
    """V-variable window gather (cesm_window_gather_mv; the contract is in include/cesm_hip.h): cond [T, M, Vc, H, W]
    and tgt [T, M, V, H, W] fp32 on the GPU, times [n, K] and meta [n, 4] = (member, anchor, i, j) int64, csel: V
    indices into the Vc forcing planes.  Returns cwin [n, V, K, h, w], x0 [n, V, h, w] (out: that pair, to write into
    instead of allocating).

    CPU times / meta (what the loaders draw) are range-checked here, before anything is launched, and reach the device
    through one pinned staging buffer with a non-blocking copy; device times / meta are passed as they are and not read
    back (the kernel clamps every index)."""
    return _window_gather("window_gather_mv", cond, tgt, times, meta, csel, h, w, out, None)


def window_gather_mc(cond, tgt, times, meta, csel, h, w, out=None):
    """window_gather_mv with the cond plane count separated from V (cesm_window_gather_mc): csel holds Cc indices (1 ..
    4) into the Vc forcing planes, whatever V is.  Returns cwin [n, Cc, K, h, w], x0 [n, V, h, w]; everything else is
    window_gather_mv's."""
    return _window_gather("window_gather_mc", cond, tgt, times, meta, csel, h, w, out, len(csel))


def _window_gather(fn, cond, tgt, times, meta, csel, h, w, out, ncond):
    """the two gathers: ncond None is window_gather_mv (len(csel) must be V), else the count of cond planes"""
    for name, t, nd in (("cond", cond, 5), ("tgt", tgt, 5), ("times", times, 2), ("meta", meta, 2)):
        if not torch.is_tensor(t) or t.ndim != nd:
            raise RuntimeError(f"shape mismatch: {name} must be {nd}-D, got "
                               f"{tuple(t.shape) if torch.is_tensor(t) else type(t).__name__}")
    T, M, Vc, H, W = cond.shape
    V = tgt.shape[2]
    if tuple(tgt.shape) != (T, M, V, H, W):
        raise RuntimeError(f"shape mismatch: tgt {tuple(tgt.shape)} against cond {tuple(cond.shape)}")
    n, K = times.shape
    if tuple(meta.shape) != (n, 4):
        raise RuntimeError(f"shape mismatch: meta must be {(n, 4)}, got {tuple(meta.shape)}")
    for name, t, dt in (("cond", cond, torch.float32), ("tgt", tgt, torch.float32), ("times", times, torch.int64),
                        ("meta", meta, torch.int64)):
        if t.dtype != dt:
            raise RuntimeError(f"dtype mismatch: {name} is {t.dtype}, expected {dt}")
    h, w = int(h), int(w)
    csel = [int(c) for c in csel]
    Cc = V if ncond is None else int(ncond)
    if (not 1 <= V <= GATHER_MAX_V or not 1 <= Cc <= GATHER_MAX_V or len(csel) != Cc or K < 1 or n < 1 or
            min(T, M, Vc, h, w) < 1 or h > H or w > W):
        raise ValueError(f"{fn}: unsupported shape V={V} (1 .. {GATHER_MAX_V}) csel={csel} K={K} n={n} "
                         f"crop {h} x {w} of {H} x {W}")
    for c in csel:
        if not 0 <= c < Vc:
            raise ValueError(f"{fn}: csel = {c} outside [0, {Vc - 1}]")
    if times.device != meta.device:
        raise RuntimeError(f"tensors on different devices: {times.device} and {meta.device}")
    if not times.is_cuda:
        _gather_range("times", times, 0, T - 1, fn)
        _gather_range("member (meta[:, 0])", meta[:, 0], 0, M - 1, fn)
        _gather_range("anchor (meta[:, 1])", meta[:, 1], 0, T - 1, fn)
        _gather_range("i (meta[:, 2])", meta[:, 2], 0, H - h, fn)
        _gather_range("j (meta[:, 3])", meta[:, 3], 0, W - w, fn)
    _chk(cond)
    _chk(tgt)
    if tgt.device != cond.device:
        raise RuntimeError(f"tensors on different devices: {tgt.device} and {cond.device}")
    if times.is_cuda:
        _chk(times)
        _chk(meta)
        if times.device != cond.device:
            raise RuntimeError(f"tensors on different devices: {times.device} and {cond.device}")
    else:
        # one pinned block (the caching host allocator keeps it until the copy below has run), one copy, no synchronise
        stage = torch.empty(n * (K + 4), dtype=torch.int64, pin_memory=True)
        stage[:n * K].view(n, K).copy_(times)
        stage[n * K:].view(n, 4).copy_(meta)
        both = stage.to(cond.device, non_blocking=True)
        times, meta = both[:n * K].view(n, K), both[n * K:].view(n, 4)
    if out is None:
        cwin = empty((n, Cc, K, h, w), torch.float32, cond.device)
        x0 = empty((n, V, h, w), torch.float32, cond.device)
    else:
        cwin, x0 = out
        _chk(cwin, (n, Cc, K, h, w), torch.float32)
        _chk(x0, (n, V, h, w), torch.float32)
        if cwin.device != cond.device or x0.device != cond.device:
            raise RuntimeError(f"tensors on different devices: {cwin.device}, {x0.device} and {cond.device}")
    cs = csel + [0] * (GATHER_MAX_V - Cc)
    if ncond is None:
        _mv_call("cesm_window_gather_mv", f"V={V} Vc={Vc} csel={csel} K={K} crop {h} x {w} of {H} x {W}", P(cond),
                 P(tgt), P(times), P(meta), P(cwin), P(x0), n, K, V, Vc, *cs, T, M, H, W, h, w, S())
    else:
        _mv_call("cesm_window_gather_mc", f"V={V} Cc={Cc} Vc={Vc} csel={csel} K={K} crop {h} x {w} of {H} x {W}",
                 P(cond), P(tgt), P(times), P(meta), P(cwin), P(x0), n, K, V, Cc, Vc, *cs, T, M, H, W, h, w, S())
    return cwin, x0


def conv_fwd_variant(dtype, Nb, Hi, Wi, C1, C2, Ho, Wo, Cout, Co1, KH, KW, S, P, U):
    """name of the kernel cesm_conv_fwd selects for these arguments (host-only query)"""
    return lib().cesm_conv_fwd_variant(_DT[dtype], Nb, Hi, Wi, C1, C2, Ho, Wo, Cout, Co1, KH, KW, S, P, U).decode()


def tflash_bwd_variant(F, HW):
    """name of the dq kernel cesm_tflash_bwd selects (host-only query)"""
    return lib().cesm_tflash_bwd_variant(F, HW).decode()


def conv_wgrad_variant(dtype, Nb, Hi, Wi, C1, C2, Ho, Wo, Cout, Co1, KH, KW, S, P, U, with_bias=False):
    """name of the kernel cesm_conv_wgrad selects (host-only query)"""
    return lib().cesm_conv_wgrad_variant(_DT[dtype], Nb, Hi, Wi, C1, C2, Ho, Wo, Cout, Co1, KH, KW, S, P, U,
                                         int(bool(with_bias))).decode()
