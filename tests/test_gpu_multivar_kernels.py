"""The stem and head kernels for V target variables (csrc/multivar.h) against fp64 F.conv3d and its autograd on the CPU.

Conventions of test_gpu_stem_dgrad.py: the reference gets the operands as the kernel reads them (in bf16 mode x_t, cond,
w and dy rounded to bf16 first; the kernels convert the fp32 inputs and master weight themselves), every output buffer
is NaN-filled before the launch, every case is launched twice and must be bit-identical.  An input that the forward
broadcasts over frames is an expanded leaf in the reference, so autograd sums its gradient over the frames.

18 x 21 is one full 16 x 16 tile plus partial right and bottom tiles; the halo crosses all four borders.  V = 3 gives
K = 294 taps, no multiple of 32 (padded to 320 in the MFMA forward); KS = 3 gives K = 36 (padded to 64) and an 18-wide
halo inside the 22-wide LDS rows; Co = 128 is two 64-channel groups (grid.y in the forward and weight gradient, a loop
in the data gradient).

Gates (relative L2 vs fp64): the project's kernel gates, TOL of test_gpu_kernels.py: fp32 < 1e-5, bf16 < 1e-2 (bf16
output rounding).  The bf16 data gradient has fp32 outputs and exact bf16 products, so on pre-rounded operands only the
fp32 accumulation inside the MFMA is left: gate = 2 x the measured worst case (DGRAD_BF16_MEASURED).
"""
import functools

import pytest
import torch
import torch.nn.functional as F

from cesm_emulator_amd import kernels as K
from cesm_emulator_amd._lib import lib

pytestmark = pytest.mark.gpu

TOL = {torch.float32: 1e-5, torch.bfloat16: 1e-2}
# measured on an MI355X, worst case over STEM_CASES (both outputs, and each alone): 7.955e-7 (dxt of the V = 2,
# Co = 128 case; the fp32 kernel's worst is 2.25e-6 on the same case); the gate is 2x that
DGRAD_BF16_MEASURED = 7.955e-7
DGRAD_BF16_GATE = 2 * DGRAD_BF16_MEASURED

B, H, W = 2, 18, 21
FRAMES = [(3, 3, 3), (3, 1, 3), (3, 3, 1), (1, 1, 1)]   # (F, Fx, Fc)
#             V  Co   KS  F  Fx Fc
STEM_CASES = [(V, 64, 7, *fr) for V in (2, 3, 4) for fr in FRAMES] + [(2, 64, 3, 3, 1, 3), (2, 128, 7, 3, 1, 3)]
HEAD_CASES = [(V, C, Fr) for V in (2, 4) for C in (64, 128) for Fr in (1, 3)]
DTYPES = [torch.float32, torch.bfloat16]
stem_ids = lambda c: "V%d_Co%d_K%d_F%d_Fx%d_Fc%d" % c  # noqa: E731


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return (torch.linalg.vector_norm(a - b) / torch.linalg.vector_norm(b).clamp_min(1e-30)).item()


def to_cl(x):  # [B,C,F,H,W] -> [B*F,H,W,C]
    Bn, C, Fr, Hh, Ww = x.shape
    return x.permute(0, 2, 3, 4, 1).reshape(Bn * Fr, Hh, Ww, C).contiguous()


def q(x, cdt):
    return x.to(cdt).double()


@functools.lru_cache(maxsize=None)
def stem_ref(case, cdt):
    """CPU operands (fp32; dy already in the compute dtype) and the fp64 results on them, computed once per case"""
    V, Co, KS, Fr, Fx, Fc = case
    g = torch.Generator().manual_seed(10000 * V + 100 * Co + 10 * KS + 3 * Fr + Fx)
    xt = torch.randn(B, V, Fx, H, W, generator=g)
    cond = torch.randn(B, V, Fc, H, W, generator=g)
    w = torch.randn(Co, 2 * V, 1, KS, KS, generator=g) * 0.1
    bias = torch.randn(Co, generator=g)
    dy = torch.randn(B, Co, Fr, H, W, generator=g).to(cdt)
    xr, cr = q(xt, cdt).requires_grad_(True), q(cond, cdt).requires_grad_(True)
    wr = q(w, cdt).requires_grad_(True)
    x = torch.cat([xr.expand(-1, -1, Fr, -1, -1), cr.expand(-1, -1, Fr, -1, -1)], dim=1)
    y = F.conv3d(x, wr, bias.double(), padding=(0, KS // 2, KS // 2))
    gx, gc, gw = torch.autograd.grad(y, (xr, cr, wr), dy.double())
    return dict(xt=xt, cond=cond, w=w, bias=bias, dy=to_cl(dy), y=to_cl(y.detach()), dxt=gx, dcond=gc, dw=gw)


def nan(shape, dev, dtype=torch.float32):
    return torch.full(shape, float("nan"), device=dev, dtype=dtype)


def dev_ops(r, dev):
    return [r[k].to(dev).contiguous() for k in ("xt", "cond", "w", "bias", "dy")]


def run_fwd(case, cdt, xt, cond, w, bias):
    V, Co, KS, Fr, Fx, Fc = case
    y = nan((B * Fr, H, W, Co), xt.device, cdt)
    rc = lib().cesm_stem_fwd_mv(K._DT[cdt], K.P(xt), K.P(cond), K.P(w), K.P(bias), K.P(y), B, V, Fr, Fx, Fc, H, W, Co,
                                KS, K.S())
    assert rc == 0
    torch.cuda.synchronize()
    return y


def run_wgrad(case, xt, cond, dy, nblk=7):
    """a small partials count (7 blocks over 18 pixel tiles per pair): blocks get 2 or 3 tiles each"""
    V, Co, KS, Fr, Fx, Fc = case
    dw = nan((Co, 2 * V, 1, KS, KS), xt.device)
    part = nan((nblk, Co * 2 * V * KS * KS), xt.device)
    rc = lib().cesm_stem_wgrad_mv(K.dtcode(dy), K.P(xt), K.P(cond), K.P(dy), K.P(dw), K.P(part), nblk, B, V, Fr, Fx,
                                  Fc, H, W, Co, KS, 0, K.S())
    assert rc == 0
    torch.cuda.synchronize()
    assert not torch.isnan(part).any()   # every partial the reduction reads was written
    return dw


def run_dgrad(case, dy, w, want_xt=True, want_cond=True):
    V, Co, KS, Fr, Fx, Fc = case
    dxt, dcond = nan((B, V, Fx, H, W), dy.device), nan((B, V, Fc, H, W), dy.device)
    rc = lib().cesm_stem_dgrad_mv(K.dtcode(dy), K.P(dy), K.P(w), K.P(dxt if want_xt else None),
                                  K.P(dcond if want_cond else None), B, V, Fr, Fx, Fc, H, W, Co, KS, K.S())
    assert rc == 0
    torch.cuda.synchronize()
    return dxt, dcond


@pytest.mark.parametrize("cdt", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("case", STEM_CASES, ids=stem_ids)
def test_stem_fwd(dev, case, cdt):
    r = stem_ref(case, cdt)
    xt, cond, w, bias, dy = dev_ops(r, dev)
    y = run_fwd(case, cdt, xt, cond, w, bias)
    e = rel(y, r["y"])
    print(f"stem_fwd {stem_ids(case)} {cdt}: rel {e:.3e}")
    assert torch.equal(y, run_fwd(case, cdt, xt, cond, w, bias))   # finite everywhere (NaN != NaN) and repeatable
    assert e < TOL[cdt]


@pytest.mark.parametrize("cdt", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("case", STEM_CASES, ids=stem_ids)
def test_stem_wgrad(dev, case, cdt):
    r = stem_ref(case, cdt)
    xt, cond, w, bias, dy = dev_ops(r, dev)
    dw = run_wgrad(case, xt, cond, dy)
    e = rel(dw, r["dw"])
    print(f"stem_wgrad {stem_ids(case)} {cdt}: rel {e:.3e}")
    assert torch.equal(dw, run_wgrad(case, xt, cond, dy))
    assert e < TOL[cdt]
    # the wrapper (512 partial blocks, most of them without a tile) accumulates onto dw
    acc = dw.clone()
    K.stem_wgrad(xt, cond, dy, acc, case[3], accumulate=True)
    assert rel(acc, 2 * r["dw"]) < TOL[cdt]


def dgrad_gate(cdt):
    return TOL[cdt] if cdt == torch.float32 else DGRAD_BF16_GATE


@pytest.mark.parametrize("cdt", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("case", STEM_CASES, ids=stem_ids)
def test_stem_dgrad(dev, case, cdt):
    r = stem_ref(case, cdt)
    xt, cond, w, bias, dy = dev_ops(r, dev)
    dxt, dcond = run_dgrad(case, dy, w)
    ex, ec = rel(dxt, r["dxt"]), rel(dcond, r["dcond"])
    print(f"stem_dgrad {stem_ids(case)} {cdt}: dxt rel {ex:.3e}  dcond rel {ec:.3e}")
    dxt2, dcond2 = run_dgrad(case, dy, w)
    assert torch.equal(dxt, dxt2) and torch.equal(dcond, dcond2)
    assert ex < dgrad_gate(cdt) and ec < dgrad_gate(cdt)


@pytest.mark.parametrize("cdt", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("which", ["dxt_null", "dcond_null"])
@pytest.mark.parametrize("case", [STEM_CASES[1], STEM_CASES[9]], ids=stem_ids)   # V = 2 and V = 4, x_t broadcast
def test_stem_dgrad_null_output(dev, case, which, cdt):
    """one output null: the other is complete and correct, the null one's buffer (not passed) stays NaN.  With dxt
    null no requested output is a broadcast one, so the frames are split over blocks: a second launch geometry."""
    r = stem_ref(case, cdt)
    xt, cond, w, bias, dy = dev_ops(r, dev)
    want_xt = which == "dcond_null"
    dxt, dcond = run_dgrad(case, dy, w, want_xt=want_xt, want_cond=not want_xt)
    got, ref, other = (dxt, r["dxt"], dcond) if want_xt else (dcond, r["dcond"], dxt)
    e = rel(got, ref)
    print(f"stem_dgrad {stem_ids(case)} {which} {cdt}: rel {e:.3e}")
    assert torch.isnan(other).all()
    again = run_dgrad(case, dy, w, want_xt=want_xt, want_cond=not want_xt)[0 if want_xt else 1]
    assert torch.equal(got, again)
    assert e < dgrad_gate(cdt)


# ------------------------------------------------------------------------------------------------ head
@functools.lru_cache(maxsize=None)
def head_ref(case, cdt):
    V, C, Fr = case
    g = torch.Generator().manual_seed(1000 * V + 10 * C + Fr)
    x = torch.randn(B, C, Fr, H, W, generator=g).to(cdt)
    w = torch.randn(V, C, 1, 1, 1, generator=g) * 0.2
    bias = torch.randn(V, generator=g)
    dout = torch.randn(B, V, H, W, generator=g)
    xr = x.double().requires_grad_(True)
    wr, br = w.double().requires_grad_(True), bias.double().requires_grad_(True)
    out = F.conv3d(xr, wr, br)[:, :, Fr // 2]
    gx, gw, gb = torch.autograd.grad(out, (xr, wr, br), dout.double())
    return dict(x=to_cl(x), w=w, bias=bias, dout=dout, out=out.detach(), dx=to_cl(gx), dw=gw, db=gb)


def run_head_bwd(case, x, w, dout, nblk=5):
    V, C, Fr = case
    dx = nan(tuple(x.shape), x.device, x.dtype)
    dw, db = nan((V, C), x.device), nan((V,), x.device)
    part = nan((nblk, V * (C + 1)), x.device)
    rc = lib().cesm_head_bwd_mv(K.dtcode(x), K.P(dout), K.P(x), K.P(w), K.P(dx), K.P(dw), K.P(db), K.P(part), nblk, B, V,
                                Fr, H * W, C, 0, K.S())
    assert rc == 0
    torch.cuda.synchronize()
    assert not torch.isnan(part).any()
    return dx, dw, db


@pytest.mark.parametrize("cdt", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("case", HEAD_CASES, ids=lambda c: "V%d_C%d_F%d" % c)
def test_head(dev, case, cdt):
    V, C, Fr = case
    r = head_ref(case, cdt)
    x, w, bias, dout = [r[k].to(dev).contiguous() for k in ("x", "w", "bias", "dout")]

    def fwd():
        out = nan((B, V, H, W), dev)
        assert lib().cesm_head_fwd_mv(K.dtcode(x), K.P(x), K.P(w), K.P(bias), K.P(out), B, V, Fr, H * W, C, K.S()) == 0
        torch.cuda.synchronize()
        return out
    out = fwd()
    dx, dw, db = run_head_bwd(case, x, w, dout)
    errs = dict(out=rel(out, r["out"]), dx=rel(dx, r["dx"]), dw=rel(dw, r["dw"].view(V, C)), db=rel(db, r["db"]))
    print(f"head V={V} C={C} F={Fr} {cdt}: " + "  ".join(f"{k} {v:.3e}" for k, v in errs.items()))
    assert torch.equal(out, fwd())
    dx2, dw2, db2 = run_head_bwd(case, x, w, dout)
    assert torch.equal(dx, dx2) and torch.equal(dw, dw2) and torch.equal(db, db2)
    for k, e in errs.items():
        assert e < TOL[cdt], k
    # the wrappers: module-shaped weight, allocate, accumulate; no gradient buffers -> dx only
    assert torch.equal(K.head_fwd(x, w, bias, B, Fr), out)
    gw, gb = dw.clone().view(V, C, 1, 1, 1), db.clone()
    assert torch.equal(K.head_bwd(dout, x, w, gw, gb, B, Fr), dx)
    assert rel(gw, 2 * r["dw"]) < TOL[cdt] and rel(gb, 2 * r["db"]) < TOL[cdt]
    assert torch.equal(K.head_bwd(dout, x, w, None, None, B, Fr), dx)


# ------------------------------------------------------------------------------------------------ V = 1 and refusals
@pytest.mark.parametrize("cdt", DTYPES, ids=["fp32", "bf16"])
def test_single_variable_is_the_existing_path(dev, cdt):
    """V = 1 through the wrappers and the *_mv entries = the single-variable entry points, bit for bit"""
    Co, KS, Fr, Fx, Fc, C = 64, 7, 3, 1, 3, 64
    g = torch.Generator().manual_seed(7)
    xt = torch.randn(B, 1, Fx, H, W, generator=g).to(dev)
    cond = torch.randn(B, 1, Fc, H, W, generator=g).to(dev)
    w = (torch.randn(Co, 2, 1, KS, KS, generator=g) * 0.1).to(dev)
    bias = torch.randn(Co, generator=g).to(dev)
    dy = torch.randn(B * Fr, H, W, Co, generator=g).to(dev, cdt)
    L, dt = lib(), K._DT[cdt]
    y0 = nan((B * Fr, H, W, Co), dev, cdt)
    assert L.cesm_stem_fwd(dt, K.P(xt), K.P(cond), K.P(w), K.P(bias), K.P(y0), B, Fr, Fx, Fc, H, W, Co, KS, K.S()) == 0
    assert torch.equal(K.stem_fwd(xt, cond, w, bias, Fr, cdt), y0)
    assert torch.equal(K.stem_fwd(xt[:, 0], cond[:, 0], w, bias, Fr, cdt), y0)   # variable axis left out
    dw0, part = nan(tuple(w.shape), dev), nan((512, w.numel()), dev)
    assert L.cesm_stem_wgrad(dt, K.P(xt), K.P(cond), K.P(dy), K.P(dw0), K.P(part), 512, B, Fr, Fx, Fc, H, W, Co, KS, 0,
                             K.S()) == 0
    dw1 = nan(tuple(w.shape), dev)
    K.stem_wgrad(xt, cond, dy, dw1, Fr, accumulate=False)
    assert torch.equal(dw1, dw0)
    gx0, gc0 = nan((B, Fx, H, W), dev), nan((B, Fc, H, W), dev)
    assert L.cesm_stem_dgrad(dt, K.P(dy), K.P(w), K.P(gx0), K.P(gc0), B, Fr, Fx, Fc, H, W, Co, KS, K.S()) == 0
    gx1, gc1 = K.stem_dgrad(dy, w, B, Fr, Fx, Fc)
    assert torch.equal(gx1, gx0) and torch.equal(gc1, gc0)
    hx = torch.randn(B * Fr, H, W, C, generator=g).to(dev, cdt)
    hw, hb = torch.randn(1, C, 1, 1, 1, generator=g).to(dev), torch.randn(1, generator=g).to(dev)
    dout = torch.randn(B, 1, H, W, generator=g).to(dev)
    o0 = nan((B, 1, H, W), dev)
    assert L.cesm_head_fwd(dt, K.P(hx), K.P(hw), K.P(hb), K.P(o0), B, Fr, H * W, C, K.S()) == 0
    assert torch.equal(K.head_fwd(hx, hw, hb, B, Fr), o0)
    dx0, hdw0, hdb0, hp = nan(tuple(hx.shape), dev, cdt), nan((C,), dev), nan((1,), dev), nan((256, C + 1), dev)
    assert L.cesm_head_bwd(dt, K.P(dout), K.P(hx), K.P(hw), K.P(dx0), K.P(hdw0), K.P(hdb0), K.P(hp), 256, B, Fr, H * W,
                           C, 0, K.S()) == 0
    hdw1, hdb1 = nan((1, C, 1, 1, 1), dev), nan((1,), dev)
    dx1 = K.head_bwd(dout, hx, hw, hdw1, hdb1, B, Fr, accumulate=False)
    torch.cuda.synchronize()
    assert torch.equal(dx1, dx0) and torch.equal(hdw1.view(-1), hdw0) and torch.equal(hdb1, hdb0)


def test_unsupported_shapes_raise(dev):
    Fr = 3
    xt5 = torch.zeros(B, 5, 1, H, W, device=dev)
    w5 = torch.zeros(64, 10, 1, 7, 7, device=dev)
    b = torch.zeros(64, device=dev)
    dy = torch.zeros(B * Fr, H, W, 64, device=dev)
    with pytest.raises(ValueError):   # V = 5
        K.stem_fwd(xt5, xt5, w5, b, Fr, torch.float32)
    with pytest.raises(ValueError):
        K.stem_wgrad(xt5, xt5, dy, torch.zeros_like(w5), Fr)
    with pytest.raises(ValueError):
        K.stem_dgrad(dy, w5, B, Fr, 1, 1)
    xt2 = torch.zeros(B, 2, 1, H, W, device=dev)
    with pytest.raises(ValueError):   # KS > 7
        K.stem_fwd(xt2, xt2, torch.zeros(64, 4, 1, 9, 9, device=dev), b, Fr, torch.bfloat16)
    with pytest.raises(ValueError):   # odd channel count: no 2V
        K.stem_fwd(xt2, xt2, torch.zeros(64, 3, 1, 7, 7, device=dev), b, Fr, torch.float32)
    with pytest.raises(ValueError):   # frame count neither 1 nor F
        K.stem_fwd(torch.zeros(B, 2, 2, H, W, device=dev), xt2, torch.zeros(64, 4, 1, 7, 7, device=dev), b, Fr,
                   torch.float32)
    with pytest.raises(RuntimeError):  # cond's channels do not match the weight's V
        K.stem_fwd(xt2, torch.zeros(B, 1, 1, H, W, device=dev), torch.zeros(64, 4, 1, 7, 7, device=dev), b, Fr,
                   torch.float32)
    hx = torch.zeros(B * Fr, H, W, 64, device=dev)
    with pytest.raises(ValueError):   # 5 head outputs
        K.head_fwd(hx, torch.zeros(5, 64, device=dev), torch.zeros(5, device=dev), B, Fr)
    with pytest.raises(ValueError):   # weight no multiple of C
        K.head_fwd(hx, torch.zeros(100, device=dev), torch.zeros(1, device=dev), B, Fr)
