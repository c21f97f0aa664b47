"""The stem kernels with the cond plane count Cc separated from V (cesm_stem_*_mc, csrc/multivar.h) against fp64
F.conv3d and its autograd on the CPU.

Conventions of test_gpu_multivar_kernels.py: the reference gets the operands as the kernel reads them (in bf16 mode
x_t, cond, w and dy rounded to bf16 first), every output buffer is NaN-filled before the launch, every case is launched
twice and must be bit-identical.  An input that the forward broadcasts over frames is an expanded leaf in the reference.

18 x 21 is one full 16 x 16 tile plus partial right and bottom tiles.  The twelve (V, Cc) with V != Cc cover P = V + Cc
= 3 .. 7: odd P leaves a last plane pair with one plane (the phantom plane), (1, 2) and (3, 4) have a pair that
straddles the x_t / cond boundary, P = 5 gives K = 245 taps (padded to 256: the padding taps read a staged halo element
against a zero weight).

Gates (relative L2 vs fp64): TOL of test_gpu_multivar_kernels.py: fp32 < 1e-5, bf16 < 1e-2.  The bf16 data gradient has
fp32 outputs and exact bf16 products, so on pre-rounded operands only the fp32 accumulation order is left: gate = 2 x
the measured worst case (DGRAD_BF16_MEASURED).
"""
import functools

import pytest
import torch
import torch.nn.functional as F

from cesm_emulator_amd import kernels as K
from cesm_emulator_amd._lib import lib

pytestmark = pytest.mark.gpu

TOL = {torch.float32: 1e-5, torch.bfloat16: 1e-2}
# measured on an MI355X, worst case over STEM_CASES (both outputs, and each alone): 7.919e-7 (dxt of the V = 2, Cc = 3,
# Co = 128 case; the fp32 kernel's worst is 2.37e-6 on the same case); the gate is 2x that
DGRAD_BF16_MEASURED = 7.919e-7
DGRAD_BF16_GATE = 2 * DGRAD_BF16_MEASURED

B, H, W = 2, 18, 21
FRAMES = [(3, 3, 3), (3, 1, 3), (3, 3, 1), (1, 1, 1)]   # (F, Fx, Fc)
PAIRS = [(V, Cc) for V in (1, 2, 3, 4) for Cc in (1, 2, 3, 4) if V != Cc]
#             V  Cc  Co  KS  F  Fx Fc
STEM_CASES = ([(V, Cc, 64, 7, 3, 1, 3) for V, Cc in PAIRS] +
              [(V, Cc, 64, 7, *fr) for V, Cc in ((1, 2), (2, 1), (3, 4)) for fr in FRAMES if fr != (3, 1, 3)] +
              [(1, 2, 64, 3, 3, 1, 3), (2, 3, 128, 7, 3, 1, 3)])
DTYPES = [torch.float32, torch.bfloat16]
stem_ids = lambda c: "V%d_Cc%d_Co%d_K%d_F%d_Fx%d_Fc%d" % c  # noqa: E731


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
    V, Cc, Co, KS, Fr, Fx, Fc = case
    g = torch.Generator().manual_seed(100000 * V + 10000 * Cc + 100 * Co + 10 * KS + 3 * Fr + Fx)
    xt = torch.randn(B, V, Fx, H, W, generator=g)
    cond = torch.randn(B, Cc, Fc, H, W, generator=g)
    w = torch.randn(Co, V + Cc, 1, KS, KS, generator=g) * 0.1
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


def launch_fwd(case, xt, cond, w, bias, y):
    V, Cc, Co, KS, Fr, Fx, Fc = case
    rc = lib().cesm_stem_fwd_mc(K._DT[y.dtype], K.P(xt), K.P(cond), K.P(w), K.P(bias), K.P(y), B, V, Cc, Fr, Fx, Fc, H,
                                W, Co, KS, K.S())
    assert rc == 0
    torch.cuda.synchronize()


def launch_wgrad(case, xt, cond, dy, dw, part, nblk):
    V, Cc, Co, KS, Fr, Fx, Fc = case
    rc = lib().cesm_stem_wgrad_mc(K.dtcode(dy), K.P(xt), K.P(cond), K.P(dy), K.P(dw), K.P(part), nblk, B, V, Cc, Fr, Fx,
                                  Fc, H, W, Co, KS, 0, K.S())
    assert rc == 0
    torch.cuda.synchronize()


def launch_dgrad(case, dy, w, dxt, dcond):
    V, Cc, Co, KS, Fr, Fx, Fc = case
    rc = lib().cesm_stem_dgrad_mc(K.dtcode(dy), K.P(dy), K.P(w), K.P(dxt), K.P(dcond), B, V, Cc, Fr, Fx, Fc, H, W, Co,
                                  KS, K.S())
    assert rc == 0
    torch.cuda.synchronize()


def run_fwd(case, cdt, xt, cond, w, bias):
    y = nan((B * case[4], H, W, case[2]), xt.device, cdt)
    launch_fwd(case, xt, cond, w, bias, y)
    return y


def run_wgrad(case, xt, cond, dy, nblk=7):
    """a small partials count (7 blocks over 18 pixel tiles per pair): blocks get 2 or 3 tiles each"""
    V, Cc, Co, KS, Fr, Fx, Fc = case
    dw = nan((Co, V + Cc, 1, KS, KS), xt.device)
    part = nan((nblk, Co * (V + Cc) * KS * KS), xt.device)
    launch_wgrad(case, xt, cond, dy, dw, part, nblk)
    assert not torch.isnan(part).any()   # every partial the reduction reads was written
    return dw


def run_dgrad(case, dy, w, want_xt=True, want_cond=True):
    V, Cc, Co, KS, Fr, Fx, Fc = case
    dxt, dcond = nan((B, V, Fx, H, W), dy.device), nan((B, Cc, Fc, H, W), dy.device)
    launch_dgrad(case, dy, w, dxt if want_xt else None, dcond if want_cond else None)
    return dxt, dcond


def dgrad_gate(cdt):
    return TOL[cdt] if cdt == torch.float32 else DGRAD_BF16_GATE


@pytest.mark.parametrize("cdt", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("case", STEM_CASES, ids=stem_ids)
def test_stem_fwd(dev, case, cdt):
    r = stem_ref(case, cdt)
    xt, cond, w, bias, dy = dev_ops(r, dev)
    y = run_fwd(case, cdt, xt, cond, w, bias)
    e = rel(y, r["y"])
    print(f"stem_fwd_mc {stem_ids(case)} {cdt}: rel {e:.3e}")
    assert torch.equal(y, run_fwd(case, cdt, xt, cond, w, bias))   # finite everywhere (NaN != NaN) and repeatable
    assert e < TOL[cdt]
    assert torch.equal(K.stem_fwd_mc(xt, cond, w, bias, case[4], cdt), y)


@pytest.mark.parametrize("cdt", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("case", STEM_CASES, ids=stem_ids)
def test_stem_wgrad(dev, case, cdt):
    r = stem_ref(case, cdt)
    xt, cond, w, bias, dy = dev_ops(r, dev)
    dw = run_wgrad(case, xt, cond, dy)
    e = rel(dw, r["dw"])
    print(f"stem_wgrad_mc {stem_ids(case)} {cdt}: rel {e:.3e}")
    assert torch.equal(dw, run_wgrad(case, xt, cond, dy))
    assert e < TOL[cdt]
    # the wrapper (512 partial blocks, most of them without a tile) accumulates onto dw
    acc = dw.clone()
    K.stem_wgrad_mc(xt, cond, dy, acc, case[4], accumulate=True)
    assert rel(acc, 2 * r["dw"]) < TOL[cdt]


@pytest.mark.parametrize("cdt", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("which", ["both", "dxt_null", "dcond_null"])
@pytest.mark.parametrize("case", STEM_CASES, ids=stem_ids)
def test_stem_dgrad(dev, case, which, cdt):
    """both outputs, and each alone: the null one's buffer (not passed) stays NaN.  With the broadcast output null the
    frames are split over blocks: a second launch geometry."""
    r = stem_ref(case, cdt)
    xt, cond, w, bias, dy = dev_ops(r, dev)
    want_xt, want_cond = which != "dxt_null", which != "dcond_null"
    dxt, dcond = run_dgrad(case, dy, w, want_xt, want_cond)
    dxt2, dcond2 = run_dgrad(case, dy, w, want_xt, want_cond)
    for name, want, got, again, ref in (("dxt", want_xt, dxt, dxt2, r["dxt"]),
                                        ("dcond", want_cond, dcond, dcond2, r["dcond"])):
        if not want:
            assert torch.isnan(got).all()
            continue
        e = rel(got, ref)
        print(f"stem_dgrad_mc {stem_ids(case)} {which} {cdt}: {name} rel {e:.3e}")
        assert torch.equal(got, again)
        assert e < dgrad_gate(cdt), name
    if which == "both":
        gx, gc = K.stem_dgrad_mc(dy, w, B, case[0], case[4], case[5], case[6])
        assert torch.equal(gx, dxt) and torch.equal(gc, dcond)


# ------------------------------------------------------------------------------------------------ the phantom plane
MARGIN = 512  # elements on each side: more than one plane (18 x 21 = 378) and than one weight row (7 x 49 = 343)


def guarded(t, dev):
    """(view, whole): a contiguous 16-byte-aligned copy of t in the middle of a larger NaN-filled allocation"""
    whole = nan((MARGIN + t.numel() + MARGIN,), dev, t.dtype)
    view = whole[MARGIN:MARGIN + t.numel()].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 == 0 and view.is_contiguous()
    return view, whole


def margins(whole):
    """the bits of both margins"""
    it = torch.int32 if whole.element_size() == 4 else torch.int16
    return torch.cat([whole[:MARGIN], whole[-MARGIN:]]).view(it).clone()


@pytest.mark.parametrize("cdt", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("case", [(1, 2, 64, 7, 3, 1, 3), (2, 3, 64, 7, 3, 1, 3), (3, 4, 64, 7, 3, 1, 3)], ids=stem_ids)
def test_phantom_plane_touches_nothing(dev, case, cdt):
    """odd P: the last plane pair has one plane.  Every tensor is a view inside a larger allocation whose margins are
    NaN: a read of the phantom plane or of its weights would poison a result, a write of its taps would change a
    margin (or the next output channel's row, which the gate sees)."""
    V, Cc, Co, KS, Fr, Fx, Fc = case
    r = stem_ref(case, cdt)
    nblk = 7
    ops = {k: guarded(r[k].contiguous(), dev) for k in ("xt", "cond", "w", "bias", "dy")}
    outs = dict(y=guarded(nan((B * Fr, H, W, Co), "cpu", cdt), dev),
                dw=guarded(nan((Co, V + Cc, 1, KS, KS), "cpu"), dev),
                part=guarded(nan((nblk, Co * (V + Cc) * KS * KS), "cpu"), dev),
                dxt=guarded(nan((B, V, Fx, H, W), "cpu"), dev),
                dcond=guarded(nan((B, Cc, Fc, H, W), "cpu"), dev))
    before = {k: margins(v[1]) for k, v in {**ops, **outs}.items()}
    xt, cond, w, bias, dy = (ops[k][0] for k in ("xt", "cond", "w", "bias", "dy"))
    launch_fwd(case, xt, cond, w, bias, outs["y"][0])
    launch_wgrad(case, xt, cond, dy, outs["dw"][0], outs["part"][0], nblk)
    launch_dgrad(case, dy, w, outs["dxt"][0], outs["dcond"][0])
    for k, gate in (("y", TOL[cdt]), ("dw", TOL[cdt]), ("dxt", dgrad_gate(cdt)), ("dcond", dgrad_gate(cdt))):
        got = outs[k][0]
        assert torch.isfinite(got).all(), k
        e = rel(got, r[k])
        print(f"phantom {stem_ids(case)} {cdt}: {k} rel {e:.3e}")
        assert e < gate, k
    assert torch.isfinite(outs["part"][0]).all()
    for k, v in {**ops, **outs}.items():
        assert torch.equal(margins(v[1]), before[k]), k


# ------------------------------------------------------------------------------------------------ Cc == V and refusals
@pytest.mark.parametrize("cdt", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("V", [1, 2])
def test_equal_counts_are_the_existing_path(dev, V, cdt):
    """Cc == V through the *_mc entries = the *_mv entries, bit for bit"""
    Co, KS, Fr, Fx, Fc = 64, 7, 3, 1, 3
    g = torch.Generator().manual_seed(7 + V)
    xt = torch.randn(B, V, Fx, H, W, generator=g).to(dev)
    cond = torch.randn(B, V, Fc, H, W, generator=g).to(dev)
    w = (torch.randn(Co, 2 * V, 1, KS, KS, generator=g) * 0.1).to(dev)
    bias = torch.randn(Co, generator=g).to(dev)
    dy = torch.randn(B * Fr, H, W, Co, generator=g).to(dev, cdt)
    assert torch.equal(K.stem_fwd_mc(xt, cond, w, bias, Fr, cdt), K.stem_fwd(xt, cond, w, bias, Fr, cdt))
    dw0, dw1 = nan(tuple(w.shape), dev), nan(tuple(w.shape), dev)
    K.stem_wgrad(xt, cond, dy, dw0, Fr, accumulate=False)
    K.stem_wgrad_mc(xt, cond, dy, dw1, Fr, accumulate=False)
    assert torch.equal(dw0, dw1)
    gx0, gc0 = K.stem_dgrad(dy, w, B, Fr, Fx, Fc)
    gx1, gc1 = K.stem_dgrad_mc(dy, w, B, V, Fr, Fx, Fc)
    assert torch.equal(gx1.view(gx0.shape), gx0) and torch.equal(gc1.view(gc0.shape), gc0)


def test_unsupported_shapes_raise(dev):
    Fr = 3
    b = torch.zeros(64, device=dev)
    dy = torch.zeros(B * Fr, H, W, 64, device=dev)
    xt1 = torch.zeros(B, 1, 1, H, W, device=dev)
    c5 = torch.zeros(B, 5, 1, H, W, device=dev)
    w6 = torch.zeros(64, 6, 1, 7, 7, device=dev)
    with pytest.raises(ValueError):   # Cc = 5
        K.stem_fwd_mc(xt1, c5, w6, b, Fr, torch.float32)
    with pytest.raises(ValueError):
        K.stem_wgrad_mc(xt1, c5, dy, torch.zeros_like(w6), Fr)
    with pytest.raises(ValueError):
        K.stem_dgrad_mc(dy, w6, B, 1, Fr, 1, 1)
    c2 = torch.zeros(B, 2, 1, H, W, device=dev)
    with pytest.raises(ValueError):   # KS > 7
        K.stem_fwd_mc(xt1, c2, torch.zeros(64, 3, 1, 9, 9, device=dev), b, Fr, torch.bfloat16)
    with pytest.raises(ValueError):   # Co no multiple of 64
        K.stem_fwd_mc(xt1, c2, torch.zeros(32, 3, 1, 7, 7, device=dev), torch.zeros(32, device=dev), Fr, torch.float32)
    with pytest.raises(ValueError):   # frame count neither 1 nor F
        K.stem_fwd_mc(torch.zeros(B, 1, 2, H, W, device=dev), c2, torch.zeros(64, 3, 1, 7, 7, device=dev), b, Fr,
                      torch.float32)
    with pytest.raises(RuntimeError):  # the inputs' channels do not add up to the weight's
        K.stem_fwd_mc(xt1, c2, torch.zeros(64, 4, 1, 7, 7, device=dev), b, Fr, torch.float32)
    with pytest.raises(ValueError):   # no conditioning map left
        K.stem_dgrad_mc(dy, torch.zeros(64, 3, 1, 7, 7, device=dev), B, 3, Fr, 1, 1)
