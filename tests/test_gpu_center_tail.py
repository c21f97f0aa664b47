"""The centre-frame tail of the network: only frame F // 2 reaches the head, so the residual 1x1 conv, the
last GroupNorm's apply and what the backward derives from the head's gradient alone run on that frame's B images.

1. the row-window GroupNorm entry points and the frame copies against the dense kernels, bit for bit;
2. out_conv through the executor, centre-frame path against the all-frames path;
3. the whole network, centre-frame path against the all-frames path, and F = 1 (always the all-frames path).

`torch.equal` treats -0 as equal to +0, the only difference that skipping exact-zero terms of a sum can make.
"""
import json
import os
from types import SimpleNamespace

import pytest
import torch

from cesm_emulator_amd import kernels as K
from cesm_emulator_amd import video_net as VN
from cesm_emulator_amd.model import UNet, Diffusion

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BF, F32 = torch.bfloat16, torch.float32

# (B, F, H, W, C, G): windows that start and end inside a reduction chunk, off the 32-row thread stride (HW = 35),
# HW = 1, the first possible window (F = 2: frame 1 is the last frame), B = 1
CASES = [(1, 2, 5, 7, 64, 8), (2, 3, 5, 7, 64, 8), (2, 12, 9, 33, 64, 8), (3, 5, 4, 36, 128, 8), (1, 12, 1, 1, 64, 8)]


def _case(dev, case, dt, with_ss, seed=0):
    B, Fr, H, W, C, G = case
    g = torch.Generator(device=dev).manual_seed(seed)
    HW = H * W
    c = SimpleNamespace(B=B, F=Fr, HW=HW, C=C, G=G, lo=(Fr // 2) * HW, n=HW)
    c.y = torch.randn(B * Fr, H, W, C, device=dev, generator=g).to(dt)
    c.gamma = 1 + 0.5 * torch.randn(C, device=dev, generator=g)
    c.beta = 0.5 * torch.randn(C, device=dev, generator=g)
    c.ss = 0.5 * torch.randn(B, 2 * C, device=dev, generator=g) if with_ss else None
    c.stats = K.gn_stats(c.y, B, G)
    c.comp = torch.randn(B, HW, C, device=dev, generator=g).to(dt)  # a compact [B][row_n][C] operand
    return c


def _rows(t, c):
    """a full tensor as [B, rows_b, C]"""
    return t.view(c.B, c.F * c.HW, c.C)


def _scattered(c, fill):
    """c.comp over the window rows of a full tensor otherwise holding `fill` (torch indexing, not the kernel)"""
    full = torch.full((c.B, c.F * c.HW, c.C), fill, device=c.y.device, dtype=c.y.dtype)
    full[:, c.lo:c.lo + c.n] = c.comp
    return full.view(c.y.shape)


@pytest.mark.parametrize("with_ss", [False, True])
@pytest.mark.parametrize("dt", [BF, F32])
@pytest.mark.parametrize("case", CASES)
def test_gn_apply_rows(dev, case, dt, with_ss):
    """gn_apply_rows == the window rows of gn_apply fed the scattered residual; rows of y outside the window are not
    read (NaN there changes nothing)"""
    c = _case(dev, case, dt, with_ss)
    y_nan = _rows(c.y.clone(), c)
    y_nan[:, :c.lo] = float("nan")
    y_nan[:, c.lo + c.n:] = float("nan")
    y_nan = y_nan.view(c.y.shape)
    for res_c in (None, c.comp):
        res = None if res_c is None else _scattered(c, 0.0)
        ref = _rows(K.gn_apply(c.y, c.stats, c.gamma, c.beta, c.ss, res, c.B, c.G), c)[:, c.lo:c.lo + c.n]
        out = K.gn_apply_rows(c.y, c.stats, c.gamma, c.beta, c.ss, res_c, c.B, c.G, c.lo, c.n)
        assert out.shape == (c.B, c.n, c.C)
        assert torch.equal(out, ref)
        assert torch.equal(K.gn_apply_rows(y_nan, c.stats, c.gamma, c.beta, c.ss, res_c, c.B, c.G, c.lo, c.n), ref)


@pytest.mark.parametrize("with_ss", [False, True])
@pytest.mark.parametrize("dt", [BF, F32])
@pytest.mark.parametrize("case", CASES)
def test_gn_bwd_rows(dev, case, dt, with_ss):
    """gn_bwd_rows(dout_c) == gn_bwd(dout_c scattered into zeros) on dy, dss, dgamma, dbeta and dbias (accumulated
    onto the same starting values), and on dy with every parameter-gradient pointer null"""
    c = _case(dev, case, dt, with_ss)
    dout_full = _scattered(c, 0.0)
    g = torch.Generator(device=dev).manual_seed(7)
    init = [torch.randn(c.C, device=dev, generator=g) for _ in range(3)]
    a = [t.clone() for t in init]
    b = [t.clone() for t in init]
    dy_ref, dss_ref = K.gn_bwd(dout_full, c.y, c.stats, c.gamma, c.beta, c.ss, a[0], a[1], c.B, c.G, True, dbias=a[2])
    dy, dss = K.gn_bwd_rows(c.comp, c.y, c.stats, c.gamma, c.beta, c.ss, b[0], b[1], c.B, c.G, True, c.lo, c.n,
                            dbias=b[2])
    assert dy.shape == c.y.shape
    assert torch.equal(dy, dy_ref)
    assert torch.equal(dss, dss_ref)
    for got, want, name in zip(b, a, ("dgamma", "dbeta", "dbias")):
        assert torch.equal(got, want), name
    dy0, dss0 = K.gn_bwd_rows(c.comp, c.y, c.stats, c.gamma, c.beta, c.ss, None, None, c.B, c.G, False, c.lo, c.n)
    assert dss0 is None and torch.equal(dy0, dy_ref)


@pytest.mark.parametrize("dt", [BF, F32])
@pytest.mark.parametrize("case", CASES)
def test_rows_gather_scatter(dev, case, dt):
    """gather -> scatter round-trips; scatter leaves the rows outside the window bit-unchanged (NaN-filled first)"""
    c = _case(dev, case, dt, False)
    comp = K.rows_gather(c.y, c.B, c.lo, c.n)
    assert comp.shape == (c.B, c.n, c.C)
    assert torch.equal(comp, _rows(c.y, c)[:, c.lo:c.lo + c.n])
    bits = torch.int16 if dt == BF else torch.int32
    full = torch.full(c.y.shape, float("nan"), device=dev, dtype=dt)
    before = _rows(full.clone(), c).view(bits)
    K.rows_scatter(comp, full, c.B, c.lo, c.n)
    after = _rows(full, c)
    assert torch.equal(after[:, c.lo:c.lo + c.n], comp)
    assert torch.equal(after.view(bits)[:, :c.lo], before[:, :c.lo])
    assert torch.equal(after.view(bits)[:, c.lo + c.n:], before[:, c.lo + c.n:])
    assert torch.equal(K.rows_gather(full, c.B, c.lo, c.n), comp)


def test_row_window_is_checked(dev):
    """a window that leaves the sample raises before anything is launched"""
    c = _case(dev, CASES[1], BF, False)
    for lo, n in ((c.lo + 1, c.n * 2), (-1, c.n), (0, 0)):
        with pytest.raises((RuntimeError, K.KernelError)):
            K.rows_gather(c.y, c.B, lo, n)
        with pytest.raises((RuntimeError, K.KernelError)):
            K.gn_apply_rows(c.y, c.stats, c.gamma, c.beta, None, None, c.B, c.G, lo, n)


# ------------------------------------------------------------------ out_conv, centre-frame path vs all-frames path
def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return (torch.linalg.vector_norm(a - b) / torch.linalg.vector_norm(b).clamp_min(1e-30)).item()


# the gate tests/test_gpu_prod_parity.py puts on a conv kernel's weight / bias gradient (e_dw, e_db < 1e-2 there)
WGRAD_REL_GATE = 1e-2


def _nan_empty(shape, dtype, device):
    """kernels.empty from a NaN-filled pool: whatever a kernel reads without anyone having written it shows up"""
    t = torch.empty(shape, dtype=dtype, device=device)
    return t.fill_(float("nan")) if t.is_floating_point() else t


def _run_out_block(monkeypatch, m, x, r, dout, B, Fr, center):
    monkeypatch.setattr(VN, "CENTER_TAIL", center)
    monkeypatch.setattr(K, "empty", _nan_empty)
    for p in m.out_conv.parameters():
        p.grad = None
    rc = VN.RunCtx(m, B, Fr, x.dtype, True)
    tape = SimpleNamespace()
    out = m.out_forward(rc, x, r, tape)
    assert (tape.out_rb.win is not None) == center and tape.head_F == (1 if center else Fr)
    dx, dr = m.out_backward(rc, dout, tape)
    torch.cuda.synchronize()
    grads = {n: p.grad.clone() for n, p in m.out_conv.named_parameters()}
    return SimpleNamespace(out=out, dx=dx, dr=dr, grads=grads)


@pytest.mark.parametrize("shape", [(2, 3, 8, 32), (1, 12, 9, 36)])
def test_out_block_center_vs_all_frames(dev, monkeypatch, shape):
    """head output, d/dx, d/dr and every parameter gradient of block1, block2 and the head: torch.equal.  The two
    res_conv gradients sum the same bf16 products in another split-K partition: each against a float64 sum, and the
    centre-frame path's error at most 2x the all-frames path's.  Every kernel output and workspace is NaN-filled
    before the launch, so a read of a row that the centre-frame path does not write would surface."""
    B, Fr, H, W = shape
    C = 64
    torch.manual_seed(3)
    net = UNet(ch_mults=(1, 2, 4)).to(dev)
    net.compute_dtype = BF
    m = net.net
    g = torch.Generator(device=dev).manual_seed(11)
    x = torch.randn(B * Fr, H, W, C, device=dev, generator=g).to(BF)
    r = torch.randn(B * Fr, H, W, C, device=dev, generator=g).to(BF)
    dout = torch.randn(B, 1, H, W, device=dev, generator=g)
    old = _run_out_block(monkeypatch, m, x, r, dout, B, Fr, False)
    new = _run_out_block(monkeypatch, m, x, r, dout, B, Fr, True)
    assert torch.equal(new.out, old.out) and torch.isfinite(new.out).all()
    assert torch.equal(new.dx, old.dx) and torch.isfinite(new.dx).all()
    assert torch.equal(new.dr, old.dr) and torch.isfinite(new.dr).all()
    special = ("0.res_conv.weight", "0.res_conv.bias")
    for name in old.grads:
        if name not in special:
            assert torch.equal(new.grads[name], old.grads[name]), name
    # float64 reference of the res_conv gradients: dW = dh^T cat(x, r), db = column sums of dh over the centre frames,
    # dh = the head's data gradient = dout (x) w_head rounded to bf16
    HW = H * W
    lo = (Fr // 2) * HW
    hw = m.out_conv[1].weight.reshape(-1)
    dh = (dout.reshape(B * HW, 1) * hw.reshape(1, C)).to(BF).double()
    xc = torch.cat([x.view(B, Fr * HW, C)[:, lo:lo + HW], r.view(B, Fr * HW, C)[:, lo:lo + HW]], 2).double()
    refs = {special[0]: (dh.t() @ xc.reshape(B * HW, 2 * C)), special[1]: dh.sum(0)}
    for name in special:
        e_new = rel(new.grads[name].reshape(refs[name].shape), refs[name])
        e_old = rel(old.grads[name].reshape(refs[name].shape), refs[name])
        print(f"{name} {shape}: rel err centre-frame path {e_new:.3e}, all-frames path {e_old:.3e}")
        assert e_new < WGRAD_REL_GATE and e_old < WGRAD_REL_GATE, (name, e_new, e_old)
        assert e_new <= 2 * e_old, (name, e_new, e_old)


# ------------------------------------------------------------------ whole network
def _loss_grads(d, x0, cond, t, noise):
    for p in d.parameters():
        p.grad = None
    loss = d.loss(x0, cond, t=t, noise=noise)
    loss.backward()
    torch.cuda.synchronize()
    return loss.detach().clone(), {n: p.grad.detach().clone() for n, p in d.named_parameters() if p.grad is not None}


def _net_and_inputs(dev, B, Fr, H, W):
    with open(os.path.join(ROOT, "config", "baseline")) as f:
        mults = tuple(json.load(f)["unet"]["ch_mults"])
    torch.manual_seed(1)
    net = UNet(ch_mults=mults).to(dev)
    net.compute_dtype = BF
    g = torch.Generator(device=dev).manual_seed(5)
    x0 = torch.randn(B, 1, H, W, device=dev, generator=g)
    cond = torch.randn(B, 1, Fr, H, W, device=dev, generator=g)
    noise = torch.randn(B, 1, H, W, device=dev, generator=g)
    t = torch.randint(0, 1000, (B,), device=dev, generator=g)
    return Diffusion(net).to(dev), (x0, cond, t, noise)


def test_whole_net_center_vs_all_frames(dev, monkeypatch):
    """baseline net, F = 8, 32 x 48, B = 2, bf16: the loss and every gradient but res_conv's two are bit-equal"""
    d, inp = _net_and_inputs(dev, 2, 8, 32, 48)
    monkeypatch.setattr(VN, "CENTER_TAIL", False)
    l_old, g_old = _loss_grads(d, *inp)
    monkeypatch.setattr(VN, "CENTER_TAIL", True)
    l_new, g_new = _loss_grads(d, *inp)
    assert torch.equal(l_new, l_old) and torch.isfinite(l_new)
    assert g_new.keys() == g_old.keys()
    special = [n for n in g_old if "out_conv.0.res_conv." in n]
    assert len(special) == 2
    for n in g_old:
        if n in special:
            assert rel(g_new[n], g_old[n]) < WGRAD_REL_GATE, n
        else:
            assert torch.equal(g_new[n], g_old[n]), n


def test_single_frame_takes_all_frames_path(dev, monkeypatch):
    """F = 1 has no other frame to skip: the switch changes nothing and the step works"""
    d, inp = _net_and_inputs(dev, 2, 1, 32, 48)
    monkeypatch.setattr(VN, "CENTER_TAIL", True)
    l_new, g_new = _loss_grads(d, *inp)
    monkeypatch.setattr(VN, "CENTER_TAIL", False)
    l_old, g_old = _loss_grads(d, *inp)
    assert torch.isfinite(l_new) and torch.equal(l_new, l_old)
    for n in g_old:
        assert torch.equal(g_new[n], g_old[n]), n
