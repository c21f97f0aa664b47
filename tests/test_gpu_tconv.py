"""Temporal-conv blocks (UNet(use_temp_attn=False)) on the GPU: csrc/tconv.h against torch, kernel by kernel and through
the whole network (oracle/ref_cpu.py with the blocks swapped, tests/tconv_ref.py).

Gates
  fp32 kernels   forward relative L2 < 1e-5; dx, dW, db, dgamma < 1e-4 against a float64 torch composition (the
                 project's fp32 gates)
  bf16 kernels   each output's relative L2 error against float64 (on the same bf16-rounded x / dy) at most 1.5 x the
                 error of a torch emulation with the kernel's rounding points (fp32 LayerNorm of the bf16 input, n and W
                 rounded to bf16, fp32 accumulation, the residual, one rounding at the end), the project's bf16 convention
  network fp32   forward < 1e-5, loss < 1e-5, every parameter and input gradient < 1e-4 against the swapped oracle
  network bf16   forward < 5e-2; training steps bit-repeatable, and bit-identical under the LDS / register polluters
Shapes: B = 2, F in {1, 2, 3, 12, 20}, 5 x 7 (35 pixels: no full tile) and 16 x 24, C in {64, 128}: F = 1, 2 pad on both
sides at once, F = 20 is two frame runs of the bf16 kernels (16 + 4), 16 x 24 = 384 pixels is several pixel tiles.
"""
import contextlib
import ctypes
import functools
import os

import pytest
import torch
import torch.nn.functional as TF

from cesm_emulator_amd import kernels as K
from cesm_emulator_amd import input_grads
from cesm_emulator_amd.ema import EMA
from cesm_emulator_amd.model import UNet, Diffusion
from cesm_emulator_amd.optim import FusedAdamW
from oracle import ref_cpu as R
from tests.tconv_ref import swapped_oracle, randomize_tconv

pytestmark = pytest.mark.gpu

EPS = 1e-5
SHAPES = [(F, H, W, C) for C in (64, 128) for (H, W) in ((5, 7), (16, 24)) for F in (1, 2, 3, 12, 20)]
B = 2


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return (torch.linalg.vector_norm(a - b) / torch.linalg.vector_norm(b).clamp_min(1e-30)).item()


def ln(x, gamma, dt):
    x = x.to(dt)
    mean = x.mean(-1, keepdim=True)
    var = x.var(-1, unbiased=False, keepdim=True)
    return (x - mean) / torch.sqrt(var + EPS) * gamma.to(dt)


def fconv(n, w, bias, Bn, F):
    """n [B*F, H, W, C] -> sum_k W[:, :, k] n[f + k - 1] + bias, same layout"""
    Nb, H, W, C = n.shape
    t = n.view(Bn, F, H * W, C).permute(0, 2, 3, 1).reshape(Bn * H * W, C, F)
    y = TF.conv1d(t, w, bias, padding=1)
    return y.view(Bn, H * W, C, F).permute(0, 3, 1, 2).reshape(Nb, H, W, C)


def block(x, gamma, w, bias, Bn, F, dt, rnd=None):
    """x + bias + conv(LN(x) gamma); rnd: a rounding applied to n and W (the bf16 kernel's operands)"""
    n = ln(x, gamma, dt)
    w = w.to(dt)
    if rnd is not None:
        n, w = rnd(n), rnd(w)
    return x.to(dt) + fconv(n, w, bias.to(dt), Bn, F)


class _RoundBf16(torch.autograd.Function):
    """round to bf16 in the forward, pass the gradient through (the kernel's backward re-derives the same rounded n)"""

    @staticmethod
    def forward(ctx, t):
        return t.bfloat16().to(t.dtype)

    @staticmethod
    def backward(ctx, g):
        return g


def grads(x, gamma, w, bias, dy, Bn, F, dt, rnd=None):
    x, gamma, w, bias = (t.detach().to(dt).requires_grad_(True) for t in (x, gamma, w, bias))
    y = block(x, gamma, w, bias, Bn, F, dt, rnd)
    y.backward(dy.to(dt))
    return {"y": y.detach(), "dx": x.grad, "dw": w.grad, "db": bias.grad, "dgamma": gamma.grad}


@functools.lru_cache(maxsize=None)
def case(F, H, W, C):
    """inputs of one shape (CPU) and their float64 results, computed once"""
    g = torch.Generator().manual_seed(1000 * C + 100 * F + H)
    x = torch.randn(B * F, H, W, C, generator=g) * 1.5 + 0.3
    dy = torch.randn(B * F, H, W, C, generator=g)
    gamma = 1 + 0.2 * torch.randn(C, generator=g)
    w = torch.randn(C, C, 3, generator=g) * 0.05
    bias = torch.randn(C, generator=g) * 0.1
    return x, dy, gamma, w, bias


@functools.lru_cache(maxsize=None)
def ref64(F, H, W, C, bf16_inputs):
    x, dy, gamma, w, bias = case(F, H, W, C)
    if bf16_inputs:
        x, dy = x.bfloat16().float(), dy.bfloat16().float()
    return grads(x, gamma, w, bias, dy, B, F, torch.float64)


def run_kernels(dev, x, dy, gamma, w, bias, Bn, F, cdt, want=("dgamma", "dw", "db"), prefill=None):
    C = x.shape[-1]
    xd, dyd = x.to(dev, cdt).contiguous(), dy.to(dev, cdt).contiguous()
    gd, wd, bd = gamma.to(dev), w.to(dev).contiguous(), bias.to(dev)
    wp = K.conv_pack(wd, cdt, C, C, 1, 3, 0, 0)
    wpt = K.conv_pack(wd, cdt, C, C, 1, 3, 1, 1)
    y, mr = K.tconv_fwd(xd, gd, wp, bd, Bn, F, save=True, eps=EPS)
    y0, none = K.tconv_fwd(xd, gd, wp, bd, Bn, F, save=False, eps=EPS)
    assert none is None and torch.equal(y, y0)
    out = {"y": y, "mr": mr}
    shapes = {"dgamma": (C,), "dw": (C, C, 3), "db": (C,)}
    dst = {k: (torch.zeros(shapes[k], device=dev) if prefill is None else prefill[k].to(dev).clone()) if k in want else None
           for k in shapes}
    out["dx"] = K.tconv_bwd(xd, dyd, mr, gd, wpt, dst["dgamma"], dst["dw"], dst["db"], Bn, F, eps=EPS)
    out.update(dst)
    torch.cuda.synchronize()
    return out


# ------------------------------------------------------------------------------------------ 1: kernels, fp32
@pytest.mark.parametrize("F,H,W,C", SHAPES)
def test_kernels_fp32(dev, F, H, W, C):
    x, dy, gamma, w, bias = case(F, H, W, C)
    ref = ref64(F, H, W, C, False)
    got = run_kernels(dev, x, dy, gamma, w, bias, B, F, torch.float32)
    errs = {k: rel(got[k], ref[k]) for k in ("y", "dx", "dw", "db", "dgamma")}
    print(f"tconv fp32 F={F} {H}x{W} C={C}: " + " ".join(f"{k}={v:.2e}" for k, v in errs.items()))
    assert errs["y"] < 1e-5
    for k in ("dx", "dw", "db", "dgamma"):
        assert errs[k] < 1e-4, (k, errs[k])
    # the saved statistics are the LayerNorm's
    xx = x.double().view(-1, C)
    mr = got["mr"].double().cpu()
    assert rel(mr[:, 0], xx.mean(-1)) < 1e-5
    assert rel(mr[:, 1], 1 / torch.sqrt(xx.var(-1, unbiased=False) + EPS)) < 1e-5


@pytest.mark.parametrize("cdt", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("F,H,W,C", [(3, 5, 7, 64), (20, 16, 24, 64), (2, 16, 24, 128)])
def test_accumulate_null_destinations_and_sample_boundary(dev, cdt, F, H, W, C):
    x, dy, gamma, w, bias = case(F, H, W, C)
    full = run_kernels(dev, x, dy, gamma, w, bias, B, F, cdt)
    # repeatable bit for bit
    again = run_kernels(dev, x, dy, gamma, w, bias, B, F, cdt)
    for k in ("y", "dx", "dw", "db", "dgamma"):
        assert torch.equal(full[k], again[k]), k
    # (+)= into pre-filled destinations
    g = torch.Generator().manual_seed(5)
    pre = {"dgamma": torch.randn(C, generator=g), "dw": torch.randn(C, C, 3, generator=g), "db": torch.randn(C, generator=g)}
    acc = run_kernels(dev, x, dy, gamma, w, bias, B, F, cdt, prefill=pre)
    for k, p in pre.items():
        assert torch.allclose(acc[k], p.to(dev) + full[k], rtol=1e-6, atol=1e-6 * full[k].abs().max().item()), k
    # a null destination is skipped and leaves the others bit-identical
    for drop in ("dgamma", "dw", "db"):
        part = run_kernels(dev, x, dy, gamma, w, bias, B, F, cdt, want=tuple(k for k in pre if k != drop))
        assert part[drop] is None
        for k in ("y", "dx", "dw", "db", "dgamma"):
            if k != drop:
                assert torch.equal(part[k], full[k]), (drop, k)
    none = run_kernels(dev, x, dy, gamma, w, bias, B, F, cdt, want=())
    assert torch.equal(none["dx"], full["dx"])
    # frames never mix across samples: B = 2 is two B = 1 calls, bit for bit
    h = x.shape[0] // 2
    for s in range(2):
        one = run_kernels(dev, x[s * h:(s + 1) * h], dy[s * h:(s + 1) * h], gamma, w, bias, 1, F, cdt)
        assert torch.equal(one["y"], full["y"][s * h:(s + 1) * h]), "y: frames leak across samples"
        assert torch.equal(one["dx"], full["dx"][s * h:(s + 1) * h]), "dx: frames leak across samples"


# ------------------------------------------------------------------------------------------ 2: kernels, bf16
@pytest.mark.parametrize("F,H,W,C", SHAPES)
def test_kernels_bf16(dev, F, H, W, C):
    x, dy, gamma, w, bias = case(F, H, W, C)
    xb, dyb = x.bfloat16().float(), dy.bfloat16().float()
    ref = ref64(F, H, W, C, True)
    emu = grads(xb, gamma, w, bias, dyb, B, F, torch.float32, rnd=_RoundBf16.apply)
    emu["y"], emu["dx"] = emu["y"].bfloat16(), emu["dx"].bfloat16()  # the one rounding at the end
    got = run_kernels(dev, x, dy, gamma, w, bias, B, F, torch.bfloat16)
    line, bad = [], []
    for k in ("y", "dx", "dw", "db", "dgamma"):
        e_k, e_e = rel(got[k], ref[k]), rel(emu[k], ref[k])
        line.append(f"{k}={e_k:.2e}/{e_e:.2e}")
        if not e_k <= 1.5 * e_e:
            bad.append((k, e_k, e_e))
    print(f"tconv bf16 F={F} {H}x{W} C={C} (kernel/emulation vs float64): " + " ".join(line))
    assert not bad, bad


def test_kernel_c256_bf16_and_fp32(dev):
    """the widest supported block (weights re-read per frame instead of register-resident): same gates"""
    F, H, W, C = 3, 5, 7, 256
    x, dy, gamma, w, bias = case(F, H, W, C)
    ref = ref64(F, H, W, C, False)
    got = run_kernels(dev, x, dy, gamma, w, bias, B, F, torch.float32)
    assert rel(got["y"], ref["y"]) < 1e-5
    for k in ("dx", "dw", "db", "dgamma"):
        assert rel(got[k], ref[k]) < 1e-4, k
    refb = ref64(F, H, W, C, True)
    emu = grads(x.bfloat16().float(), gamma, w, bias, dy.bfloat16().float(), B, F, torch.float32, rnd=_RoundBf16.apply)
    emu["y"], emu["dx"] = emu["y"].bfloat16(), emu["dx"].bfloat16()
    gotb = run_kernels(dev, x, dy, gamma, w, bias, B, F, torch.bfloat16)
    for k in ("y", "dx", "dw", "db", "dgamma"):
        assert rel(gotb[k], refb[k]) <= 1.5 * rel(emu[k], refb[k]), k


def test_unsupported_width_is_an_error(dev):
    x = torch.zeros(2, 4, 4, 96, device=dev)
    with pytest.raises(ValueError, match="96"):
        K.tconv_fwd(x, torch.ones(96, device=dev), torch.zeros(96, 288, device=dev), torch.zeros(96, device=dev), 1, 2)


# ------------------------------------------------------------------------------------------ 3: whole network, fp32
MULTS, NB, NF, NH, NW = (1, 2, 4, 8), 2, 3, 32, 48


def net_inputs(Bn, Fr, H, W, seed=3):
    g = torch.Generator().manual_seed(seed)
    x0 = torch.randn(Bn, 1, H, W, generator=g)
    cond = torch.randn(Bn, 1, Fr, H, W, generator=g)
    t = torch.randint(0, 1000, (Bn,), generator=g)
    noise = torch.randn(Bn, 1, H, W, generator=g)
    return x0, cond, t, noise


@functools.lru_cache(maxsize=None)
def oracle_net(mults):
    torch.manual_seed(1)
    return randomize_tconv(swapped_oracle(mults))


@functools.lru_cache(maxsize=None)
def oracle_run():
    """the swapped oracle's forward and backward at (1, 2, 4, 8), B = 2, F = 3, 32 x 48, once"""
    ref = oracle_net(MULTS)
    ref.zero_grad(set_to_none=True)
    x0, cond, t, noise = net_inputs(NB, NF, NH, NW)
    x_t = R.Diffusion(ref).q_sample(x0, t, noise)[0].detach().requires_grad_(True)
    c = cond.clone().requires_grad_(True)
    y = ref(x_t, c, t)
    loss = TF.mse_loss(y, noise)
    loss.backward()
    pg = {n: p.grad.clone() for n, p in ref.named_parameters() if p.grad is not None}
    ref.zero_grad(set_to_none=True)
    return x_t.detach(), cond, t, noise, y.detach(), loss.item(), x_t.grad.clone(), c.grad.clone(), pg


def make_prod(ref, dev, cdt, mults):
    prod = UNet(use_temp_attn=False, ch_mults=mults)
    prod.load_state_dict(ref.state_dict(), strict=True)
    prod = prod.to(dev)
    prod.compute_dtype = cdt
    return prod


def test_network_fp32_matches_swapped_oracle(dev):
    x_t, cond, t, noise, y_ref, loss_ref, dxt_ref, dcond_ref, pg = oracle_run()
    prod = make_prod(oracle_net(MULTS), dev, torch.float32, MULTS)
    xr = x_t.to(dev).requires_grad_(True)
    cr = cond.to(dev).requires_grad_(True)
    y = prod(xr, cr, t.to(dev))
    loss = TF.mse_loss(y, noise.to(dev))
    loss.backward()
    e = rel(y.detach(), y_ref)
    print(f"tconv network fp32: fwd {e:.2e} loss {abs(loss.item() - loss_ref) / abs(loss_ref):.2e}")
    assert e < 1e-5
    assert abs(loss.item() - loss_ref) / abs(loss_ref) < 1e-5
    worst = ("", 0.0)
    seen = 0
    for name, p in prod.named_parameters():
        if name not in pg:
            continue
        assert p.grad is not None, name
        eg = rel(p.grad, pg[name])
        worst = max(worst, (name, eg), key=lambda v: v[1])
        seen += "temporal_conv" in name
        assert eg < 1e-4, (name, eg)
    assert seen == 6
    print(f"worst parameter gradient: {worst[0]} {worst[1]:.2e}; dcond {rel(cr.grad, dcond_ref):.2e} "
          f"dx_t {rel(xr.grad, dxt_ref):.2e}")
    assert rel(cr.grad, dcond_ref) < 1e-4 and rel(xr.grad, dxt_ref) < 1e-4


def test_input_grads_only_leaves_parameters_alone(dev):
    """saliency.input_grads through the temporal-conv blocks: the oracle's input gradients, and no p.grad created"""
    x_t, cond, t, noise, y_ref, loss_ref, dxt_ref, dcond_ref, pg = oracle_run()
    prod = make_prod(oracle_net(MULTS), dev, torch.float32, MULTS)
    d = Diffusion(prod).to(dev)
    x0, _, _, _ = net_inputs(NB, NF, NH, NW)
    loss, dxt, dcond = input_grads(d, x0.to(dev), cond.to(dev), t=t.to(dev), noise=noise.to(dev))
    assert all(p.grad is None for p in prod.parameters())
    assert abs(loss.item() - loss_ref) / abs(loss_ref) < 1e-5
    assert rel(dcond, dcond_ref) < 1e-4 and rel(dxt, dxt_ref) < 1e-4
    # frozen temporal-conv parameters: their gradients are not computed, the others are unchanged
    for n, p in prod.named_parameters():
        if "temporal_conv" in n:
            p.requires_grad_(False)
    y = prod(x_t.to(dev), cond.to(dev), t.to(dev))
    TF.mse_loss(y, noise.to(dev)).backward()
    for n, p in prod.named_parameters():
        if "temporal_conv" in n:
            assert p.grad is None, n
        elif n in pg:
            assert rel(p.grad, pg[n]) < 1e-4, n


def test_network_fp32_single_frame(dev):
    """(1, 2, 4), F = 1 (the sampler's forward): the centre tap alone"""
    mults = (1, 2, 4)
    ref = oracle_net(mults)
    prod = make_prod(ref, dev, torch.float32, mults)
    x0, cond, t, noise = net_inputs(2, 1, 16, 24, seed=4)
    with torch.no_grad():
        y_ref = ref(x0, cond, t)
        y = prod(x0.to(dev), cond.to(dev), t.to(dev))
    e = rel(y, y_ref)
    print(f"tconv network fp32 F=1: fwd {e:.2e}")
    assert e < 1e-5


def test_two_train_steps_match_oracle(dev):
    """AdamW + clip twice: the second step runs on weight images re-packed after the first (stale packs would show)"""
    mults = (1, 2, 4)
    torch.manual_seed(1)
    ref = randomize_tconv(swapped_oracle(mults))
    prod = make_prod(ref, dev, torch.float32, mults)
    dref, dprod = R.Diffusion(ref), Diffusion(prod).to(dev)
    opt_r = R.make_optimizer(dref)
    opt_p = FusedAdamW(dprod.parameters(), lr=2e-4, betas=(0.9, 0.999), weight_decay=1e-4, max_grad_norm=1.0)
    for step in range(2):
        x0, cond, t, noise = net_inputs(2, 3, 32, 48, seed=10 + step)
        lr_ = R.train_step(dref, opt_r, x0, cond, t=t, noise=noise)
        opt_p.zero_grad()
        lp = dprod.loss(x0.to(dev), cond.to(dev), t=t.to(dev), noise=noise.to(dev))
        lp.backward()
        opt_p.step(loss=lp.detach())
        assert abs(lp.item() - lr_.item()) / abs(lr_.item()) < 1e-5
    pr = dict(prod.named_parameters())
    worst, frac_bad = 0.0, 0.0
    for name, p in ref.named_parameters():
        d = (pr[name].detach().cpu().double() - p.detach().double()).abs()
        worst = max(worst, rel(pr[name].detach(), p.detach()))
        frac_bad = max(frac_bad, (d > 0.05 * 2e-4).double().mean().item())
    print(f"tconv params after 2 steps: worst rel err {worst:.3e}, worst fraction off by >5% of lr {frac_bad:.2e}")
    assert worst < 1e-4 and frac_bad < 1e-3


# ------------------------------------------------------------------------------------------ 4: whole network, bf16
def test_network_bf16_close(dev):
    x_t, cond, t, noise, y_ref, *_ = oracle_run()
    prod = make_prod(oracle_net(MULTS), dev, torch.bfloat16, MULTS)
    with torch.no_grad():
        y = prod(x_t.to(dev), cond.to(dev), t.to(dev))
    e = rel(y, y_ref)
    print(f"tconv network bf16: fwd {e:.2e}")
    assert e < 5e-2


def bf16_step(dev, ctx=contextlib.nullcontext()):
    torch.manual_seed(3)
    net = randomize_tconv(UNet(use_temp_attn=False, ch_mults=MULTS)).to(dev)
    net.compute_dtype = torch.bfloat16
    d = Diffusion(net).to(dev)
    x0, cond, t, noise = (v.to(dev) for v in net_inputs(1, 12, 32, 48, seed=5))
    with ctx:
        loss = d.loss(x0, cond, t=t, noise=noise)
        loss.backward()
        torch.cuda.synchronize()
    out = {"loss": loss.detach().clone()}
    out.update({n: p.grad.detach().clone() for n, p in net.named_parameters() if p.grad is not None})
    return out


def test_bf16_train_step_is_bit_repeatable(dev):
    a, b = bf16_step(dev), bf16_step(dev)
    assert len(a) > 100 and sum("temporal_conv" in k for k in a) == 6
    for k in a:
        assert torch.isfinite(a[k].float()).all(), k
        assert torch.equal(a[k], b[k]), k


DIAG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "diag", "libvgpr_pollute.so")
PATTERNS = (0x7FC07FC0, 0, 0x3F800000, 0x7F7F7F7F)


@pytest.fixture(scope="module")
def pol():
    assert os.path.exists(DIAG), "tools/diag/libvgpr_pollute.so missing: run __graft_entry__.build()"
    lib = ctypes.CDLL(DIAG)
    for fn in (lib.vgpr_pollute, lib.lds_pollute):
        fn.argtypes = [ctypes.c_uint, ctypes.c_int, ctypes.c_void_p]
    return lib


@contextlib.contextmanager
def polluted(monkeypatch, pol, bits):
    """every kernels.call preceded by the LDS and register polluters on the current stream"""
    orig = K.call

    def call(name, *args):
        st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        assert pol.lds_pollute(bits, 2048, st) == 0 and pol.vgpr_pollute(bits, 8192, st) == 0
        return orig(name, *args)

    with monkeypatch.context() as m:
        m.setattr(K, "call", call)
        yield


def test_bf16_train_step_independent_of_stale_state(dev, monkeypatch, pol):
    res = [bf16_step(dev, polluted(monkeypatch, pol, bits)) for bits in PATTERNS]
    for k, r in enumerate(res):
        for nm, t in r.items():
            assert torch.isfinite(t.float()).all(), f"pattern {k}: non-finite {nm}"
            assert torch.equal(t, res[0][nm]), f"pattern {k}: {nm} depends on stale LDS / register contents"


# ------------------------------------------------------------------------------------------ 5: sampling
@pytest.mark.parametrize("cdt", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_graph_sampler_equals_eager_and_ema_samples(dev, cdt):
    torch.manual_seed(1)
    net = randomize_tconv(UNet(use_temp_attn=False, ch_mults=(1, 2, 4))).to(dev)
    net.compute_dtype = cdt
    d = Diffusion(net).to(dev)
    shape = (2, 1, 16, 24)
    g = torch.Generator().manual_seed(11)
    cond = torch.randn(*shape, generator=g).to(dev)
    x_T = torch.randn(*shape, generator=g).to(dev)

    def sample(use_graph):
        return d.sample(cond, shape, dev, steps=3, use_graph=use_graph, x_T=x_T).clone()

    y_eager, y_graph = sample(False), sample(True)
    assert torch.isfinite(y_graph).all()
    assert torch.equal(y_graph, y_eager)
    # one optimizer step, then the EMA's weights: the sample is what a fresh network with those weights gives
    opt = FusedAdamW(d.parameters(), lr=1e-3, max_grad_norm=1.0)
    ema = EMA(net, opt, beta=0.5, warmup=False)
    with ema.applied(d):
        s0 = sample(True)
    x0, c5, t, noise = (v.to(dev) for v in net_inputs(2, 3, 16, 24, seed=6))
    opt.zero_grad()
    loss = d.loss(x0, c5, t=t, noise=noise)
    loss.backward()
    opt.step(loss=loss.detach())
    with ema.applied(d):
        s1 = sample(True)
    assert d.model is net and torch.isfinite(s1).all() and not torch.equal(s1, s0)
    fresh = UNet(use_temp_attn=False, ch_mults=(1, 2, 4)).to(dev)
    fresh.load_state_dict(ema.ema_model.state_dict())
    fresh.compute_dtype = cdt
    fresh.eval()
    d.model = fresh
    want = sample(True)
    d.model = net
    assert torch.equal(s1, want), "ema_model sampled from stale packed weights"
    # and a compute_dtype change re-packs too
    other = torch.float32 if cdt == torch.bfloat16 else torch.bfloat16
    net.compute_dtype = other
    y_other = sample(False)
    net.compute_dtype = cdt
    assert torch.isfinite(y_other).all() and torch.equal(sample(False), sample(True))
