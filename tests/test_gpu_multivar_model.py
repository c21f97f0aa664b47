"""The whole network with V target variables against oracle/ref_cpu.py (CPU fp32): UNet(out_channels=V) on the HIP
stem and head of csrc/multivar.h.  ch_mults = (1, 2, 4), B = 2, 16 x 24, V in {2, 3}.

Gates are those of test_gpu_model.py (fp32 forward < 1e-5, loss < 1e-5, parameter gradients < 1e-4, bf16 forward
< 5e-2), of test_gpu_input_grad.py's setting for the input gradients (< 1e-4) and of the sampler tests (graph == eager
bit for bit, < 1e-4 against the oracle's loop).  Every oracle result is computed once and shared.
"""
import functools

import pytest
import torch
import torch.nn.functional as F

from cesm_emulator_amd import input_grads
from cesm_emulator_amd.model import UNet, Diffusion
from cesm_emulator_amd.train import make_optimizer, train_step
from oracle import ref_cpu as R

pytestmark = pytest.mark.gpu

MULTS = (1, 2, 4)
B, H, W = 2, 16, 24
T_SAMPLE = 8


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return (torch.linalg.vector_norm(a - b) / torch.linalg.vector_norm(b).clamp_min(1e-30)).item()


@functools.lru_cache(maxsize=None)
def ref_net(V):
    torch.manual_seed(1)
    return R.UNet(out_channels=V, ch_mults=MULTS)


def make_prod(V, dev, cdt):
    prod = UNet(out_channels=V, ch_mults=MULTS)
    prod.load_state_dict(ref_net(V).state_dict(), strict=True)
    prod = prod.to(dev)
    prod.compute_dtype = cdt
    return prod


@functools.lru_cache(maxsize=None)
def inputs(V, Fr, seed=0):
    g = torch.Generator().manual_seed(seed + 10 * V + Fr)
    x0 = torch.randn(B, V, H, W, generator=g)
    cond = torch.randn(B, V, Fr, H, W, generator=g)
    t = torch.randint(0, 1000, (B,), generator=g)
    noise = torch.randn(B, V, H, W, generator=g)
    return x0, cond, t, noise


@functools.lru_cache(maxsize=None)
def oracle_forward(V, Fr):
    x0, cond, t, _ = inputs(V, Fr)
    with torch.no_grad():
        return ref_net(V)(x0, cond, t)


@functools.lru_cache(maxsize=None)
def oracle_loss_grads(V):
    """the oracle's Diffusion.loss at F = 3 with x_t and cond as leaves: loss, d/d x_t, d/d cond, parameter gradients"""
    ref = ref_net(V)
    x0, cond, t, noise = inputs(V, 3)
    ref.zero_grad(set_to_none=True)
    d = R.Diffusion(ref)
    x_t = d.q_sample(x0, t, noise)[0].detach().requires_grad_(True)
    c = cond.clone().requires_grad_(True)
    loss = F.mse_loss(ref(x_t, c, t), noise)
    loss.backward()
    pg = {n: p.grad.clone() for n, p in ref.named_parameters() if p.grad is not None}
    ref.zero_grad(set_to_none=True)
    return loss.item(), x_t.grad.clone(), c.grad.clone(), pg


@pytest.mark.parametrize("Fr", [3, 1])
@pytest.mark.parametrize("V", [2, 3])
def test_forward_parity_fp32(dev, V, Fr):
    prod = make_prod(V, dev, torch.float32)
    x0, cond, t, _ = inputs(V, Fr)
    with torch.no_grad():
        y = prod(x0.to(dev), cond.to(dev), t.to(dev))
    assert y.shape == (B, V, H, W)
    err = rel(y, oracle_forward(V, Fr))
    print(f"fwd rel err fp32 V={V} F={Fr}: {err:.3e}")
    assert err < 1e-5


def test_forward_accepts_4d_cond(dev):
    """cond [B, V, H, W] is the F = 1 window"""
    V = 2
    prod = make_prod(V, dev, torch.float32)
    x0, cond, t, _ = inputs(V, 1)
    with torch.no_grad():
        y = prod(x0.to(dev), cond[:, :, 0].to(dev), t.to(dev))
    assert rel(y, oracle_forward(V, 1)) < 1e-5


@pytest.mark.parametrize("V", [2, 3])
def test_loss_and_gradients_fp32(dev, V):
    prod = make_prod(V, dev, torch.float32)
    d = Diffusion(prod).to(dev)
    x0, cond, t, noise = inputs(V, 3)
    l_ref, _, _, pg = oracle_loss_grads(V)
    lp = d.loss(x0.to(dev), cond.to(dev), t=t.to(dev), noise=noise.to(dev))
    lp.backward()
    print(f"V={V}: loss {lp.item():.6f} vs {l_ref:.6f}")
    assert abs(lp.item() - l_ref) / abs(l_ref) < 1e-5
    worst = 0.0
    pr = dict(prod.named_parameters())
    assert set(pg) == {n for n, p in pr.items() if p.requires_grad}
    for name, g in pg.items():
        assert pr[name].grad is not None, name
        e = rel(pr[name].grad, g)
        worst = max(worst, e)
        assert e < 1e-4, (name, e)
    print(f"V={V}: worst parameter gradient rel err {worst:.3e}")


def test_input_grads_fp32(dev):
    V = 2
    prod = make_prod(V, dev, torch.float32)
    d = Diffusion(prod).to(dev)
    x0, cond, t, noise = inputs(V, 3)
    l_ref, gx, gc, _ = oracle_loss_grads(V)
    loss, dxt, dcond = input_grads(d, x0.to(dev), cond.to(dev), t=t.to(dev), noise=noise.to(dev))
    assert dxt.shape == x0.shape and dcond.shape == cond.shape
    ex, ec = rel(dxt, gx), rel(dcond, gc)
    print(f"input_grads V={V}: loss rel {abs(loss.item() - l_ref) / abs(l_ref):.3e}, dx_t rel {ex:.3e}, "
          f"dcond rel {ec:.3e}")
    assert abs(loss.item() - l_ref) / abs(l_ref) < 1e-5
    assert ex < 1e-4 and ec < 1e-4
    assert all(p.grad is None for p in prod.parameters())


def test_bf16_forward_and_repeatable_train_step(dev):
    V = 2
    x0, cond, t, noise = inputs(V, 3)
    args = [a.to(dev) for a in (x0, cond)]
    prod = make_prod(V, dev, torch.bfloat16)
    with torch.no_grad():
        y = prod(args[0], args[1], t.to(dev))
    err = rel(y, oracle_forward(V, 3))
    print(f"fwd rel err bf16 V={V}: {err:.3e}")
    assert err < 5e-2
    params = []
    for _ in range(2):   # identical state, identical step
        d = Diffusion(make_prod(V, dev, torch.bfloat16)).to(dev)
        opt = make_optimizer(d, {})
        loss = train_step(d, opt, args[0], args[1], 1.0, t=t.to(dev), noise=noise.to(dev))
        torch.cuda.synchronize()
        assert torch.isfinite(loss)
        params.append((loss.clone(), {n: p.detach().clone() for n, p in d.model.named_parameters()}))
    assert torch.equal(params[0][0], params[1][0])
    bad = [n for n, p in params[0][1].items() if not torch.equal(p, params[1][1][n])]
    assert not bad, bad[:5]
    moved = [n for n, p in params[0][1].items() if not torch.equal(p.cpu(), dict(ref_net(V).named_parameters())[n])]
    assert "net.input_conv.weight" in moved and "net.out_conv.1.weight" in moved   # the step reached both ends


@functools.lru_cache(maxsize=None)
def sampler_case():
    V = 2
    g = torch.Generator().manual_seed(11)
    shape = (B, V, H, W)
    cond = torch.randn(B, V, H, W, generator=g)
    x_T = torch.randn(shape, generator=g)
    noise_seq = torch.randn(T_SAMPLE, *shape, generator=g)
    y_ref = R.Diffusion(ref_net(V), timesteps=T_SAMPLE).sample(cond, shape, "cpu", x_T=x_T, noise_seq=noise_seq)
    return shape, cond, x_T, noise_seq, y_ref


def test_sampler_graph_eager_oracle(dev):
    shape, cond, x_T, noise_seq, y_ref = sampler_case()
    d = Diffusion(make_prod(2, dev, torch.float32), timesteps=T_SAMPLE).to(dev)
    c, xT, ns = cond.to(dev), x_T.to(dev), noise_seq.to(dev)
    y_eager = d.sample(c, shape, dev, use_graph=False, x_T=xT, noise_seq=ns)
    y_graph = d.sample(c, shape, dev, use_graph=True, x_T=xT, noise_seq=ns)
    assert y_graph.shape == shape
    assert torch.equal(y_eager, y_graph)
    err = rel(y_graph, y_ref)
    print(f"sample V=2 T={T_SAMPLE} vs the oracle loop: rel {err:.3e}")
    assert err < 1e-4
    z_eager = d.sample(c, shape, dev, use_graph=False, x_T=xT, steps=4, ddim_eta=0.0)
    z_graph = d.sample(c, shape, dev, use_graph=True, x_T=xT, steps=4, ddim_eta=0.0)
    assert torch.isfinite(z_graph).all() and torch.equal(z_eager, z_graph)


def test_channel_mismatch_raises(dev):
    prod = make_prod(2, dev, torch.float32)
    x0, cond, t, _ = inputs(2, 3)
    with pytest.raises(ValueError, match="x_t has 2 channels and cond 1"):
        prod(x0.to(dev), cond[:, :1].to(dev), t.to(dev))
    with pytest.raises(ValueError, match="x_t has 1 channels and cond 2"):
        prod(x0[:, :1].to(dev), cond.to(dev), t.to(dev))
