"""The whole network with Cc conditioning maps for V target variables, UNet(out_channels=V, cond_channels=Cc), against
oracle/ref_cpu.py (CPU fp32).  The oracle is its UNet(out_channels=V) with net.input_conv replaced by a
Conv3d(V + Cc -> 64, (1, 7, 7)): its forward only concatenates x_t and cond, so nothing else changes; the weights go
over through state_dict.  ch_mults = (1, 2, 4), B = 2, 16 x 24, F = 3, (V, Cc) in {(1, 3), (2, 3)}.

Gates are those of test_gpu_multivar_model.py for the same quantities: fp32 forward < 1e-5, loss < 1e-5, parameter
gradients < 1e-4, input gradients < 1e-4, bf16 forward < 5e-2, graph == eager bit for bit, the sampler < 1e-4 against
the oracle's loop.  Every oracle result is computed once and shared.
"""
import functools

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from cesm_emulator_amd import checkpoint as CK
from cesm_emulator_amd import input_grads, saliency_wrt_cond
from cesm_emulator_amd import kernels as K
from cesm_emulator_amd.ema import EMA
from cesm_emulator_amd.model import UNet, Diffusion
from cesm_emulator_amd.train import make_optimizer, train_step
from oracle import ref_cpu as R

pytestmark = pytest.mark.gpu

MULTS = (1, 2, 4)
B, H, W = 2, 16, 24
T_SAMPLE = 8
CASES = [(1, 3), (2, 3)]
ids = lambda c: "V%d_Cc%d" % c  # noqa: E731


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return (torch.linalg.vector_norm(a - b) / torch.linalg.vector_norm(b).clamp_min(1e-30)).item()


@functools.lru_cache(maxsize=None)
def ref_net(V, Cc):
    torch.manual_seed(1)
    ref = R.UNet(out_channels=V, ch_mults=MULTS)
    ref.net.input_conv = nn.Conv3d(V + Cc, 64, (1, 7, 7), padding=(0, 3, 3))
    return ref


def make_prod(case, dev, cdt):
    V, Cc = case
    prod = UNet(out_channels=V, ch_mults=MULTS, cond_channels=Cc)
    prod.load_state_dict(ref_net(V, Cc).state_dict(), strict=True)
    prod = prod.to(dev)
    prod.compute_dtype = cdt
    return prod


@functools.lru_cache(maxsize=None)
def inputs(case, Fr, seed=0):
    V, Cc = case
    g = torch.Generator().manual_seed(seed + 100 * V + 10 * Cc + Fr)
    x0 = torch.randn(B, V, H, W, generator=g)
    cond = torch.randn(B, Cc, Fr, H, W, generator=g)
    t = torch.randint(0, 1000, (B,), generator=g)
    noise = torch.randn(B, V, H, W, generator=g)
    return x0, cond, t, noise


@functools.lru_cache(maxsize=None)
def oracle_forward(case, Fr):
    x0, cond, t, _ = inputs(case, Fr)
    with torch.no_grad():
        return ref_net(*case)(x0, cond, t)


@functools.lru_cache(maxsize=None)
def oracle_loss_grads(case):
    """the oracle's Diffusion.loss at F = 3 with x_t and cond as leaves: loss, d/d x_t, d/d cond, parameter gradients"""
    ref = ref_net(*case)
    x0, cond, t, noise = inputs(case, 3)
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
@pytest.mark.parametrize("case", CASES, ids=ids)
def test_forward_parity_fp32(dev, case, Fr):
    prod = make_prod(case, dev, torch.float32)
    x0, cond, t, _ = inputs(case, Fr)
    with torch.no_grad():
        y = prod(x0.to(dev), cond.to(dev), t.to(dev))
    assert y.shape == (B, case[0], H, W)
    err = rel(y, oracle_forward(case, Fr))
    print(f"fwd rel err fp32 {ids(case)} F={Fr}: {err:.3e}")
    assert err < 1e-5
    if Fr == 1:   # cond [B, Cc, H, W] is the F = 1 window
        with torch.no_grad():
            assert torch.equal(prod(x0.to(dev), cond[:, :, 0].to(dev), t.to(dev)), y)


@pytest.mark.parametrize("case", CASES, ids=ids)
def test_loss_and_gradients_fp32(dev, case):
    prod = make_prod(case, dev, torch.float32)
    d = Diffusion(prod).to(dev)
    x0, cond, t, noise = inputs(case, 3)
    l_ref, _, _, pg = oracle_loss_grads(case)
    lp = d.loss(x0.to(dev), cond.to(dev), t=t.to(dev), noise=noise.to(dev))
    lp.backward()
    print(f"{ids(case)}: loss {lp.item():.6f} vs {l_ref:.6f}")
    assert abs(lp.item() - l_ref) / abs(l_ref) < 1e-5
    worst = 0.0
    pr = dict(prod.named_parameters())
    assert set(pg) == {n for n, p in pr.items() if p.requires_grad}
    for name, g in pg.items():
        assert pr[name].grad is not None, name
        e = rel(pr[name].grad, g)
        worst = max(worst, e)
        assert e < 1e-4, (name, e)
    print(f"{ids(case)}: worst parameter gradient rel err {worst:.3e}")


@pytest.mark.parametrize("case", CASES, ids=ids)
def test_input_grads_fp32(dev, case):
    prod = make_prod(case, dev, torch.float32)
    d = Diffusion(prod).to(dev)
    x0, cond, t, noise = inputs(case, 3)
    l_ref, gx, gc, _ = oracle_loss_grads(case)
    loss, dxt, dcond = input_grads(d, x0.to(dev), cond.to(dev), t=t.to(dev), noise=noise.to(dev))
    assert dxt.shape == x0.shape and dcond.shape == cond.shape   # dcond has Cc channels
    ex, ec = rel(dxt, gx), rel(dcond, gc)
    print(f"input_grads {ids(case)}: loss rel {abs(loss.item() - l_ref) / abs(l_ref):.3e}, dx_t rel {ex:.3e}, "
          f"dcond rel {ec:.3e}")
    assert abs(loss.item() - l_ref) / abs(l_ref) < 1e-5
    assert ex < 1e-4 and ec < 1e-4
    assert all(p.grad is None for p in prod.parameters())
    s = saliency_wrt_cond(d, x0.to(dev), cond.to(dev), t=t.to(dev), noise=noise.to(dev), normalize=False)
    assert s.shape == cond.shape and torch.equal(s, dcond.abs())


@pytest.mark.parametrize("case", CASES, ids=ids)
def test_bf16_forward_and_repeatable_train_steps(dev, case):
    x0, cond, t, noise = inputs(case, 3)
    args = [a.to(dev) for a in (x0, cond)]
    prod = make_prod(case, dev, torch.bfloat16)
    with torch.no_grad():
        y = prod(args[0], args[1], t.to(dev))
    err = rel(y, oracle_forward(case, 3))
    print(f"fwd rel err bf16 {ids(case)}: {err:.3e}")
    assert err < 5e-2
    params = []
    for _ in range(2):   # identical state, two identical steps
        d = Diffusion(make_prod(case, dev, torch.bfloat16)).to(dev)
        opt = make_optimizer(d, {})
        for _ in range(2):
            loss = train_step(d, opt, args[0], args[1], 1.0, t=t.to(dev), noise=noise.to(dev))
        torch.cuda.synchronize()
        assert torch.isfinite(loss)
        params.append((loss.clone(), {n: p.detach().clone() for n, p in d.model.named_parameters()}))
    assert torch.equal(params[0][0], params[1][0])
    bad = [n for n, p in params[0][1].items() if not torch.equal(p, params[1][1][n])]
    assert not bad, bad[:5]
    ref_p = dict(ref_net(*case).named_parameters())
    moved = [n for n, p in params[0][1].items() if not torch.equal(p.cpu(), ref_p[n])]
    assert "net.input_conv.weight" in moved and "net.out_conv.1.weight" in moved   # the step reached both ends


@functools.lru_cache(maxsize=None)
def sampler_case(case):
    V, Cc = case
    g = torch.Generator().manual_seed(11 + Cc)
    shape = (B, V, H, W)
    cond = torch.randn(B, Cc, H, W, generator=g)
    x_T = torch.randn(shape, generator=g)
    noise_seq = torch.randn(T_SAMPLE, *shape, generator=g)
    y_ref = R.Diffusion(ref_net(*case), timesteps=T_SAMPLE).sample(cond, shape, "cpu", x_T=x_T, noise_seq=noise_seq)
    return shape, cond, x_T, noise_seq, y_ref


@pytest.mark.parametrize("case", CASES, ids=ids)
def test_sampler_graph_eager_oracle(dev, case):
    shape, cond, x_T, noise_seq, y_ref = sampler_case(case)
    d = Diffusion(make_prod(case, dev, torch.float32), timesteps=T_SAMPLE).to(dev)
    c, xT, ns = cond.to(dev), x_T.to(dev), noise_seq.to(dev)
    y_eager = d.sample(c, shape, dev, use_graph=False, x_T=xT, noise_seq=ns)
    y_graph = d.sample(c, shape, dev, use_graph=True, x_T=xT, noise_seq=ns)
    assert y_graph.shape == shape
    assert torch.equal(y_eager, y_graph)
    err = rel(y_graph, y_ref)
    print(f"sample {ids(case)} T={T_SAMPLE} vs the oracle loop: rel {err:.3e}")
    assert err < 1e-4
    z_eager = d.sample(c, shape, dev, use_graph=False, x_T=xT, steps=4, ddim_eta=0.0)
    z_graph = d.sample(c, shape, dev, use_graph=True, x_T=xT, steps=4, ddim_eta=0.0)
    assert torch.isfinite(z_graph).all() and torch.equal(z_eager, z_graph)
    # guided: 2 B rows, the null condition is all Cc maps zero
    g_eager = d.sample(c, shape, dev, use_graph=False, x_T=xT, steps=4, guidance_scale=2.0)
    g_graph = d.sample(c, shape, dev, use_graph=True, x_T=xT, steps=4, guidance_scale=2.0)
    assert torch.isfinite(g_graph).all() and torch.equal(g_eager, g_graph)
    assert not torch.equal(g_graph, z_graph)


def test_p_uncond_one_is_the_null_condition(dev):
    case = (1, 3)
    x0, cond, t, noise = (a.to(dev) for a in inputs(case, 3))
    d = Diffusion(make_prod(case, dev, torch.float32), p_uncond=1.0).to(dev)
    d.train()
    a = d.loss(x0, cond, t=t, noise=noise).detach()
    d0 = Diffusion(d.model).to(dev)
    b = d0.loss(x0, torch.zeros_like(cond), t=t, noise=noise).detach()
    assert torch.isfinite(a) and torch.equal(a, b)


def test_sample_ensemble_and_counterfactual_shapes(dev):
    from cesm_emulator_amd.saliency import counterfactual_delta
    case = (2, 3)
    shape, cond, x_T, _, _ = sampler_case(case)
    d = Diffusion(make_prod(case, dev, torch.float32), timesteps=T_SAMPLE).to(dev)
    ens = d.sample_ensemble(cond.to(dev), 3, steps=2)
    assert ens.shape == (B, 3, 2, H, W) and torch.isfinite(ens).all()
    delta = counterfactual_delta(d, cond.to(dev), steps=2, paired=True)
    assert delta.shape == shape and torch.isfinite(delta).all()


def test_checkpoint_round_trip_samples_alike(dev, tmp_path):
    case = (1, 3)
    shape, cond, x_T, _, _ = sampler_case(case)
    cfg = {"unet": {"out_channels": 1, "base_ch": 64, "ch_mults": list(MULTS), "groups": 8, "cond_channels": 3},
           "train": {"timesteps": T_SAMPLE, "beta_schedule": "linear"}}
    d = Diffusion(make_prod(case, dev, torch.float32), timesteps=T_SAMPLE).to(dev)
    path = tmp_path / "mc.pt"
    CK.save_checkpoint(path, d, None, 1, cfg)
    d2, _ = CK.load_diffusion_from_checkpoint(path, device=dev)
    assert d2.model.net.n_cond == 3
    d2.model.compute_dtype = torch.float32
    a = d.sample(cond.to(dev), shape, dev, x_T=x_T.to(dev), steps=4)
    b = d2.sample(cond.to(dev), shape, dev, x_T=x_T.to(dev), steps=4)
    assert torch.equal(a, b)


def test_ema_attaches_and_samples(dev):
    case = (1, 3)
    x0, cond, t, noise = (a.to(dev) for a in inputs(case, 3))
    shape, c1, x_T, _, _ = sampler_case(case)
    d = Diffusion(make_prod(case, dev, torch.bfloat16), timesteps=T_SAMPLE).to(dev)
    opt = make_optimizer(d, {})
    ema = EMA(d.model, opt, beta=0.5)
    assert ema.ema_model.net.n_cond == 3
    train_step(d, opt, x0, cond, 1.0, t=t % T_SAMPLE, noise=noise)
    with ema.applied(d):
        y = d.sample(c1.to(dev), shape, dev, x_T=x_T.to(dev), steps=2)
    assert y.shape == shape and torch.isfinite(y).all()


def test_default_model_never_takes_the_new_entries(dev, monkeypatch):
    """cond_channels=None and cond_channels=V run the stem as it always was: with the four new wrappers failing,
    forward and gradients are bit-equal from the same weights"""
    for name in ("stem_fwd_mc", "stem_wgrad_mc", "stem_dgrad_mc", "window_gather_mc"):
        monkeypatch.setattr(K, name, lambda *a, _n=name, **k: pytest.fail(f"the default model called kernels.{_n}"))
    torch.manual_seed(1)
    sd = R.UNet(out_channels=2, ch_mults=MULTS).state_dict()
    g = torch.Generator().manual_seed(5)
    x0, cond = torch.randn(B, 2, H, W, generator=g).to(dev), torch.randn(B, 2, 3, H, W, generator=g).to(dev)
    t, noise = torch.randint(0, 1000, (B,), generator=g).to(dev), torch.randn(B, 2, H, W, generator=g).to(dev)
    res = []
    for kw in ({}, {"cond_channels": 2}):
        m = UNet(out_channels=2, ch_mults=MULTS, **kw)
        m.load_state_dict(sd, strict=True)
        m = m.to(dev)
        d = Diffusion(m).to(dev)
        with torch.no_grad():
            y = m(x0, cond, t)
        c = cond.clone().requires_grad_(True)
        d.loss(x0, c, t=t, noise=noise).backward()
        res.append((y, c.grad.clone(), {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None}))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    assert "net.input_conv.weight" in res[0][2] and set(res[0][2]) == set(res[1][2])
    for n, gr in res[0][2].items():
        assert torch.equal(gr, res[1][2][n]), n


def test_channel_mismatch_raises(dev):
    prod = make_prod((1, 3), dev, torch.float32)
    x0, cond, t, _ = inputs((1, 3), 3)
    with pytest.raises(ValueError, match="x_t has 1 channels and cond 1; they need 1 and 3"):
        prod(x0.to(dev), cond[:, :1].to(dev), t.to(dev))
