"""Few-step DDIM sampling, host side (no GPU): the strided time grid Diffusion.sample_schedule and the float64
step coefficients Diffusion.ddim_coefs (the definition the update kernel and the GPU tests refer to).

* schedule: strictly increasing, ends at T-1, starts at 0 (steps >= 2), exhaustively for T < 40;
* eta = 1 on the full grid is the DDPM step: the coefficients equal the ancestral step's within 5e-6 (2x the
  worst case 2.35e-6, on b at T = 1000, which comes from the fp32 rounding of alphas_cumprod both sides share);
* eta = 0 maps q_sample(x0, t, eps) onto q_sample(x0, t_prev, eps) (and onto x0 for t_prev = -1) to float64 rounding;
* bad arguments raise ValueError.
"""
import pytest
import torch

from cesm_emulator_amd.model import Diffusion


def diffusion(T):
    return Diffusion(torch.nn.Identity(), timesteps=T)


def test_schedule_properties_exhaustive():
    for T in range(1, 40):
        d = diffusion(T)
        for steps in range(1, T + 1):
            tau = d.sample_schedule(steps)
            assert len(tau) == steps and all(type(v) is int for v in tau), (T, steps)
            assert all(b > a for a, b in zip(tau, tau[1:])), (T, steps, tau)
            assert tau[-1] == T - 1, (T, steps, tau)
            assert 0 <= tau[0], (T, steps, tau)
            if steps >= 2:
                assert tau[0] == 0, (T, steps, tau)
        assert d.sample_schedule(T) == list(range(T))
        assert d.sample_schedule(1) == [T - 1]


def test_schedule_literals_and_errors():
    tau = diffusion(1000).sample_schedule(50)
    assert len(tau) == 50
    assert tau[:4] == [0, 20, 41, 61] and tau[-3:] == [958, 979, 999]
    assert diffusion(12).sample_schedule(5) == [0, 3, 6, 8, 11]
    assert diffusion(1000).sample_schedule(1000) == list(range(1000))
    for T in (12, 1000):
        for steps in (0, T + 1):
            with pytest.raises(ValueError):
                diffusion(T).sample_schedule(steps)


@pytest.mark.parametrize("T", [12, 1000])
def test_coefs_eta1_full_grid_is_ddpm(T):
    d = diffusion(T)
    t = torch.arange(T)
    a, b, s = d.ddim_coefs(t, t - 1, 1.0)
    assert a.dtype == b.dtype == s.dtype == torch.float64 and a.shape == t.shape
    ra = d.sqrt_recip_alphas.double()
    rb = -ra * d.betas.double() / d.sqrt_one_minus_alphas_cumprod.double()
    rs = torch.sqrt(d.posterior_variance.double())
    errs = [(x - y).abs().max().item() for x, y in ((a, ra), (b, rb), (s, rs))]
    print(f"T={T}: max |a|, |b|, |sigma| difference to the DDPM step {errs}")
    assert max(errs) <= 5e-6
    # ints give the same numbers as tensors
    a1, b1, s1 = d.ddim_coefs(T - 1, T - 2 if T > 1 else -1, 1.0)
    assert (a1.item(), b1.item(), s1.item()) == (a[-1].item(), b[-1].item(), s[-1].item())


def test_eta0_is_consistent_with_q_sample():
    d = diffusion(1000)
    g = torch.Generator().manual_seed(5)
    t = torch.tensor([999, 999, 500, 500, 20, 1, 1, 0, 7])
    tp = torch.tensor([979, -1, 0, 499, -1, 0, -1, -1, 3])
    x0 = torch.randn(len(t), 64, generator=g, dtype=torch.float64)
    eps = torch.randn(len(t), 64, generator=g, dtype=torch.float64)
    ac = d.alphas_cumprod.double()
    at = ac[t][:, None]
    ap = torch.where(tp < 0, torch.ones_like(at[:, 0]), ac[tp.clamp_min(0)])[:, None]
    x_t = at.sqrt() * x0 + (1 - at).sqrt() * eps
    a, b, s = d.ddim_coefs(t, tp, 0.0)
    assert (s == 0).all()
    got = a[:, None] * x_t + b[:, None] * eps
    want = ap.sqrt() * x0 + (1 - ap).sqrt() * eps
    scale = torch.linalg.vector_norm(want, dim=1)
    err = (torch.linalg.vector_norm(got - want, dim=1) / scale).max().item()
    print("eta = 0 consistency, worst relative L2", err)
    assert err <= 1e-12
    last = tp < 0
    err0 = (torch.linalg.vector_norm(got[last] - x0[last], dim=1) / torch.linalg.vector_norm(x0[last], dim=1)).max()
    assert err0.item() <= 1e-12


def test_bad_arguments_raise():
    d = diffusion(12)
    for t, tp in ((5, 5), (5, 6), (0, 0), (12, 3), (3, -2), (-1, -1)):
        with pytest.raises(ValueError):
            d.ddim_coefs(t, tp, 0.0)
    with pytest.raises(ValueError):
        d.ddim_coefs(torch.tensor([5, 4]), torch.tensor([3, 4]), 0.5)
    with pytest.raises(ValueError):
        d.ddim_coefs(5, 3, -0.1)
    with pytest.raises(ValueError):
        d.ddim_coefs(5, 3, float("nan"))
