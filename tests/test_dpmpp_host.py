"""DPM-Solver++(2M) sampling, host side (no GPU): the log-SNR time grid Diffusion.sample_schedule(steps, "logsnr") and
the float64 step coefficients Diffusion.dpmpp_coefs (the definition the update kernel and the GPU tests refer to).

* schedule: pinned lists, and for T in {1, 2, 3, 12, 1000} and every steps up to min(T, 60) strictly increasing, of
  length steps, ending at T-1 and starting at 0 (steps >= 2); bad arguments raise ValueError;
* coefficients against an independent float64 restatement of the textbook update (x0 first, then the extrapolated
  D = w_c x0 + w_p x0_last, then x_prev = (sigma_prev / sigma_t) x - alpha_prev expm1(-h) D) to 1e-12 relative;
  without history (a, b) are ddim_coefs(t, t_prev, 0)'s to 1e-10 relative;
* convergence on an analytic per-pixel Gaussian score in float64, against 1000 DDIM steps on the uniform grid:
  err(2M, logsnr, N) < err(DDIM, uniform, N) / 3 for N in {10, 20, 40} (measured ratios 5.4, 6.0, 8.4: the factor 3
  leaves about 2x margin) and err(2M, logsnr, N) strictly decreasing over N = 5, 10, 20, 40.  The test prints the
  table of all four solver x spacing combinations (DESIGN.md "Sampler (F1)" quotes it).
"""
import math

import numpy as np
import pytest
import torch

from cesm_emulator_amd.model import Diffusion


def diffusion(T):
    return Diffusion(torch.nn.Identity(), timesteps=T)


def test_logsnr_schedule_pinned():
    d = diffusion(1000)
    assert d.sample_schedule(10, "logsnr") == [0, 5, 22, 73, 202, 410, 603, 757, 886, 999]
    d = diffusion(12)
    assert d.sample_schedule(4, "logsnr") == [0, 1, 3, 11]
    assert d.sample_schedule(5, "logsnr") == [0, 1, 2, 4, 11]
    assert d.sample_schedule(12, "logsnr") == list(range(12))


@pytest.mark.parametrize("T", [1, 2, 3, 12, 1000])
def test_logsnr_schedule_properties(T):
    d = diffusion(T)
    for steps in range(1, min(T, 60) + 1):
        tau = d.sample_schedule(steps, "logsnr")
        assert len(tau) == steps and all(type(v) is int for v in tau), (T, steps)
        assert all(b > a for a, b in zip(tau, tau[1:])), (T, steps, tau)
        assert tau[-1] == T - 1, (T, steps, tau)
        if steps >= 2:
            assert tau[0] == 0, (T, steps, tau)
    assert d.sample_schedule(1, "logsnr") == [T - 1]
    assert d.sample_schedule(T, "logsnr") == list(range(T))


def test_schedule_errors_and_uniform_unchanged():
    for T in (1, 12, 1000):
        d = diffusion(T)
        for spacing in ("uniform", "logsnr"):
            for steps in (0, T + 1):
                with pytest.raises(ValueError):
                    d.sample_schedule(steps, spacing)
        with pytest.raises(ValueError):
            d.sample_schedule(1, "cosine")
        for steps in range(1, min(T, 60) + 1):
            assert d.sample_schedule(steps, "uniform") == d.sample_schedule(steps)
            assert d.sample_schedule(steps, spacing="uniform") == d.sample_schedule(steps)


def textbook(d, x, eps, x0_last, t, t_prev, t_last):
    """DPM-Solver++(2M) (Lu et al. 2022, algorithm 2) in float64, written from the paper and not from dpmpp_coefs"""
    ac = d.alphas_cumprod.double()

    def asl(u):
        a, s = math.sqrt(ac[u].item()), math.sqrt(1.0 - ac[u].item())
        return a, s, math.log(a / s)

    a_t, s_t, l_t = asl(t)
    x0 = (x - s_t * eps) / a_t
    if t_prev < 0:
        return x0, x0
    a_p, s_p, l_p = asl(t_prev)
    h = l_p - l_t
    D = x0
    if t_last >= 0:
        r = (l_t - asl(t_last)[2]) / h
        D = (1.0 + 1.0 / (2.0 * r)) * x0 - (1.0 / (2.0 * r)) * x0_last
    return (s_p / s_t) * x - a_p * math.expm1(-h) * D, x0


TRIPLES = [(999, 979, -1), (500, 0, 757), (1, -1, 5), (1, 0, 2), (998, 997, 999), (0, -1, -1), (0, -1, 1),
           (410, 202, 603), (999, 0, -1), (5, 0, 22)]


@pytest.mark.parametrize("T", [1000, 12])
def test_coefs_match_textbook_update(T):
    d = diffusion(T)
    g = torch.Generator().manual_seed(0)
    x, eps, x0_last = (torch.randn(257, dtype=torch.float64, generator=g) for _ in range(3))
    triples = TRIPLES if T == 1000 else [(11, 4, -1), (4, 2, 11), (2, 1, 4), (1, 0, 2), (0, -1, 1), (11, 10, -1)]
    for t, tp, tl in triples:
        a, b, c, c1, c2 = d.dpmpp_coefs(t, tp, tl)
        assert all(v.dtype == torch.float64 for v in (a, b, c, c1, c2))
        want, want0 = textbook(d, x, eps, x0_last, t, tp, tl)
        got, got0 = a * x + b * eps + c * x0_last, c1 * x + c2 * eps
        scale = (a * x).abs() + (b * eps).abs() + (c * x0_last).abs()
        assert ((got - want).abs() <= 1e-12 * scale).all(), (t, tp, tl)
        assert ((got0 - want0).abs() <= 1e-12 * ((c1 * x).abs() + (c2 * eps).abs())).all(), (t, tp, tl)
        if tl < 0 or tp < 0:
            assert c.item() == 0.0, (t, tp, tl)
    # tensors broadcast against each other and against ints, and give what the scalars give
    tt = torch.tensor([t for t, _, _ in triples])
    tp = torch.tensor([p for _, p, _ in triples])
    tl = torch.tensor([l for _, _, l in triples])
    batched = d.dpmpp_coefs(tt, tp, tl)
    for k, tr in enumerate(triples):
        for vb, vs in zip(batched, d.dpmpp_coefs(*tr)):
            assert vb[k].item() == vs.item(), tr
    assert d.dpmpp_coefs(tt.clamp_min(1), 0, -1)[0].shape == tt.shape


@pytest.mark.parametrize("T", [1000, 12])
def test_no_history_is_ddim_eta0(T):
    d = diffusion(T)
    pairs = [(t, tp) for t in (T - 1, T // 2, 1, 0) for tp in (t - 1, t // 2, 0, -1) if -1 <= tp < t]
    for t, tp in pairs:
        a, b, c, c1, c2 = d.dpmpp_coefs(t, tp, -1)
        da, db, _ = d.ddim_coefs(t, tp, 0.0)
        assert abs(a.item() - da.item()) <= 1e-10 * abs(da.item()), (t, tp)
        assert abs(b.item() - db.item()) <= 1e-10 * abs(db.item()), (t, tp)
        assert c.item() == 0.0
        if tp == -1:
            assert a.item() == c1.item() and b.item() == c2.item()
    # the last step ignores the history: same coefficients with and without one
    if T > 2:
        for u, v in zip(d.dpmpp_coefs(1, -1, 2), d.dpmpp_coefs(1, -1, -1)):
            assert u.item() == v.item()


def test_equal_logsnr_spacing_gives_half_weights():
    """r = 1 (the previous step spanned the same log-SNR interval): c = -G / 2, and a, b carry w_c = 3/2"""
    d = diffusion(1000)
    # build a table on which lambda is exactly linear in the index over three entries: ac = sigmoid(2 lambda)
    lam = torch.tensor([1.0, 0.5, 0.0], dtype=torch.float64)
    d.alphas_cumprod[:3] = torch.sigmoid(2 * lam).float()
    ac = d.alphas_cumprod[:3].double()
    lam = 0.5 * torch.log(ac / (1 - ac))
    t, tp, tl = 1, 0, 2
    h = (lam[tp] - lam[t]).item()
    r = ((lam[t] - lam[tl]) / h).item()
    assert abs(r - 1.0) < 1e-6  # the fp32 table bends the line a little: r is 1 to fp32 rounding
    G = -math.sqrt(ac[tp].item()) * math.expm1(-h)
    a, b, c, c1, c2 = d.dpmpp_coefs(t, tp, tl)
    assert abs(c.item() - (-G / (2 * r))) <= 1e-12 * abs(G)
    assert abs(c.item() + G / 2) <= 1e-6 * abs(G)


def test_coefs_range_checks():
    d = diffusion(12)
    bad = [(12, 3, -1), (-1, -1, -1), (5, 5, -1), (5, 6, -1), (5, -2, -1), (5, 3, 5), (5, 3, 4), (5, 3, 12), (5, 3, -2),
           (0, -1, 0)]
    for tr in bad:
        with pytest.raises(ValueError):
            d.dpmpp_coefs(*tr)
    with pytest.raises(ValueError):
        d.dpmpp_coefs(torch.tensor([5, 5]), torch.tensor([3, 5]), -1)
    with pytest.raises(ValueError):
        d.dpmpp_coefs(torch.tensor([5, 5]), 3, torch.tensor([-1, 5]))
    d.dpmpp_coefs(11, 10, -1), d.dpmpp_coefs(0, -1, 11), d.dpmpp_coefs(10, -1, 11)  # the edges are valid


# ---- convergence on an analytic score
def analytic_case(n=4096):
    """per-pixel Gaussian data x0 ~ N(mu, s^2): the exact eps-prediction is known in closed form"""
    rng = np.random.default_rng(0)
    mu = rng.normal(size=n) * 0.7
    s = 0.25 + rng.random(size=n)
    x_T = rng.normal(size=n)
    return mu, s, x_T


def run_sampler(d, mu, s, x_T, steps, solver, spacing):
    """the sampler's loop in float64, driven only by sample_schedule and dpmpp_coefs / ddim_coefs"""
    ac = d.alphas_cumprod.double().numpy()

    def eps_exact(x, t):
        return math.sqrt(1.0 - ac[t]) * (x - math.sqrt(ac[t]) * mu) / (ac[t] * s * s + 1.0 - ac[t])

    tau = d.sample_schedule(steps, spacing)
    x, x0_last, t_last = x_T.copy(), np.zeros_like(x_T), -1
    for t, tp in zip(reversed(tau), reversed([-1] + tau[:-1])):
        eps = eps_exact(x, t)
        if solver == "ddim":
            a, b, _ = (v.item() for v in d.ddim_coefs(t, tp, 0.0))
            x = a * x + b * eps
        else:
            a, b, c, c1, c2 = (v.item() for v in d.dpmpp_coefs(t, tp, t_last))
            x, x0_last, t_last = a * x + b * eps + c * x0_last, c1 * x + c2 * eps, t
    return x


COMBOS = [("ddim", "uniform"), ("ddim", "logsnr"), ("dpmpp2m", "uniform"), ("dpmpp2m", "logsnr")]


def convergence_table(Ns):
    d = diffusion(1000)
    mu, s, x_T = analytic_case()
    ref = run_sampler(d, mu, s, x_T, 1000, "ddim", "uniform")
    return {(N, *c): float(np.linalg.norm(run_sampler(d, mu, s, x_T, N, *c) - ref) / np.linalg.norm(ref))
            for N in Ns for c in COMBOS}


def test_convergence_on_analytic_score():
    Ns = (5, 10, 20, 40, 50)
    err = convergence_table(Ns)
    print("\nrelative L2 error against 1000 DDIM steps (uniform grid), analytic Gaussian score, float64")
    print("| N | DDIM, uniform t | DDIM, log-SNR grid | 2M, uniform t | 2M, log-SNR grid |")
    print("|---|---|---|---|---|")
    for N in Ns:
        print(f"| {N} | " + " | ".join(f"{err[(N, *c)]:.4f}" for c in COMBOS) + " |")
    for N in (10, 20, 40):
        ratio = err[(N, "ddim", "uniform")] / err[(N, "dpmpp2m", "logsnr")]
        print(f"N = {N}: err(DDIM, uniform) / err(2M, logsnr) = {ratio:.2f}")
        assert err[(N, "dpmpp2m", "logsnr")] < err[(N, "ddim", "uniform")] / 3, N
    seq = [err[(N, "dpmpp2m", "logsnr")] for N in (5, 10, 20, 40)]
    assert all(b < a for a, b in zip(seq, seq[1:])), seq
