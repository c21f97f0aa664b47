"""Host side of the ensemble verification (no GPU): the float64 reference the GPU tests judge the kernel by
(`ref64`, written from the contract in include/cesm_hip.h), known answers, the accumulator arithmetic of
ensemble.summarize / EnsembleVerifier.result, the argument errors that must come before any launch, and the C ABI.

Contract per pixel (M members x_m, observation y):
  s = sum x_m, mean = s / M;  q = sum (x_m - mean)^2, var = q / (M - 1);  A = sum |x_m - y|,  P = sum_{i<j} |x_i - x_j|,
  crps = A / M - P / (M (M - 1));  rank = #{m : x_m < y}.
Accumulator row v: sums over b, h, w of w_r {1, (mean - y)^2, var, crps, [rank = r] for r = 0 .. M}, w_r = w[row0[b] + h]."""
import ctypes
import math

import pytest
import torch

from cesm_emulator_amd import ensemble as E
from cesm_emulator_amd import kernels as K
from cesm_emulator_amd import _lib
from cesm_emulator_amd.model import Diffusion, check_row0


def pairwise_abs(x):
    """P = sum_{i<j} |x_i - x_j| over dim 1 of a float64 [B, M, ...], pair by pair"""
    P = torch.zeros_like(x[:, 0])
    for i in range(1, x.shape[1]):
        P += (x[:, i:i + 1] - x[:, :i]).abs().sum(dim=1)
    return P


def sorted_abs(x):
    """the same sum from the order statistics: sum_k (2k - M + 1) x_(k)"""
    M = x.shape[1]
    xs = x.sort(dim=1).values
    k = torch.arange(M, dtype=torch.float64).view(1, M, *([1] * (x.ndim - 2)))
    return ((2 * k - M + 1) * xs).sum(dim=1)


def ref64(ens, obs=None, w=None, row0=None):
    """float64 CPU reference of cesm_ens_stats: dict of s, q, mean, var and, with obs, A, P, crps, rank (int64), each
    [B, V, H, W]; with w also acc [V, 4 + M + 1] (entries the kernel leaves alone without obs are NaN here)"""
    x = ens.detach().cpu().double()
    B, M, V, H, W = x.shape
    s = x.sum(dim=1)
    mean = s / M
    q = ((x - mean[:, None]) ** 2).sum(dim=1)
    out = {"s": s, "q": q, "mean": mean, "var": q / (M - 1)}
    if obs is not None:
        y = obs.detach().cpu().double()
        out["A"] = (x - y[:, None]).abs().sum(dim=1)
        out["P"] = pairwise_abs(x)
        out["crps"] = out["A"] / M - out["P"] / (M * (M - 1))
        out["rank"] = (x < y[:, None]).sum(dim=1)
    if w is not None:
        wd = w.detach().cpu().double()
        r0 = [0] * B if row0 is None else [int(v) for v in row0]
        wr = torch.stack([wd[r:r + H] for r in r0]).view(B, 1, H, 1).expand(B, V, H, W)
        assert wr.shape[2] == H, "row window leaves the grid"
        acc = torch.full((V, 4 + M + 1), float("nan"), dtype=torch.float64)
        acc[:, 0] = wr.sum(dim=(0, 2, 3))
        acc[:, 2] = (wr * out["var"]).sum(dim=(0, 2, 3))
        if obs is not None:
            acc[:, 1] = (wr * (mean - y) ** 2).sum(dim=(0, 2, 3))
            acc[:, 3] = (wr * out["crps"]).sum(dim=(0, 2, 3))
            for r in range(M + 1):
                acc[:, 4 + r] = (wr * (out["rank"] == r)).sum(dim=(0, 2, 3))
        out["acc"] = acc
    return out


# ------------------------------------------------------------------------------------------ the reference itself
@pytest.mark.parametrize("M", [2, 3, 8, 40, 128])
def test_pairwise_sum_equals_the_sorted_form(M):
    g = torch.Generator().manual_seed(M)
    x = torch.randn(3, M, 2, 4, 5, generator=g, dtype=torch.float64)
    a, b = pairwise_abs(x), sorted_abs(x)
    assert float(((a - b).abs() / a).max()) <= 1e-12
    # and both are the plain double sum over all ordered pairs, halved
    c = (x[:, :, None] - x[:, None, :]).abs().sum(dim=(1, 2)) / 2
    assert float(((a - c).abs() / a).max()) <= 1e-12


def _one(xs, y):
    ens = torch.tensor(xs, dtype=torch.float32).view(1, len(xs), 1, 1, 1)
    obs = torch.tensor([y], dtype=torch.float32).view(1, 1, 1, 1)
    r = ref64(ens, obs, torch.ones(1))
    return {k: float(v.reshape(-1)[0]) for k, v in r.items() if k != "acc"}, r["acc"]


def test_known_answers():
    r, acc = _one([0.0, 2.0], 1.0)
    assert r["crps"] == 0.0 and r["var"] == 2.0 and r["rank"] == 1 and r["mean"] == 1.0
    assert acc[0].tolist() == [1.0, 0.0, 2.0, 0.0, 0.0, 1.0, 0.0]
    r, _ = _one([0.0, 0.0], 3.0)
    assert r["crps"] == 3.0 and r["rank"] == 2 and r["var"] == 0.0
    # y equal to a member: that member does not count towards the rank (ties are not-less)
    r, _ = _one([1.0, 2.0, 3.0], 2.0)
    assert r["rank"] == 1
    r, _ = _one([2.0, 2.0, 2.0], 2.0)
    assert r["rank"] == 0 and r["crps"] == 0.0
    # a three-member case by hand: A = 1 + 0 + 3 = 4, P = 1 + 4 + 3 = 8, crps = 4/3 - 8/6 = 0
    r, _ = _one([0.0, 1.0, 4.0], 1.0)
    assert r["A"] == 4.0 and r["P"] == 8.0 and abs(r["crps"]) <= 1e-15 and r["rank"] == 1


def test_reference_accumulator_uses_the_crop_rows():
    g = torch.Generator().manual_seed(1)
    ens = torch.randn(2, 3, 1, 2, 3, generator=g)
    obs = torch.randn(2, 1, 2, 3, generator=g)
    w = torch.tensor([1.0, 2.0, 4.0, 8.0])
    r = ref64(ens, obs, w, [0, 2])
    assert float(r["acc"][0, 0]) == 3 * (1 + 2) + 3 * (4 + 8)
    assert abs(float(r["acc"][0, 4:].sum()) - float(r["acc"][0, 0])) <= 1e-12
    assert torch.isnan(ref64(ens, None, w)["acc"][0, [1, 3, 4, 5, 6, 7]]).all()


# ------------------------------------------------------------------------------------------ accumulator arithmetic
def test_summarize_and_verifier_result_on_a_hand_made_accumulator():
    M = 3
    acc = torch.tensor([[4.0, 8.0, 2.0, 1.0, 1.0, 0.5, 2.0, 0.5],
                        [2.0, 0.5, 0.5, 3.0, 0.0, 0.0, 0.0, 2.0]], dtype=torch.float64)
    r = E.summarize(acc, M)
    def close(got, want):  # torch's sqrt and math.sqrt may differ in the last bit
        return all(abs(a - b) <= 4e-16 * abs(b) for a, b in zip(got.tolist(), want))

    assert r["mse"].tolist() == [2.0, 0.25] and close(r["rmse"], [math.sqrt(2.0), 0.5])
    assert r["var"].tolist() == [0.5, 0.25] and close(r["spread"], [math.sqrt(0.5), 0.5])
    assert r["crps"].tolist() == [0.25, 1.5]
    want_ssr = [math.sqrt(4.0 / 3.0 * 0.5 / 2.0), math.sqrt(4.0 / 3.0 * 0.25 / 0.25)]
    assert close(r["ssr"], want_ssr)
    assert r["rank_hist"].tolist() == [[0.25, 0.125, 0.5, 0.125], [0.0, 0.0, 0.0, 1.0]]
    assert r["rank_hist"].sum(dim=1).tolist() == [1.0, 1.0]
    no = E.summarize(acc, M, has_obs=False)
    assert no["var"].tolist() == [0.5, 0.25] and no["mse"] is None and no["rank_hist"] is None and no["crps"] is None
    with pytest.raises(ValueError, match="acc"):
        E.summarize(acc, 4)

    v = E.EnsembleVerifier(M, 2, device="cpu")
    assert tuple(v.acc.shape) == (2, 8) and v.acc.dtype == torch.float64 and float(v.acc.abs().sum()) == 0.0
    v.acc.copy_(acc)
    got = v.result()
    assert all(torch.equal(got[k], r[k]) for k in E.SCALARS)
    v.reset()
    assert float(v.acc.abs().sum()) == 0.0
    for bad in (1, 129):
        with pytest.raises(ValueError, match="members"):
            E.EnsembleVerifier(bad, 1, device="cpu")


# ------------------------------------------------------------------------------------------ errors before a launch
@pytest.fixture
def launches(monkeypatch):
    calls = []
    monkeypatch.setattr(K, "call", lambda name, *args: calls.append(name))
    return calls


def test_argument_errors_come_before_any_launch(launches):
    w = torch.ones(4)
    obs = torch.zeros(2, 1, 4, 8)
    with pytest.raises(ValueError, match="at least 2"):
        K.ens_stats(torch.zeros(2, 1, 1, 4, 8), obs, w)
    with pytest.raises(NotImplementedError, match="128"):
        K.ens_stats(torch.zeros(2, 129, 1, 4, 8), obs, w)
    ens = torch.zeros(2, 3, 1, 4, 8)
    with pytest.raises(ValueError, match="need obs"):
        K.ens_stats(ens, None, w, crps=True)
    with pytest.raises(ValueError, match="need obs"):
        K.ens_stats(ens, None, w, rank=True)
    with pytest.raises(ValueError, match="no output"):
        K.ens_stats(ens, None, w, mean=False, var=False, acc=False)
    with pytest.raises(RuntimeError, match="shape"):
        K.ens_stats(ens[0], obs, w)
    with pytest.raises(RuntimeError, match="shape"):
        K.ens_stats(ens, obs[:, :, :2], w)
    with pytest.raises(RuntimeError, match="shape"):
        K.ens_stats(ens, obs, w[:3])
    with pytest.raises(RuntimeError, match="shape"):
        K.ens_stats(ens, obs, w, torch.zeros(3, dtype=torch.int64))
    with pytest.raises(RuntimeError, match="shape"):
        K.ens_stats(ens, obs, w, acc=torch.zeros(1, 9, dtype=torch.float64))
    # CPU tensors are refused like every other wrapper
    with pytest.raises(RuntimeError, match="device tensors"):
        K.ens_stats(ens, obs, w)
    with pytest.raises(RuntimeError, match="device tensors"):
        E.ensemble_stats(ens, obs)
    with pytest.raises(RuntimeError, match="device tensors"):
        E.EnsembleVerifier(3, 1, device="cpu").update(ens, obs)
    # a list / CPU row0 is range-checked (Hg = H = 4 without lat: only 0 fits; with 6 latitudes 0 .. 2)
    with pytest.raises(ValueError, match="row0"):
        E.ensemble_stats(ens, obs, row0=[0, 1])
    with pytest.raises(ValueError, match="row0"):
        E.ensemble_stats(ens, obs, lat=torch.linspace(-50, 50, 6), row0=[0, 3])
    with pytest.raises(ValueError, match="row0"):
        E.ensemble_stats(ens, obs, lat=torch.linspace(-50, 50, 6), row0=torch.tensor([-1, 0]))
    with pytest.raises(ValueError, match="row0"):
        E.EnsembleVerifier(3, 1, lat=torch.linspace(-50, 50, 6), device="cpu").update(ens, obs, row0=[0, 1, 2])
    with pytest.raises(ValueError, match="rows"):
        E.ensemble_stats(ens, obs, lat=[0.0, 1.0])
    assert launches == []


def test_row0_check_is_the_diffusions():
    """Diffusion._row0 and ensemble_stats share check_row0: same tensors out, same errors"""
    d = Diffusion(torch.nn.Identity(), lat_weight=0.5, lat=torch.linspace(-90, 90, 12))
    assert d._row0(None, 2, 4, 12, "cpu") is None and check_row0(None, 2, 4, 12, "cpu") is None
    got = d._row0([0, 8], 2, 4, 12, "cpu")
    assert got.dtype == torch.int64 and got.tolist() == [0, 8]
    assert torch.equal(got, check_row0(torch.tensor([0, 8]), 2, 4, 12, "cpu"))
    for bad in ([9, 0], [0], [-1, 0]):
        with pytest.raises(ValueError, match="row0"):
            d._row0(bad, 2, 4, 12, "cpu")
        with pytest.raises(ValueError, match="row0"):
            check_row0(bad, 2, 4, 12, "cpu")
    with pytest.raises(ValueError, match="whole grid"):
        Diffusion(torch.nn.Identity(), lat_weight=0.5)._row0([1], 1, 4, 4, "cpu")


def test_sample_ensemble_argument_errors():
    d = Diffusion(torch.nn.Identity(), timesteps=4)
    cond = torch.zeros(2, 1, 4, 8)
    with pytest.raises(ValueError, match="members"):
        d.sample_ensemble(cond, 0)
    with pytest.raises(ValueError, match="member_batch"):
        d.sample_ensemble(cond, 2, member_batch=0)
    with pytest.raises(ValueError, match="x_T"):
        d.sample_ensemble(cond, 2, x_T=torch.zeros(4, 1, 4, 8))
    with pytest.raises(ValueError, match="noise_seq"):
        d.sample_ensemble(cond, 2, noise_seq=torch.zeros(4, 4, 1, 4, 8))
    with pytest.raises(ValueError, match="cond"):
        d.sample_ensemble(cond[0], 2)
    with pytest.raises(ValueError, match="steps"):
        d.sample_ensemble(cond, 2, steps=9)


# ------------------------------------------------------------------------------------------ C ABI
def test_header_declares_the_entry_point_and_the_library_exports_it():
    decls = _lib.parse_header()
    assert "cesm_ens_stats" in decls
    res, args = decls["cesm_ens_stats"]
    assert res is ctypes.c_int and len(args) == 18
    assert args[:10] == [ctypes.c_void_p] * 10 and args[10:17] == [ctypes.c_int] * 7 and args[17] is ctypes.c_void_p
    from cesm_emulator_amd.build import build
    build()
    assert hasattr(ctypes.CDLL(str(_lib.LIBPATH)), "cesm_ens_stats")
