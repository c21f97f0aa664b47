"""Host side of the weighted loss (no GPU): the latitude and min-SNR weight tables against their formulas restated
here in float64, the constructor's argument checks, the unchanged checkpoint keys, the `loss` block of the training
config, and the crop row offsets a loader hands to the loss."""
import math

import numpy as np
import pytest
import torch

from cesm_emulator_amd import data as DA
from cesm_emulator_amd.model import Diffusion, latitude_weights
from cesm_emulator_amd.train import make_diffusion


def _diff(**kw):
    return Diffusion(torch.nn.Identity(), **kw)


# ------------------------------------------------------------------------------------------ latitude weights
@pytest.mark.parametrize("Hg", [192, 5])
def test_latitude_weights_match_the_formula(Hg):
    """w = clamp_min(cos(deg2rad(lat)), 0) / (mean + 1e-8) over lat = linspace(-90, 90, Hg), restated with math.cos"""
    lat = [-90.0 + 180.0 * i / (Hg - 1) for i in range(Hg)]
    c = [max(math.cos(math.radians(x)), 0.0) for x in lat]
    want = np.asarray(c) / (sum(c) / Hg + 1e-8)
    d = _diff(lat_weight=1.0)
    for got in (d.lat_weights(Hg, "cpu"), _diff(lat_weight=1.0, lat=lat).lat_weights(7 if Hg > 7 else Hg, "cpu"),
                latitude_weights(torch.tensor(lat))):
        assert got.dtype == torch.float32 and tuple(got.shape) == (Hg,)
        assert np.abs(got.double().numpy() - want).max() <= 1e-6
        assert abs(float(got.double().mean()) - 1.0) <= 1e-6
        assert abs(float(got[0])) <= 1e-6 and abs(float(got[-1])) <= 1e-6
        assert float(got.min()) >= 0.0
    assert d.lat_weights(Hg, "cpu") is d.lat_weights(Hg, "cpu")  # cached per (Hg, device)


def test_latitudes_past_the_poles_clamp_to_zero_and_short_lat_raises():
    w = latitude_weights([-100.0, 0.0, 100.0])
    assert w[0] == 0.0 and w[2] == 0.0 and abs(float(w[1]) - 3.0) <= 1e-6
    with pytest.raises(ValueError, match="rows"):
        _diff(lat=[-45.0, 0.0, 45.0]).lat_weights(4, "cpu")


# ------------------------------------------------------------------------------------------ min-SNR table
def test_min_snr_table_matches_the_formula():
    gamma = 5.0
    d = _diff(min_snr_gamma=gamma)
    a = d.min_snr_weight
    assert a.dtype == torch.float32 and tuple(a.shape) == (d.T,)
    ac = d.alphas_cumprod.double()
    snr = ac / (1.0 - ac)
    want = torch.minimum(torch.ones_like(ac), gamma * (1.0 - ac) / ac)
    assert torch.equal(a, want.float())  # float64 from the fp32 entries, rounded once
    assert torch.allclose(want, torch.minimum(snr, torch.full_like(snr, gamma)) / snr, rtol=1e-12, atol=0.0)
    assert bool((a[snr <= gamma] == 1.0).all()) and bool((snr <= gamma).any()) and bool((snr > gamma).any())
    assert bool((a[1:] >= a[:-1]).all())
    assert float(a.min()) > 0.0 and float(a.max()) <= 1.0
    assert _diff().min_snr_weight is None


# ------------------------------------------------------------------------------------------ constructor
@pytest.mark.parametrize("kw", [{"lat_weight": -0.1}, {"lat_weight": 1.1}, {"min_snr_gamma": 0}, {"min_snr_gamma": -1},
                                {"min_snr_gamma": "5"}, {"min_snr_gamma": True}, {"lat_weight": float("nan")}])
def test_constructor_rejects(kw):
    with pytest.raises(ValueError):
        _diff(**kw)


def test_defaults_and_weighted_flag():
    assert not _diff().weighted and not _diff(lat=[0.0, 1.0]).weighted
    assert _diff(lat_weight=0.5).weighted and _diff(min_snr_gamma=5).weighted
    d = _diff(lat_weight=1, min_snr_gamma=2)
    assert d.lat_weight == 1.0 and d.min_snr_gamma == 2.0


def test_row0_checked_on_the_host():
    x0 = torch.zeros(2, 1, 4, 8)
    whole = _diff(lat_weight=0.5)
    with pytest.raises(ValueError, match="row0"):  # no lat: the batch is the whole grid
        whole.loss_components(x0, None, row0=[0, 1])
    crop = _diff(lat_weight=0.5, lat=np.linspace(-90, 90, 12))
    for bad in ([0, 9], [-1, 0], torch.tensor([8, 9]), [0], [0, 0, 0]):
        with pytest.raises(ValueError, match="row0"):
            crop.loss_components(x0, None, row0=bad)
    with pytest.raises(ValueError, match="row0"):
        crop.loss(x0, None, row0=[0, 9])
    r = crop._row0([0, 8], 2, 4, 12, "cpu")
    assert r.dtype == torch.int64 and r.tolist() == [0, 8]
    assert crop._row0(None, 2, 4, 12, "cpu") is None


# ------------------------------------------------------------------------------------------ checkpoint keys
def test_state_dict_keys_do_not_change():
    from cesm_emulator_amd.model import UNet
    net = UNet(ch_mults=(1, 2))
    plain = Diffusion(net)
    full = Diffusion(net, lat_weight=0.5, min_snr_gamma=5.0, lat=torch.linspace(-90, 90, 192))
    full.lat_weights(64, "cpu")
    assert list(full.state_dict()) == list(plain.state_dict())
    keys = [k for k in full.state_dict() if not k.startswith("model.")]
    assert keys == ["betas", "alphas", "alphas_cumprod", "alphas_cumprod_prev", "sqrt_alphas_cumprod",
                    "sqrt_one_minus_alphas_cumprod", "sqrt_recip_alphas", "posterior_variance"]
    plain.load_state_dict(full.state_dict())  # strict
    full.load_state_dict(plain.state_dict())
    # the table is a buffer all the same: it follows .to()
    assert full.to(torch.float64).min_snr_weight.dtype == torch.float64


# ------------------------------------------------------------------------------------------ config
def test_make_diffusion_reads_the_loss_block():
    net = torch.nn.Identity()
    d = make_diffusion(net, {"timesteps": 50})
    assert d.T == 50 and not d.weighted and d.model is net
    d = make_diffusion(net, {"timesteps": 20, "beta_schedule": "linear",
                             "loss": {"lat_weight": 0.25, "min_snr_gamma": 5}}, lat=np.linspace(-90, 90, 12))
    assert d.T == 20 and d.lat_weight == 0.25 and d.min_snr_gamma == 5.0 and d.weighted
    assert tuple(d.min_snr_weight.shape) == (20,) and d.lat_weights(4, "cpu").numel() == 12
    assert make_diffusion(net, {"loss": {"lat_weight": 1.0}}).min_snr_gamma is None
    with pytest.raises(ValueError, match="gamma"):
        make_diffusion(net, {"loss": {"lat_weight": 0.5, "gamma": 5}})
    with pytest.raises(ValueError):
        make_diffusion(net, {"loss": {"lat_weight": 2.0}})
    with pytest.raises(TypeError):
        make_diffusion(net, {"loss": [0.5]})
    with pytest.raises(ValueError, match="linear"):
        make_diffusion(net, {"beta_schedule": "cosine"})


@pytest.mark.parametrize("name", ["baseline", "more_blocks"])
def test_shipped_configs_keep_the_plain_loss_until_overridden(name):
    import os
    from cesm_emulator_amd import config as C
    cfg = C.load_config(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "config", name))
    assert not make_diffusion(torch.nn.Identity(), cfg["train"]).weighted
    C.apply_overrides(cfg, ["train.loss.lat_weight=0.5", "train.loss.min_snr_gamma=5"])
    d = make_diffusion(torch.nn.Identity(), cfg["train"])
    assert d.lat_weight == 0.5 and d.min_snr_gamma == 5.0


# ------------------------------------------------------------------------------------------ crop offsets
def test_row0_of_sampler_items_with_a_crop():
    """WindowSampler draws, per item, the time-reversal flag, then the crop's row and column offset (numpy's global
    RNG); row0_of is column 4, the row offset"""
    T, M, H, W, Kw, h, w = 6, 2, 12, 16, 3, 4, 8
    s = DA.WindowSampler(T, M, H, W, Kw, crop_hw=(h, w), time_reverse_p=0.5)
    idx = [5, 0, 3, 7]
    np.random.seed(11)
    items = s.items(idx)
    r0 = DA.row0_of(items)
    np.random.seed(11)
    want = []
    for _ in idx:
        np.random.rand()
        want.append(np.random.randint(0, H - h + 1))
        np.random.randint(0, W - w + 1)
    assert r0.dtype == torch.int64 and not r0.is_cuda and r0.tolist() == want
    assert len(set(want)) > 1 and all(0 <= v <= H - h for v in want)
    items[:, 4] = -1
    assert r0.tolist() == want  # a copy, not a view of the item rows
    # no crop: zeros; a centre crop: the one fixed offset
    assert DA.row0_of(DA.WindowSampler(T, M, H, W, Kw).items(idx)).tolist() == [0] * 4
    centre = DA.WindowSampler(T, M, H, W, Kw, crop_hw=(h, w), crop_mode="center")
    assert DA.row0_of(centre.items(idx)).tolist() == [4] * 4
    assert tuple(DA.row0_of(np.zeros((0, 6), dtype=np.int64)).shape) == (0,)
