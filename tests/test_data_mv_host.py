"""CPU tests of the multi-variable data path: WindowSampler.draw + host_gather_mv against the dataset restatement
(oracle.ref_data.WindowedAllMembersDatasetRef, every sample mode, bit for bit), load_fields / denormalize, the
normalisation statistics in the checkpoint, summarize(scale=), loader_from_config's argument mapping and the host
range check of kernels.window_gather_mv (raised before the library is touched: no GPU needed)."""
import itertools
import os

import numpy as np
import pytest
import torch

from cesm_emulator_amd import checkpoint as CK
from cesm_emulator_amd import data as D
from cesm_emulator_amd import kernels as K
from cesm_emulator_amd.config import load_config
from cesm_emulator_amd.ensemble import summarize
from oracle.ref_data import WindowedAllMembersDatasetRef

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T, M, H, W = 11, 3, 10, 12
MODES = [("consecutive", 5), ("random_window", 2), ("random_window", 5), ("random_global", 5)]


def _fields(V, seed=0):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((T, M, V, H, W)).astype(np.float32),
            rng.standard_normal((T, M, V, H, W)).astype(np.float32))


def _compare(cond, tgt, csel, idx, seed, Kw, **kw):
    """the items idx of the oracle dataset (fed cond[:, :, csel]) against draw + host_gather_mv, same numpy seed"""
    V = tgt.shape[2]
    ref = WindowedAllMembersDatasetRef(np.ascontiguousarray(cond[:, :, csel]), tgt, K=Kw, **kw)
    smp = D.WindowSampler(T, M, H, W, Kw, kw.pop("center"), kw.pop("crop_hw"), "random", kw.pop("time_reverse_p"),
                          kw.pop("sample_mode"), **kw)
    assert len(ref) == len(smp)
    idx = [i for i in idx if i < len(ref)]
    np.random.seed(seed)
    exp = [ref[i] for i in idx]
    np.random.seed(seed)
    times, meta = smp.draw(idx)
    assert times.shape == (len(idx), Kw) and meta.shape == (len(idx), 4)
    assert times.dtype == np.int64 and meta.dtype == np.int64
    h, w = smp.hw
    oc = np.full((len(idx), V, Kw, h, w), np.nan, np.float32)
    ox = np.full((len(idx), V, h, w), np.nan, np.float32)
    D.host_gather_mv(cond, tgt, times, meta, csel, h, w, oc, ox)
    for n, (c, x) in enumerate(exp):
        c = c.numpy()
        if c.shape[1] != Kw:
            # causal at anchor 0: the pool is empty, every frame is the anchor, and the dataset's "drop the anchor, put
            # it last" leaves a ONE-frame window.  The sampler keeps K frames, all the anchor (WindowSampler notes it).
            assert c.shape[1] == 1 and kw["causal"] and meta[n, 1] == 0 and (times[n] == 0).all()
            c = np.repeat(c, Kw, axis=1)
        np.testing.assert_array_equal(oc[n], c)
        np.testing.assert_array_equal(ox[n], x.numpy())
    assert smp.allow_replace == ref.allow_replace and smp.center == ref.center
    return smp


@pytest.mark.parametrize("Kw", [2, 5])
@pytest.mark.parametrize("mode,radius", MODES)
def test_draw_and_host_gather_match_dataset(mode, radius, Kw):
    """center x causal x keep_chronology x time_reverse_p x crop, the variable count V and the forcing layout (Vc = V
    with the identity, Vc = 1 feeding all V channels) cycling over the combinations so each value meets each option"""
    combos = itertools.product((True, False), (False, True), (True, False), (0.0, 0.5, 1.0), ((7, 9), (6, 8), None))
    for n, (center, causal, chron, p, crop) in enumerate(combos):
        V = (1, 2, 4)[n % 3]
        one_forcing = (n // 3) % 2 == 1
        cond, tgt = _fields(V, seed=n)
        if one_forcing:
            cond, csel = cond[:, :, :1], [0] * V
        else:
            csel = list(range(V))
        _compare(cond, tgt, csel, range(n % 2, T * M, 2), 100 + n, Kw, center=center, crop_hw=crop, time_reverse_p=p,
                 sample_mode=mode, window_radius=radius, keep_chronology=chron, causal=causal)


@pytest.mark.parametrize("V", [1, 2, 4])
def test_short_pool_turns_replacement_on_for_good(V):
    """radius 1 and K = 5: pool_wo_anchor holds at most 2 < 4 frames, so the first item switches allow_replace on and it
    stays on; every later item still agrees with the dataset"""
    cond, tgt = _fields(V, seed=7)
    smp = _compare(cond, tgt, list(range(V)), range(T * M), 5, 5, center=True, crop_hw=(7, 9), time_reverse_p=0.5,
                   sample_mode="random_window", window_radius=1, keep_chronology=True, causal=False,
                   allow_replace=False)
    assert smp.allow_replace is True


def test_sampler_lengths_and_consecutive_items_unchanged():
    for mode in ("random_window", "random_global"):
        assert len(D.WindowSampler(T, M, H, W, 5, sample_mode=mode)) == T * M
    assert len(D.WindowSampler(T, M, H, W, 5)) == (T - 4) * M
    with pytest.raises(ValueError):
        D.WindowSampler(T, M, H, W, 5, sample_mode="other")
    # consecutive mode: draw() is items() with the reversal applied to the times, from the same RNG draws
    smp = D.WindowSampler(T, M, H, W, 5, True, (7, 9), "random", 0.5)
    idx = list(range(len(smp)))
    np.random.seed(3)
    items = smp.items(idx)
    np.random.seed(3)
    times, meta = smp.draw(idx)
    np.testing.assert_array_equal(meta, items[:, [1, 2, 4, 5]])
    np.testing.assert_array_equal(D.row0_of(items).numpy(), meta[:, 2])
    for it, tt in zip(items, times):
        fwd = np.arange(it[0], it[0] + 5)
        np.testing.assert_array_equal(tt, fwd[[1, 0, 2, 4, 3]] if it[3] else fwd)
    assert D.WindowSampler(T, M, H, W, 5, True, causal=True).center is False


def test_cond_select_defaults():
    assert D.resolve_cond_select(None, 3, 3) == [0, 1, 2]
    assert D.resolve_cond_select(None, 1, 2) == [0, 0]
    assert D.resolve_cond_select((1, 1, 0), 2, 3) == [1, 1, 0]
    with pytest.raises(ValueError):
        D.resolve_cond_select(None, 2, 3)
    with pytest.raises(ValueError):
        D.resolve_cond_select([0, 2], 2, 2)
    with pytest.raises(ValueError):
        D.resolve_cond_select([0], 2, 2)


# ------------------------------------------------------------------ load_fields / denormalize
def _physical(rng, shape):
    """three variables with per-variable offsets 0 / 288 / 1e-5.  The spreads follow from what float32 and the
    reference's formula allow at a tolerance of 1e-6, not from the code: (a) the divisor is std + 1e-8, so the result's
    std is sigma / (sigma + 1e-8), within 1e-6 of 1 only for sigma >= 1e-2: the small-offset variable gets 0.05;
    (b) the mean is subtracted in float32, where 288 is known to half an ulp = 1.5e-5, so the result's mean is within
    1e-6 only for sigma >= 15: the temperature gets 20 K, the spread of surface temperature over the globe."""
    return (rng.standard_normal(shape), 288.0 + 20.0 * rng.standard_normal(shape),
            1e-5 + 0.05 * rng.standard_normal(shape))


def test_load_fields_single_variable_is_zscore(tmp_path):
    rng = np.random.default_rng(2)
    a = (rng.standard_normal((T, M, H, W)) * 7 + 3).astype(np.float32)
    b = (rng.standard_normal((T, M, H, W)) * 20 + 288).astype(np.float32)
    np.savez(tmp_path / "c.npz", CO2=a)
    np.save(tmp_path / "t.npy", b[:, :, None])
    c, t, norm = D.load_fields(tmp_path / "c.npz", tmp_path / "t.npy", "CO2", None)
    za, ma, sa = D.zscore(a)
    zb, mb, sb = D.zscore(b)
    assert c.shape == (T, M, 1, H, W) and t.shape == (T, M, 1, H, W)
    np.testing.assert_array_equal(c[:, :, 0], za)
    np.testing.assert_array_equal(t[:, :, 0], zb)
    assert norm["cond_mean"] == [ma] and norm["cond_std"] == [sa]
    assert norm["target_mean"] == [mb] and norm["target_std"] == [sb]
    assert norm["cond_vars"] == ["CO2"] and len(norm["target_vars"]) == 1
    # and the legacy loader is what it was
    c4, _ = D.load_cond_and_target(tmp_path / "c.npz", tmp_path / "t.npy", "CO2")
    np.testing.assert_array_equal(c4, za)
    c_raw, t_raw, n_raw = D.load_fields(tmp_path / "c.npz", tmp_path / "t.npy", "CO2", None, normalize=False)
    np.testing.assert_array_equal(c_raw[:, :, 0], a)
    assert n_raw["target_mean"] == [0.0] and n_raw["target_std"] == [1.0]


def test_load_fields_three_variables_and_round_trip(tmp_path):
    """per-variable z-scores: every plane has mean 0 and std 1 to 1e-6 (judged in float64), whatever the variable's
    offset; denormalize gives the input back to 2 ulp of the input's scale"""
    rng = np.random.default_rng(4)
    raw = [v.astype(np.float32) for v in _physical(rng, (T, M, H, W))]
    np.savez(tmp_path / "t.npz", anom=raw[0], TREFHT=raw[1], PRECT=raw[2])
    np.savez(tmp_path / "c.npz", CO2=rng.standard_normal((T, M, H, W)).astype(np.float32))
    names = ["anom", "TREFHT", "PRECT"]
    c, t, norm = D.load_fields(tmp_path / "c.npz", tmp_path / "t.npz", ["CO2"], names)
    assert c.shape == (T, M, 1, H, W) and t.shape == (T, M, 3, H, W) and t.dtype == np.float32
    assert norm["target_vars"] == names and norm["cond_vars"] == ["CO2"]
    assert all(isinstance(v, float) for k in ("cond_mean", "cond_std", "target_mean", "target_std") for v in norm[k])
    for v in range(3):
        z = t[:, :, v].astype(np.float64)
        print(f"{names[v]}: mean {z.mean():.3e} std - 1 {z.std() - 1:.3e}")
    for v in range(3):
        z = t[:, :, v].astype(np.float64)
        assert abs(z.mean()) <= 1e-6, (names[v], z.mean())
        assert abs(z.std() - 1.0) <= 1e-6, (names[v], z.std())
    # what (a) above means for a variable stored with a tiny spread (a precipitation rate in kg m-2 s-1): its z-score
    # has the std sigma / (sigma + 1e-8), the reference's formula, not 1
    tiny = (1e-5 + 1e-5 * rng.standard_normal((T, M, H, W))).astype(np.float32)
    np.save(tmp_path / "tiny.npy", tiny)
    _, zt, nt = D.load_fields(tmp_path / "c.npz", tmp_path / "tiny.npy", "CO2", None)
    sigma = nt["target_std"][0] - 1e-8
    assert abs(zt.astype(np.float64).std() - sigma / (sigma + 1e-8)) <= 1e-6 and 0.998 < zt.std() < 0.9995
    # the same three planes as one 5-D array under a single key
    np.savez(tmp_path / "t5.npz", fields=np.stack(raw, axis=2))
    _, t5, norm5 = D.load_fields(tmp_path / "c.npz", tmp_path / "t5.npz", "CO2", "fields")
    np.testing.assert_array_equal(t5, t)
    assert norm5["target_mean"] == norm["target_mean"] and norm5["target_std"] == norm["target_std"]
    # round trip, [B, V, H, W] and [B, M, V, H, W]
    back = D.denormalize(torch.from_numpy(t[0]), norm)          # [M, V, H, W] read as a batch of M
    back5 = D.denormalize(torch.from_numpy(t[:2]), norm)        # [2, M, V, H, W]
    assert torch.equal(back5[0], back)
    for v in range(3):
        scale = np.abs(raw[v]).max()
        ulp = float(np.spacing(np.float32(scale)))
        err = np.abs(back[:, v].numpy().astype(np.float64) - raw[v][0].astype(np.float64)).max()
        print(f"{names[v]}: round-trip error {err:.3e} = {err / ulp:.2f} ulp of {scale:.3e}")
        assert err <= 2 * ulp, (names[v], err, ulp)
    with pytest.raises(ValueError):
        D.denormalize(torch.zeros(2, 2, 4, 4), norm)


# ------------------------------------------------------------------ checkpoint
def test_norm_survives_the_checkpoint(tmp_path):
    from cesm_emulator_amd.model import UNet, Diffusion
    cfg = {"unet": {"in_channels": 4, "out_channels": 2, "base_ch": 64, "ch_mults": [1, 2], "groups": 8},
           "train": {"timesteps": 1000, "beta_schedule": "linear"}}
    norm = {"cond_vars": ["CO2"], "target_vars": ["TREFHT", "PRECT"], "cond_mean": [np.float32(1.5)],
            "cond_std": [2.0], "target_mean": [288.25, 1e-5], "target_std": [20.5, np.float64(1.25e-5)]}
    torch.manual_seed(0)
    diff = Diffusion(UNet(in_channels=4, out_channels=2, ch_mults=(1, 2)))
    CK.save_checkpoint(tmp_path / "with.pt", diff, None, 3, cfg, norm=norm)
    CK.save_checkpoint(tmp_path / "without.pt", diff, None, 3, cfg)
    ck = torch.load(tmp_path / "with.pt", weights_only=True)
    assert set(ck) == {"epoch", "model", "diffusion_buffers", "optimizer", "config", "norm"}
    assert "norm" not in ck["config"]
    d2, cfg2 = CK.load_diffusion_from_checkpoint(tmp_path / "with.pt", device="cpu")
    assert cfg2["norm"] == {k: [float(x) if not isinstance(x, str) else x for x in v] for k, v in norm.items()}
    assert {k: v for k, v in cfg2.items() if k != "norm"} == cfg
    for (k, a), (_, b) in zip(diff.state_dict().items(), d2.state_dict().items()):
        assert torch.equal(a, b), k
    assert set(torch.load(tmp_path / "without.pt", weights_only=True)) == {"epoch", "model", "diffusion_buffers",
                                                                          "optimizer", "config"}
    _, cfg3 = CK.load_diffusion_from_checkpoint(tmp_path / "without.pt", device="cpu")
    assert cfg3 == cfg


# ------------------------------------------------------------------ summarize(scale=)
def test_summarize_in_physical_units():
    Mm, V = 5, 3
    g = torch.Generator().manual_seed(1)
    acc = torch.rand(V, 4 + Mm + 1, generator=g, dtype=torch.float64) + 0.5
    scale = [20.5, 1.25e-5, 1.0]
    s = torch.tensor(scale, dtype=torch.float64)
    sw, mse, var, crps = acc[:, 0], acc[:, 1] / acc[:, 0], acc[:, 2] / acc[:, 0], acc[:, 3] / acc[:, 0]
    r = summarize(acc, Mm, scale=scale)
    torch.testing.assert_close(r["mse"], mse * s * s, rtol=1e-15, atol=0)
    torch.testing.assert_close(r["var"], var * s * s, rtol=1e-15, atol=0)
    torch.testing.assert_close(r["rmse"], mse.sqrt() * s, rtol=1e-15, atol=0)
    torch.testing.assert_close(r["spread"], var.sqrt() * s, rtol=1e-15, atol=0)
    torch.testing.assert_close(r["crps"], crps * s, rtol=1e-15, atol=0)
    plain = summarize(acc, Mm)
    assert torch.equal(r["ssr"], plain["ssr"]) and torch.equal(r["rank_hist"], plain["rank_hist"])
    assert torch.equal(plain["ssr"], ((Mm + 1) / Mm * var / mse).sqrt())
    assert torch.equal(plain["rmse"], mse.sqrt()) and torch.equal(plain["crps"], crps)
    no_obs = summarize(acc, Mm, has_obs=False, scale=scale)
    assert no_obs["mse"] is None and torch.equal(no_obs["spread"], r["spread"])
    with pytest.raises(ValueError):
        summarize(acc, Mm, scale=[1.0, 2.0])


# ------------------------------------------------------------------ loader_from_config
class _Recorder:
    def __init__(self, *args, **kw):
        self.args, self.kw = args, kw


@pytest.mark.parametrize("name", ["baseline", "more_blocks"])
@pytest.mark.parametrize("kind", ["device", "pinned"])
def test_loader_from_config(monkeypatch, name, kind):
    """both shipped configs map onto the loaders' arguments (the loaders themselves need a GPU:
    tests/test_gpu_window_mv.py builds them through loader_from_config)"""
    monkeypatch.setattr(D, "DeviceWindowLoader", type("Dev", (_Recorder,), {}))
    monkeypatch.setattr(D, "PinnedWindowLoader", type("Pin", (_Recorder,), {}))
    cfg = load_config(os.path.join(ROOT, "config", name))
    ds = cfg["dataset"]
    cond, tgt = object(), object()
    ld = D.loader_from_config(cfg, cond, tgt, "cuda:0", kind=kind, cond_select=[0, 0], rank=1, world=2)
    assert type(ld).__name__ == {"device": "Dev", "pinned": "Pin"}[kind]
    assert ld.args == (cond, tgt, ds["K"], cfg["train"]["batch_size"], "cuda:0")
    assert ld.kw == dict(center=ds["center"], crop_hw=tuple(ds["crop_hw"]), crop_mode=ds["crop_mode"],
                         time_reverse_p=ds["time_reverse_p"], shuffle=True, seed=cfg["train"]["seed"], rank=1, world=2,
                         cond_select=[0, 0], sample_mode=ds["sample_mode"], window_radius=ds["window_radius"],
                         keep_chronology=ds["keep_chronology"], causal=ds["causal"])
    # and the sampler takes exactly these
    smp = D.WindowSampler(T, M, H, W, ds["K"], ds["center"], ld.kw["crop_hw"], ds["crop_mode"], ds["time_reverse_p"],
                          ds["sample_mode"], window_radius=ds["window_radius"], keep_chronology=ds["keep_chronology"],
                          causal=ds["causal"])
    assert smp.hw == (H, W)  # the configs' crops are larger than this grid
    with pytest.raises(ValueError):
        D.loader_from_config(cfg, cond, tgt, "cuda:0", kind="workers")


# ------------------------------------------------------------------ host range check of the kernel wrapper
def _gather_args(V=2, Vc=1, n=3, Kw=3):
    cond = torch.zeros(T, M, Vc, H, W)
    tgt = torch.zeros(T, M, V, H, W)
    times = torch.zeros(n, Kw, dtype=torch.int64)
    meta = torch.zeros(n, 4, dtype=torch.int64)
    return cond, tgt, times, meta


@pytest.mark.parametrize("field,where,value,match", [
    ("times", (1, 2), T, rf"times = {T} "),
    ("meta", (2, 1), -1, r"anchor .* = -1 "),
    ("meta", (0, 2), H - 7 + 1, rf"i .* = {H - 7 + 1} "),
    ("meta", (0, 3), W - 8 + 1, rf"j .* = {W - 8 + 1} "),
    ("meta", (1, 0), M, rf"member .* = {M} "),
])
def test_host_range_check_names_field_and_value(monkeypatch, field, where, value, match):
    monkeypatch.setattr(K, "lib", lambda: pytest.fail("the library was touched before the range check"))
    cond, tgt, times, meta = _gather_args()
    {"times": times, "meta": meta}[field][where] = value
    with pytest.raises(ValueError, match=match):
        K.window_gather_mv(cond, tgt, times, meta, [0, 0], 7, 8)


def test_host_check_rejects_csel_and_shapes(monkeypatch):
    monkeypatch.setattr(K, "lib", lambda: pytest.fail("the library was touched before the range check"))
    cond, tgt, times, meta = _gather_args(V=2, Vc=2)
    with pytest.raises(ValueError, match=r"csel = 2 "):
        K.window_gather_mv(cond, tgt, times, meta, [0, 2], 7, 8)
    with pytest.raises(ValueError):
        K.window_gather_mv(cond, tgt, times, meta, [0], 7, 8)          # one index per variable
    with pytest.raises(ValueError):
        K.window_gather_mv(cond, tgt, times, meta, [0, 1], H + 1, 8)   # crop larger than the grid
    c5, t5, _, _ = _gather_args(V=5, Vc=5)
    with pytest.raises(ValueError):
        K.window_gather_mv(c5, t5, times, meta, [0, 1, 2, 3, 4], 7, 8)  # V > 4
    with pytest.raises(RuntimeError):
        K.window_gather_mv(cond, tgt, times.int(), meta, [0, 1], 7, 8)  # dtype
    # in range: the next thing the wrapper asks for is device tensors
    with pytest.raises(RuntimeError, match="device tensors"):
        K.window_gather_mv(cond, tgt, times, meta, [0, 1], 7, 8)
