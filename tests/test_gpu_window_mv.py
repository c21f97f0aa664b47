"""The V-variable window gather on the GPU: cesm_window_gather_mv against numpy fancy indexing (bit for bit), both
loaders on two-variable fields against the dataset restatement in all three sample modes, the unchanged V = 1 path, and
the multi-variable data path end to end (two training steps from the device loader, validate_ensemble in physical
units).  No test hands the kernel an out-of-range index: the host check is tested in tests/test_data_mv_host.py and
the kernel's clamp is defence, checked by reading it."""
import numpy as np
import pytest
import torch

from cesm_emulator_amd import data as DA
from cesm_emulator_amd import kernels as K
from cesm_emulator_amd.config import load_config
from cesm_emulator_amd.model import UNet, Diffusion
from cesm_emulator_amd.optim import FusedAdamW
from cesm_emulator_amd.train import rank_generator, train_one_epoch, validate_ensemble
from oracle.ref_data import WindowedAllMembersDatasetRef

pytestmark = pytest.mark.gpu

T, M, H, W = 11, 3, 10, 12


def _fields(V, Vc, shape=(T, M, H, W), seed=0):
    r = np.random.default_rng(seed)
    t, m, hh, ww = shape
    return (r.standard_normal((t, m, Vc, hh, ww)).astype(np.float32),
            r.standard_normal((t, m, V, hh, ww)).astype(np.float32))


def _numpy_gather(cond, tgt, times, meta, csel, h, w):
    n, Kw = times.shape
    V = tgt.shape[2]
    cw = np.empty((n, V, Kw, h, w), np.float32)
    x0 = np.empty((n, V, h, w), np.float32)
    for r in range(n):
        m, a, i, j = meta[r]
        cw[r] = cond[times[r], m][:, csel][:, :, i:i + h, j:j + w].transpose(1, 0, 2, 3)
        x0[r] = tgt[a, m][:, i:i + h, j:j + w]
    return cw, x0


def _edge_items(Kw, Tn, Mn, Hn, Wn, h, w, n=5):
    """n = 5 items on every edge: t = 0 and t = T - 1, i = H - h, j = W - w (odd where the crop leaves room: a
    misaligned source for the 16-byte stores), repeated times within a row, a reversed row"""
    di, dj = Hn - h, Wn - w
    odd_j = 1 if dj >= 1 else 0
    times = np.empty((n, Kw), np.int64)
    times[0] = np.arange(Kw) % Tn                      # starts at t = 0
    times[1] = Tn - 1 - (np.arange(Kw) % Tn)           # a reversed row that starts at t = T - 1
    times[2] = Tn // 2                                 # one frame repeated
    times[3] = np.arange(Kw)[::-1] // 2                # reversed, with repeats, ends at t = 0
    times[4] = (np.arange(Kw) * 3 + 1) % Tn            # out of order
    meta = np.array([[0, 0, 0, odd_j],
                     [Mn - 1, Tn - 1, di, dj],
                     [1 % Mn, Tn // 2, di, odd_j],
                     [0, Tn - 1, 0, dj],
                     [Mn - 1, 0, di // 2, min(dj, 3)]], np.int64)
    return times, meta


def _run_and_compare(dev, cond, tgt, times, meta, csel, h, w, device_indices=False):
    exp_c, exp_x = _numpy_gather(cond, tgt, times, meta, csel, h, w)
    dc, dt_ = torch.from_numpy(cond).to(dev), torch.from_numpy(tgt).to(dev)
    tt, mm = torch.from_numpy(times), torch.from_numpy(meta)
    if device_indices:
        tt, mm = tt.to(dev), mm.to(dev)
    outs = []
    for _ in range(2):
        # NaN everywhere first, so an element the kernel leaves unwritten shows
        cw = torch.full(exp_c.shape, float("nan"), device=dev)
        x0 = torch.full(exp_x.shape, float("nan"), device=dev)
        K.window_gather_mv(dc, dt_, tt, mm, csel, h, w, out=(cw, x0))
        outs.append((cw.cpu(), x0.cpu()))
    cw, x0 = K.window_gather_mv(dc, dt_, tt, mm, csel, h, w)  # and into outputs of its own
    assert torch.equal(cw.cpu(), outs[0][0]) and torch.equal(x0.cpu(), outs[0][1])
    assert outs[0][0].shape == exp_c.shape and outs[0][1].shape == exp_x.shape
    assert torch.equal(outs[0][0], torch.from_numpy(exp_c)) and torch.equal(outs[0][1], torch.from_numpy(exp_x))
    # two launches: identical bits (NaN-free by the comparison above, so torch.equal is a bit comparison)
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


@pytest.mark.parametrize("crop", [(6, 8), (7, 9), None], ids=["vec6x8", "scalar7x9", "full"])
@pytest.mark.parametrize("one_forcing", [False, True], ids=["VcV", "Vc1"])
@pytest.mark.parametrize("V", [1, 2, 3, 4])
@pytest.mark.parametrize("Kw", [2, 5])
def test_kernel_equals_numpy_indexing(dev, Kw, V, one_forcing, crop):
    Vc = 1 if one_forcing else V
    cond, tgt = _fields(V, Vc, seed=V * 10 + Kw)
    csel = [0] * V if one_forcing else list(range(V))[::-1]  # Vc = V: a permutation, so a wrong plane shows
    h, w = crop if crop else (H, W)
    times, meta = _edge_items(Kw, T, M, H, W, h, w)
    _run_and_compare(dev, cond, tgt, times, meta, csel, h, w, device_indices=(V % 2 == 0))


def test_kernel_grid_stride_wraps(dev):
    """n = 67 items of 16 x 24 crops, K = 3, V = 2: 8576 rows on 42 row slots per block and two rows per slot before the
    grid grows, so every slot takes more than one row"""
    shape = (9, 3, 20, 31)
    cond, tgt = _fields(2, 2, shape, seed=5)
    r = np.random.default_rng(6)
    n, Kw, h, w = 67, 3, 16, 24
    times = r.integers(0, shape[0], (n, Kw))
    meta = np.stack([r.integers(0, shape[1], n), r.integers(0, shape[0], n), r.integers(0, shape[2] - h + 1, n),
                     r.integers(0, shape[3] - w + 1, n)], axis=1)
    times[:5], meta[:5] = _edge_items(Kw, *shape, h, w)
    _run_and_compare(dev, cond, tgt, times.astype(np.int64), meta.astype(np.int64), [1, 0], h, w)


def test_unsupported_shapes_raise_value_error(dev):
    """what the library rejects (CESM_EUNSUPPORTED) reaches the caller as ValueError: asked of the entry point itself,
    past the wrapper's own checks"""
    cond, tgt = (torch.zeros(T, M, 2, H, W, device=dev) for _ in range(2))
    tt, mm = torch.zeros(2, 3, dtype=torch.int64, device=dev), torch.zeros(2, 4, dtype=torch.int64, device=dev)
    out_c, out_x = torch.zeros(2, 2, 3, 6, 8, device=dev), torch.zeros(2, 2, 6, 8, device=dev)

    def call(V=2, Vc=2, csel=(0, 1, 0, 0), Kw=3, h=6, w=8):
        K._mv_call("cesm_window_gather_mv", "probe", K.P(cond), K.P(tgt), K.P(tt), K.P(mm), K.P(out_c), K.P(out_x), 2,
                   Kw, V, Vc, *csel, T, M, H, W, h, w, K.S())

    call()
    for bad in (dict(V=0), dict(V=5), dict(csel=(0, 2, 0, 0)), dict(csel=(-1, 0, 0, 0)), dict(h=H + 1), dict(w=W + 1),
                dict(Kw=0)):
        with pytest.raises(ValueError, match="unsupported"):
            call(**bad)
    torch.cuda.synchronize()


# ------------------------------------------------------------------ loaders vs the dataset restatement
@pytest.mark.parametrize("kind", ["device", "pinned"])
@pytest.mark.parametrize("mode,extra", [("consecutive", {}), ("random_window", dict(window_radius=2)),
                                        ("random_global", dict(keep_chronology=False))],
                         ids=["consecutive", "random_window", "random_global"])
def test_loader_batches_bit_equal_to_dataset(dev, kind, mode, extra):
    """(T, M, 2, H, W) fields: every batch == the dataset's items for the same indices under the same numpy seed, and
    last_row0 == the crop rows drawn (a second sampler replays the same numpy stream)"""
    cond, tgt = _fields(2, 2, seed=3)
    Kw, bs, crop = 5, 4, (7, 9)
    ref = WindowedAllMembersDatasetRef(cond, tgt, K=Kw, center=True, crop_hw=crop, time_reverse_p=0.5, sample_mode=mode,
                                       **extra)
    cls = DA.PinnedWindowLoader if kind == "pinned" else DA.DeviceWindowLoader
    ld = cls(cond, tgt, Kw, bs, dev, center=True, crop_hw=crop, time_reverse_p=0.5, shuffle=True, seed=3,
             sample_mode=mode, **extra)
    ld.set_epoch(1)
    assert len(ld.sampler) == len(ref)
    batches = DA.shard_indices(len(ref), bs, 0, 1, True, 3, 1)
    np.random.seed(123)
    got = [(c.clone(), x.clone(), ld.last_row0.clone()) for c, x in ld]
    assert len(got) == len(batches)
    # the crop rows the dataset draws: a second sampler replays the same numpy stream
    smp = DA.WindowSampler(T, M, H, W, Kw, True, crop, "random", 0.5, mode, **extra)
    np.random.seed(123)
    rows = [smp.draw(idx)[1][:, 2] for idx in batches]
    np.random.seed(123)
    for (c, x, row0), idx, rr in zip(got, batches, rows):
        items = [ref[i] for i in idx]
        assert c.shape == (len(idx), 2, Kw, *crop) and x.shape == (len(idx), 2, *crop)
        assert torch.equal(c.cpu(), torch.stack([a for a, _ in items]))
        assert torch.equal(x.cpu(), torch.stack([b for _, b in items]))
        assert row0.dtype == torch.int64 and torch.equal(row0, torch.from_numpy(rr))
    assert len({int(v) for _, _, r in got for v in r}) > 1  # the crops really differ


def test_one_forcing_feeds_both_cond_channels(dev):
    cond, tgt = _fields(2, 1, seed=4)
    ld = DA.DeviceWindowLoader(cond, tgt, 3, 4, dev, crop_hw=(6, 8), shuffle=False)
    assert ld.csel == [0, 0]
    np.random.seed(1)
    c, x = next(iter(ld))
    assert c.shape == (4, 2, 3, 6, 8) and torch.equal(c[:, 0], c[:, 1])
    with pytest.raises(ValueError, match="cond_select"):
        DA.DeviceWindowLoader(_fields(3, 2)[0], _fields(3, 2)[1], 3, 4, dev)


@pytest.mark.parametrize("kind", ["device", "pinned"])
def test_single_variable_consecutive_path_is_unchanged(dev, kind, monkeypatch):
    """a 4-D input and the same data as (T, M, 1, H, W), consecutive mode: bit-equal batches from the same draws, both
    through cesm_window_gather (the V = 1 kernel), never the new one"""
    monkeypatch.setattr(K, "window_gather_mv", lambda *a, **k: pytest.fail("V = 1 consecutive took the new kernel"))
    monkeypatch.setattr(DA, "host_gather_mv", lambda *a, **k: pytest.fail("V = 1 consecutive took the new gather"))
    cond, tgt = _fields(1, 1, seed=8)
    cls = DA.PinnedWindowLoader if kind == "pinned" else DA.DeviceWindowLoader
    out = []
    for c_in, t_in in ((cond[:, :, 0], tgt[:, :, 0]), (cond, tgt)):
        ld = cls(c_in, t_in, 5, 4, dev, crop_hw=(7, 9), time_reverse_p=0.5, seed=2)
        np.random.seed(9)
        out.append([(c.clone(), x.clone(), ld.last_row0.clone()) for c, x in ld])
        state = np.random.get_state()[1].copy()
        out[-1].append(state)
    assert np.array_equal(out[0].pop(), out[1].pop())  # the same number of draws
    assert len(out[0]) == len(out[1]) > 1
    for (c4, x4, r4), (c5, x5, r5) in zip(*out):
        assert c4.shape[1:] == (1, 5, 7, 9) and x4.shape[1:] == (1, 7, 9)
        assert torch.equal(c4, c5) and torch.equal(x4, x5) and torch.equal(r4, r5)


@pytest.mark.parametrize("name", ["baseline", "more_blocks"])
def test_loader_from_config_builds_and_yields(dev, name):
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cfg = load_config(os.path.join(root, "config", name))
    cfg["train"]["batch_size"] = 3
    cond, tgt = _fields(2, 1, seed=2)
    for kind in ("device", "pinned"):
        ld = DA.loader_from_config(cfg, cond, tgt, dev, kind=kind)
        np.random.seed(0)
        c, x = next(iter(ld))
        assert c.shape == (3, 2, cfg["dataset"]["K"], H, W) and x.shape == (3, 2, H, W)  # crops clipped to the grid


# ------------------------------------------------------------------ end to end
def test_two_variable_training_and_validation_end_to_end(dev):
    """UNet(out_channels=2) on 16 x 24 crops, K = 3, fp32: two train_one_epoch steps fed by the device loader == the
    same two steps fed tensors assembled with numpy from the same draws (loss and parameters, bit for bit);
    validate_ensemble(norm=) reports rmse as target_std[v] x the value without norm"""
    shape = (4, 2, 20, 31)
    cond, tgt = _fields(2, 1, shape, seed=11)
    Kw, bs, crop = 3, 2, (16, 24)
    norm = {"cond_vars": ["CO2"], "target_vars": ["TREFHT", "PRECT"], "cond_mean": [0.0], "cond_std": [1.0],
            "target_mean": [288.0, 1e-5], "target_std": [20.5, 1.25e-5]}

    class TwoBatches:
        """the first two batches of a loader (train_one_epoch runs the whole iterable)"""
        def __init__(self, ld):
            self.ld = ld

        def __iter__(self):
            for k, b in enumerate(self.ld):
                if k == 2:
                    return
                self.last_row0 = self.ld.last_row0
                yield b

    def loader():
        return DA.DeviceWindowLoader(cond, tgt, Kw, bs, dev, crop_hw=crop, time_reverse_p=0.5, seed=0)

    def numpy_batches():
        smp = DA.WindowSampler(*[shape[0], shape[1], shape[2], shape[3]], Kw, True, crop, "random", 0.5)
        out = []
        for idx in DA.shard_indices(len(smp), bs, 0, 1, True, 0, 0)[:2]:
            times, meta = smp.draw(idx)
            cw, x0 = _numpy_gather(cond, tgt, times, meta, [0, 0], *crop)
            out.append((torch.from_numpy(cw), torch.from_numpy(x0)))
        return out

    res = {}
    for feed in ("loader", "numpy"):
        torch.manual_seed(0)
        net = UNet(out_channels=2, ch_mults=(1, 2)).to(dev)
        d = Diffusion(net).to(dev)
        d.generator = rank_generator(dev, 2, 0)
        opt = FusedAdamW(d.parameters(), lr=1e-3, max_grad_norm=1.0)
        np.random.seed(7)
        dl = TwoBatches(loader()) if feed == "loader" else numpy_batches()
        loss = train_one_epoch(d, dl, opt, dev, 1.0, use_amp=False)
        torch.cuda.synchronize()
        res[feed] = (loss, opt.flat.data.clone())
    print(f"epoch loss: loader {res['loader'][0]:.6f} numpy {res['numpy'][0]:.6f}")
    assert np.isfinite(res["loader"][0])
    assert res["loader"][0] == res["numpy"][0] and torch.equal(res["loader"][1], res["numpy"][1])

    def run(**kw):
        np.random.seed(21)
        torch.manual_seed(8)
        torch.cuda.manual_seed(8)
        return validate_ensemble(d, loader(), 3, steps=2, max_batches=1, **kw)

    plain, phys = run(), run(norm=norm)
    s = torch.tensor(norm["target_std"], dtype=torch.float64, device=plain["rmse"].device)
    assert plain["rmse"].shape == (2,) and bool(torch.isfinite(plain["rmse"]).all())
    assert torch.equal(phys["rmse"], plain["rmse"] * s)
    assert torch.equal(phys["crps"], plain["crps"] * s) and torch.equal(phys["mse"], plain["mse"] * (s * s))
    assert torch.equal(phys["ssr"], plain["ssr"]) and torch.equal(phys["rank_hist"], plain["rank_hist"])
