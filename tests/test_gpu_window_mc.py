"""The window gather with the cond plane count separated from V (cesm_window_gather_mc) against its numpy twin
(data.host_gather_mv), bit for bit, in all three sample modes on both store paths; the clamping contract for device
indices; and both loaders feeding a UNet(out_channels=1, cond_channels=3) for two training steps."""
import numpy as np
import pytest
import torch

from cesm_emulator_amd import data as DA
from cesm_emulator_amd import kernels as K
from cesm_emulator_amd.model import UNet, Diffusion
from cesm_emulator_amd.optim import FusedAdamW
from cesm_emulator_amd.train import rank_generator, train_one_epoch

pytestmark = pytest.mark.gpu

T, M, H, W = 9, 2, 12, 16
#          V  Cc Vc  cond_select
COUNTS = [(1, 3, 3, [2, 0, 1]), (2, 3, 4, [3, 0, 2]), (1, 2, 2, [1, 0])]
MODES = [("consecutive", {}), ("random_window", dict(window_radius=2)), ("random_global", dict(keep_chronology=False))]


def _fields(V, Vc, shape=(T, M, H, W), seed=0):
    r = np.random.default_rng(seed)
    t, m, hh, ww = shape
    return (r.standard_normal((t, m, Vc, hh, ww)).astype(np.float32),
            r.standard_normal((t, m, V, hh, ww)).astype(np.float32))


def _twin(cond, tgt, times, meta, csel, h, w):
    n, Kw = times.shape
    oc = np.full((n, len(csel), Kw, h, w), np.nan, np.float32)
    ox = np.full((n, tgt.shape[2], h, w), np.nan, np.float32)
    DA.host_gather_mv(cond, tgt, times, meta, csel, h, w, oc, ox)
    return torch.from_numpy(oc), torch.from_numpy(ox)


def _gather_twice(dev, cond, tgt, tt, mm, csel, h, w, shapes):
    dc, dt_ = torch.from_numpy(cond).to(dev), torch.from_numpy(tgt).to(dev)
    outs = []
    for _ in range(2):
        cw = torch.full(shapes[0], float("nan"), device=dev)   # an element the kernel leaves unwritten shows
        x0 = torch.full(shapes[1], float("nan"), device=dev)
        K.window_gather_mc(dc, dt_, tt, mm, csel, h, w, out=(cw, x0))
        outs.append((cw.cpu(), x0.cpu()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    cw, x0 = K.window_gather_mc(dc, dt_, tt, mm, csel, h, w)   # and into outputs of its own
    assert torch.equal(cw.cpu(), outs[0][0]) and torch.equal(x0.cpu(), outs[0][1])
    return outs[0]


@pytest.mark.parametrize("crop", [(6, 8), (5, 7)], ids=["vec6x8", "scalar5x7"])
@pytest.mark.parametrize("mode,extra", MODES, ids=[m for m, _ in MODES])
@pytest.mark.parametrize("V,Cc,Vc,csel", COUNTS, ids=["V1_Cc3_Vc3", "V2_Cc3_Vc4", "V1_Cc2_Vc2"])
def test_kernel_equals_numpy_twin(dev, V, Cc, Vc, csel, mode, extra, crop):
    cond, tgt = _fields(V, Vc, seed=10 * V + Cc)
    Kw = 3
    smp = DA.WindowSampler(T, M, H, W, Kw, True, crop, "random", 0.5, mode, **extra)
    np.random.seed(5 + Cc)
    times, meta = smp.draw(list(range(0, len(smp), max(1, len(smp) // 7)))[:7])
    # the corners of the index ranges as well
    times = np.concatenate([times, [[0] * Kw, [T - 1] * Kw]]).astype(np.int64)
    meta = np.concatenate([meta, [[0, 0, 0, 1], [M - 1, T - 1, H - crop[0], W - crop[1]]]]).astype(np.int64)
    exp_c, exp_x = _twin(cond, tgt, times, meta, csel, *crop)
    assert exp_c.shape == (len(times), Cc, Kw, *crop)
    tt, mm = torch.from_numpy(times), torch.from_numpy(meta)
    if V == 2:   # device indices: passed as they are
        tt, mm = tt.to(dev), mm.to(dev)
    cw, x0 = _gather_twice(dev, cond, tgt, tt, mm, csel, *crop, (tuple(exp_c.shape), tuple(exp_x.shape)))
    assert torch.equal(cw, exp_c) and torch.equal(x0, exp_x)


def test_device_indices_are_clamped(dev):
    """the clamping contract: device times / meta are not read back, every index is clamped into its range before an
    address is formed, so an out-of-range one gives the value of the clamped index"""
    V, Cc, Vc, csel = 1, 3, 3, [2, 0, 1]
    cond, tgt = _fields(V, Vc, seed=3)
    Kw, h, w = 3, 6, 8
    times = np.array([[-5, 4, T + 7], [2 ** 40, -2 ** 40, 3]], np.int64)
    meta = np.array([[M + 3, -1, H, -4], [-2, T + 1, -7, W + 100]], np.int64)
    ct = np.clip(times, 0, T - 1)
    cm = np.stack([np.clip(meta[:, 0], 0, M - 1), np.clip(meta[:, 1], 0, T - 1), np.clip(meta[:, 2], 0, H - h),
                   np.clip(meta[:, 3], 0, W - w)], axis=1)
    exp_c, exp_x = _twin(cond, tgt, ct, cm, csel, h, w)
    cw, x0 = _gather_twice(dev, cond, tgt, torch.from_numpy(times).to(dev), torch.from_numpy(meta).to(dev), csel, h, w,
                           (tuple(exp_c.shape), tuple(exp_x.shape)))
    assert torch.isfinite(cw).all() and torch.isfinite(x0).all()
    assert torch.equal(cw, exp_c) and torch.equal(x0, exp_x)
    # the same indices on the host are refused before anything is launched
    dc, dt_ = torch.from_numpy(cond).to(dev), torch.from_numpy(tgt).to(dev)
    with pytest.raises(ValueError, match="window_gather_mc: times"):
        K.window_gather_mc(dc, dt_, torch.from_numpy(times), torch.from_numpy(cm), csel, h, w)
    with pytest.raises(ValueError, match="window_gather_mc: member"):
        K.window_gather_mc(dc, dt_, torch.from_numpy(ct), torch.from_numpy(meta), csel, h, w)


def test_unsupported_shapes_raise_value_error(dev):
    """what the library rejects (CESM_EUNSUPPORTED) reaches the caller as ValueError: asked of the entry point itself"""
    cond = torch.zeros(T, M, 3, H, W, device=dev)
    tgt = torch.zeros(T, M, 1, H, W, device=dev)
    tt, mm = torch.zeros(2, 3, dtype=torch.int64, device=dev), torch.zeros(2, 4, dtype=torch.int64, device=dev)
    out_c, out_x = torch.zeros(2, 4, 3, 6, 8, device=dev), torch.zeros(2, 1, 6, 8, device=dev)

    def call(V=1, Cc=3, Vc=3, csel=(0, 1, 2, 0), Kw=3, h=6, w=8):
        K._mv_call("cesm_window_gather_mc", "probe", K.P(cond), K.P(tgt), K.P(tt), K.P(mm), K.P(out_c), K.P(out_x), 2,
                   Kw, V, Cc, Vc, *csel, T, M, H, W, h, w, K.S())

    call()
    for bad in (dict(V=0), dict(Cc=0), dict(Cc=5), dict(csel=(0, 3, 0, 0)), dict(csel=(-1, 0, 0, 0)), dict(h=H + 1),
                dict(w=W + 1), dict(Kw=0)):
        with pytest.raises(ValueError, match="unsupported"):
            call(**bad)
    torch.cuda.synchronize()


@pytest.mark.parametrize("kind", ["device", "pinned"])
def test_loader_feeds_two_training_steps(dev, kind):
    """(T, M, 4, H, W) forcings, one target, cond_channels=3 with a cond_select: batches are [B, 3, K, h, w], equal to
    the numpy twin on the same draws, and train_one_epoch takes two steps on a UNet(cond_channels=3) with them"""
    shape = (4, 2, 20, 31)
    cond, tgt = _fields(1, 4, shape, seed=11)
    Kw, bs, crop, csel = 3, 2, (16, 24), [3, 1, 0]
    cls = DA.PinnedWindowLoader if kind == "pinned" else DA.DeviceWindowLoader

    def loader():
        return cls(cond, tgt, Kw, bs, dev, crop_hw=crop, time_reverse_p=0.5, seed=0, cond_select=csel, cond_channels=3)

    with pytest.raises(ValueError, match="give cond_select"):
        cls(cond, tgt, Kw, bs, dev, crop_hw=crop, cond_channels=3)
    ld = loader()
    assert ld.csel == csel
    np.random.seed(7)
    got = [(c.clone(), x.clone()) for c, x in ld][:2]
    smp = DA.WindowSampler(*shape, Kw, True, crop, "random", 0.5)
    np.random.seed(7)
    for (c, x), idx in zip(got, DA.shard_indices(len(smp), bs, 0, 1, True, 0, 0)):
        times, meta = smp.draw(idx)
        exp_c, exp_x = _twin(cond, tgt, times, meta, csel, *crop)
        assert c.shape == (bs, 3, Kw, *crop) and x.shape == (bs, 1, *crop)
        assert torch.equal(c.cpu(), exp_c) and torch.equal(x.cpu(), exp_x)

    class TwoBatches:
        def __init__(self, ld):
            self.ld = ld

        def __iter__(self):
            for k, b in enumerate(self.ld):
                if k == 2:
                    return
                yield b

    torch.manual_seed(0)
    net = UNet(out_channels=1, ch_mults=(1, 2), cond_channels=3).to(dev)
    d = Diffusion(net).to(dev)
    d.generator = rank_generator(dev, 2, 0)
    opt = FusedAdamW(d.parameters(), lr=1e-3, max_grad_norm=1.0)
    w0 = net.net.input_conv.weight.detach().clone()
    np.random.seed(7)
    loss = train_one_epoch(d, TwoBatches(loader()), opt, dev, 1.0, use_amp=False)
    torch.cuda.synchronize()
    print(f"{kind}: epoch loss {loss:.6f}")
    assert np.isfinite(loss)
    assert not torch.equal(net.net.input_conv.weight.detach(), w0)
