"""Multi-forcing conditioning, host side (no GPU): UNet(cond_channels=Cc) builds the reference's module tree with a
Conv3d(V + Cc -> 64) stem, refuses Cc outside 1 .. 4, the FLOP count follows V + Cc, the config key is read, and the
data path's argument rules and numpy gather take Cc cond planes."""
import numpy as np
import pytest
import torch

from cesm_emulator_amd import data as D
from cesm_emulator_amd import flops
from cesm_emulator_amd.model import UNet
from cesm_emulator_amd.train import build_model_from_config
from oracle import ref_cpu as R


@pytest.mark.parametrize("V,Cc", [(1, 3), (2, 3), (4, 1)])
def test_state_dict_keys_are_the_oracles(V, Cc):
    ref = R.UNet(out_channels=V, ch_mults=(1, 2, 4)).state_dict()
    prod = UNet(out_channels=V, ch_mults=(1, 2, 4), cond_channels=Cc)
    sp = prod.state_dict()
    assert list(ref.keys()) == list(sp.keys())
    for k in ref:
        if k != "net.input_conv.weight":
            assert ref[k].shape == sp[k].shape, k
    assert sp["net.input_conv.weight"].shape == (64, V + Cc, 1, 7, 7)
    assert prod.net.n_vars == V and prod.net.n_cond == Cc
    assert prod.ctor_kwargs["cond_channels"] == Cc
    twin = UNet(**prod.ctor_kwargs)   # what ema.EMA builds
    assert twin.state_dict()["net.input_conv.weight"].shape == (64, V + Cc, 1, 7, 7)


def test_refusals_and_default():
    for bad in (0, 5):
        with pytest.raises(NotImplementedError, match="4"):
            UNet(out_channels=2, cond_channels=bad)
    torch.manual_seed(5)
    a = UNet(out_channels=2, ch_mults=(1, 2, 4)).state_dict()
    torch.manual_seed(5)
    b = UNet(out_channels=2, ch_mults=(1, 2, 4), cond_channels=None).state_dict()
    torch.manual_seed(5)
    c = UNet(out_channels=2, ch_mults=(1, 2, 4), cond_channels=2).state_dict()
    assert list(a.keys()) == list(b.keys()) == list(c.keys())
    for k in a:
        assert torch.equal(a[k], b[k]) and torch.equal(a[k], c[k]), k


def test_channel_mismatch_message_names_both_counts():
    m = UNet(out_channels=1, ch_mults=(1, 2, 4), cond_channels=3)
    with pytest.raises(ValueError, match=r"1 target variable\(s\) and 3 conditioning map\(s\).*cond 1"):
        m(torch.zeros(1, 1, 8, 8), torch.zeros(1, 1, 8, 8), torch.zeros(1, dtype=torch.long))


def test_flops_stem_follows_v_plus_cc():
    F, H, W = 3, 16, 24
    base = UNet(out_channels=1, ch_mults=(1, 2, 4)).net
    for V, Cc in ((1, 3), (2, 3), (3, 1)):
        n = UNet(out_channels=V, ch_mults=(1, 2, 4), cond_channels=Cc).net
        stem, head = flops.stem_head_macs(n, F, H, W)
        assert stem == F * H * W * 64 * (V + Cc) * 49
        assert head == F * H * W * 64 * V
        # nothing else in the network depends on V or Cc
        assert (flops.unet_forward_macs(n, F, H, W) - flops.unet_forward_macs(base, F, H, W) ==
                F * H * W * (64 * (V + Cc - 2) * 49 + 64 * (V - 1)))


def test_build_model_from_config_reads_the_key():
    cfg = {"out_channels": 1, "ch_mults": [1, 2, 4], "cond_channels": 3}
    m = build_model_from_config(cfg)
    assert m.net.n_cond == 3 and m.net.input_conv.weight.shape[1] == 4
    del cfg["cond_channels"]
    assert build_model_from_config(cfg).net.n_cond == 1


def test_checkpoint_round_trip(tmp_path):
    """save -> load_diffusion_from_checkpoint rebuilds the Cc-channel stem from the file's config"""
    from cesm_emulator_amd import checkpoint as CK
    from cesm_emulator_amd.model import Diffusion
    cfg = {"unet": {"out_channels": 1, "base_ch": 64, "ch_mults": [1, 2, 4], "groups": 8, "cond_channels": 3},
           "train": {"timesteps": 1000, "beta_schedule": "linear"}}
    torch.manual_seed(3)
    diff = Diffusion(UNet(out_channels=1, ch_mults=(1, 2, 4), cond_channels=3))
    path = tmp_path / "mc.pt"
    CK.save_checkpoint(path, diff, None, 4, cfg)
    d, got = CK.load_diffusion_from_checkpoint(path, device="cpu")
    assert got == cfg and d.model.net.n_cond == 3 and d.model.net.n_vars == 1
    for (k, a), (k2, b) in zip(diff.state_dict().items(), d.state_dict().items()):
        assert k == k2 and a.shape == b.shape and torch.equal(a, b), k


def test_resolve_cond_select_rules():
    r = D.resolve_cond_select
    # None: today's rule, exactly
    assert r(None, 2, 2) == [0, 1] and r(None, 1, 2) == [0, 0] and r([1, 0], 3, 2) == [1, 0]
    assert r(None, 2, 2, None) == [0, 1]
    with pytest.raises(ValueError, match="give cond_select"):
        r(None, 3, 2)
    with pytest.raises(ValueError, match=r"one index per target variable \(2\)"):
        r([0, 1, 2], 3, 2)
    with pytest.raises(ValueError, match=r"cond_select = 3 outside \[0, 2\]"):
        r([0, 3], 3, 2)
    # Cc given: Cc indices into the Vc forcings, identity when Vc == Cc
    assert r(None, 3, 1, 3) == [0, 1, 2]
    assert r([2, 0, 3], 4, 2, 3) == [2, 0, 3]
    assert r([0, 0], 1, 1, 2) == [0, 0]
    with pytest.raises(ValueError, match="give cond_select"):
        r(None, 4, 1, 3)
    with pytest.raises(ValueError, match=r"one index per conditioning map \(3\)"):
        r([0, 1], 3, 1, 3)
    with pytest.raises(ValueError, match=r"cond_select = 4 outside \[0, 3\]"):
        r([0, 1, 4], 4, 2, 3)
    for bad in (0, 5, True, 2.0):
        with pytest.raises(ValueError, match="cond_channels"):
            r(None, 2, 2, bad)


@pytest.mark.parametrize("V,Cc,Vc,csel", [(1, 3, 3, [0, 1, 2]), (2, 3, 4, [3, 0, 2]), (1, 2, 2, [1, 1])])
def test_host_gather_with_separate_counts(V, Cc, Vc, csel):
    """the numpy twin against plain slicing"""
    T, M, H, W, K, h, w, n = 9, 2, 12, 16, 3, 5, 7, 4
    rng = np.random.default_rng(V * 10 + Cc)
    cond = rng.standard_normal((T, M, Vc, H, W)).astype(np.float32)
    tgt = rng.standard_normal((T, M, V, H, W)).astype(np.float32)
    times = rng.integers(0, T, size=(n, K))
    meta = np.stack([rng.integers(0, M, n), rng.integers(0, T, n), rng.integers(0, H - h + 1, n),
                     rng.integers(0, W - w + 1, n)], axis=1)
    oc = np.full((n, Cc, K, h, w), np.nan, np.float32)
    ox = np.full((n, V, h, w), np.nan, np.float32)
    D.host_gather_mv(cond, tgt, times, meta, csel, h, w, oc, ox)
    for i in range(n):
        m, a, ci, cj = meta[i]
        for c in range(Cc):
            for k in range(K):
                assert np.array_equal(oc[i, c, k], cond[times[i, k], m, csel[c], ci:ci + h, cj:cj + w])
        assert np.array_equal(ox[i], tgt[a, m, :, ci:ci + h, cj:cj + w])
    with pytest.raises(ValueError, match="planes"):   # buffers of the V-channel layout
        D.host_gather_mv(cond, tgt, times, meta, csel, h, w, np.zeros((n, Cc + 1, K, h, w), np.float32), ox)


def test_gather_wrapper_checks_before_launch():
    """kernels.window_gather_mc raises on bad arguments and on out-of-range host indices before the library is
    touched"""
    from cesm_emulator_amd import kernels as K
    T, M, H, W = 5, 2, 8, 8
    cond, tgt = torch.zeros(T, M, 3, H, W), torch.zeros(T, M, 1, H, W)
    times, meta = torch.zeros(2, 3, dtype=torch.long), torch.zeros(2, 4, dtype=torch.long)
    with pytest.raises(ValueError, match="csel = 3"):
        K.window_gather_mc(cond, tgt, times, meta, [0, 3], 4, 4)
    with pytest.raises(ValueError, match="unsupported shape"):
        K.window_gather_mc(cond, tgt, times, meta, [0] * 5, 4, 4)
    bad = times.clone()
    bad[1, 2] = T
    with pytest.raises(ValueError, match=r"window_gather_mc: times = 5 outside \[0, 4\]"):
        K.window_gather_mc(cond, tgt, bad, meta, [0, 1, 2], 4, 4)
