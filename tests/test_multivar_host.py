"""Several target variables, host side (no GPU): UNet(out_channels=V) constructs like the reference for 1 <= V <= 4,
refuses more, and the FLOP count follows V."""
import pytest
import torch

from cesm_emulator_amd import flops
from cesm_emulator_amd.model import UNet
from oracle import ref_cpu as R


@pytest.mark.parametrize("V", [2, 4])
def test_state_dict_matches_oracle(V):
    """same seed -> the oracle's keys in order, shapes and values"""
    torch.manual_seed(3)
    ref = R.UNet(out_channels=V, ch_mults=(1, 2, 4))
    torch.manual_seed(3)
    prod = UNet(out_channels=V, ch_mults=(1, 2, 4))
    sr, sp = ref.state_dict(), prod.state_dict()
    assert list(sr.keys()) == list(sp.keys())
    for k in sr:
        assert sr[k].shape == sp[k].shape and torch.equal(sr[k], sp[k]), k
    assert sp["net.input_conv.weight"].shape == (64, 2 * V, 1, 7, 7)
    assert sp["net.out_conv.1.weight"].shape == (V, 64, 1, 1, 1)
    assert sp["net.out_conv.1.bias"].shape == (V,)
    prod.load_state_dict(sr, strict=True)


def test_more_than_four_variables_refused():
    with pytest.raises(NotImplementedError, match="4"):
        UNet(out_channels=5)
    with pytest.raises(NotImplementedError):
        UNet(out_channels=0)
    # the other refused configurations stay refused
    with pytest.raises(NotImplementedError):
        UNet(out_channels=2, use_mid_attn=True)
    with pytest.raises(NotImplementedError):
        UNet(out_channels=2, day_cond=True)


def test_flops_stem_and_head_scale_with_v():
    F, H, W = 3, 16, 24
    nets = {V: UNet(out_channels=V, ch_mults=(1, 2, 4)).net for V in (1, 2, 3)}
    total = {V: flops.unet_forward_macs(n, F, H, W) for V, n in nets.items()}
    for V, n in nets.items():
        stem, head = flops.stem_head_macs(n, F, H, W)
        assert stem == F * H * W * 64 * 2 * V * 49
        assert head == F * H * W * 64 * V
        # nothing else in the network depends on V
        assert total[V] - total[1] == (V - 1) * F * H * W * (64 * 2 * 49 + 64)
    # the oracle's module tree counts the same
    assert flops.unet_forward_macs(R.UNet(out_channels=2, ch_mults=(1, 2, 4)).net, F, H, W) == total[2]


def test_checkpoint_round_trip_two_variables(tmp_path):
    """a V = 2 checkpoint: the reference's trained state loads into the drop-in built from the file's config, and the
    drop-in's own checkpoint loads back: same keys, shapes, bit-equal tensors"""
    from cesm_emulator_amd import checkpoint as CK
    from cesm_emulator_amd.model import Diffusion
    cfg = {"unet": {"in_channels": 4, "out_channels": 2, "base_ch": 64, "ch_mults": [1, 2, 4], "groups": 8},
           "train": {"timesteps": 1000, "beta_schedule": "linear"}}
    torch.manual_seed(3)
    ref = R.Diffusion(R.UNet(out_channels=2, ch_mults=(1, 2, 4)))
    path = tmp_path / "ref_v2.pt"
    CK.save_checkpoint(path, ref, None, 4, cfg)
    d, got_cfg = CK.load_diffusion_from_checkpoint(path, device="cpu")
    assert got_cfg == cfg and d.model.net.n_vars == 2
    for (k, a), (k2, b) in zip(ref.state_dict().items(), d.state_dict().items()):
        assert k == k2 and a.shape == b.shape and torch.equal(a, b), k
    path2 = tmp_path / "ours_v2.pt"
    CK.save_checkpoint(path2, d, None, 5, cfg)
    torch.manual_seed(9)
    unet = UNet(out_channels=2, ch_mults=(1, 2, 4))
    diff = Diffusion(unet)
    assert CK.load_checkpoint(path2, unet, diff, None, device="cpu") == 6
    assert list(diff.state_dict().keys()) == list(ref.state_dict().keys())
    for (k, a), (_, b) in zip(ref.state_dict().items(), diff.state_dict().items()):
        assert a.shape == b.shape and torch.equal(a, b), k


def test_channel_mismatch_message_names_both():
    """the shape check runs before the device check, so it is testable without a GPU"""
    m = UNet(out_channels=2, ch_mults=(1, 2, 4))
    with pytest.raises(ValueError, match=r"x_t has 2 channels and cond 1"):
        m(torch.zeros(1, 2, 8, 8), torch.zeros(1, 1, 8, 8), torch.zeros(1, dtype=torch.long))
