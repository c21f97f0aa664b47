"""UNet(use_temp_attn=False), host side (no GPU): construction, key lists against the oracle network with the blocks
swapped (tests/tconv_ref.py), initialisation, refused configurations, the config surface, the FLOP count and a
checkpoint round trip."""
import pytest
import torch

from cesm_emulator_amd import flops
from cesm_emulator_amd.model import UNet, Diffusion
from cesm_emulator_amd.train import build_model_from_config
from tests.tconv_ref import swapped_oracle, randomize_tconv, expected_tconv_keys

KEYS = {
    (1, 2, 4): ["net.input_temp_op"],
    (1, 2, 4, 8): ["net.input_temp_op", "net.downs.0.3", "net.ups.3.3"],
    (1, 2, 4, 8, 8): ["net.input_temp_op", "net.downs.0.3", "net.downs.1.3", "net.ups.3.3", "net.ups.4.3"],
}


@pytest.mark.parametrize("mults", sorted(KEYS))
def test_constructs_with_the_oracle_keys(mults):
    prod = UNet(use_temp_attn=False, ch_mults=mults)
    ref = swapped_oracle(mults)
    sp, sr = prod.state_dict(), ref.state_dict()
    assert list(sp.keys()) == list(sr.keys())
    for k in sr:
        assert sp[k].shape == sr[k].shape, k
    got = sorted(k.rsplit(".fn.fn.temporal_conv.", 1)[0] for k in sp if k.endswith("temporal_conv.weight"))
    assert got == sorted(KEYS[mults]) == sorted(expected_tconv_keys(mults))
    for pre in got:
        assert f"{pre}.fn.fn.temporal_conv.bias" in sp and f"{pre}.fn.norm.gamma" in sp
        assert not any(k.startswith(pre + ".") and "to_qkv" in k for k in sp)
    # the three deepest levels and the bottleneck keep attention
    assert "net.mid_temporal_attn.fn.fn.fn.to_qkv.weight" in sp
    assert f"net.downs.{len(mults) - 1}.3.fn.fn.fn.to_qkv.weight" in sp and "net.ups.0.3.fn.fn.fn.to_qkv.weight" in sp
    if mults == (1, 2, 4, 8, 8):
        assert sp["net.downs.1.3.fn.fn.temporal_conv.weight"].shape == (128, 128, 3)
        assert sp["net.ups.4.3.fn.fn.temporal_conv.weight"].shape == (64, 64, 3)
    prod.load_state_dict(sr, strict=True)


def test_default_is_unchanged():
    """use_temp_attn=True (the default) builds the attention network with the same RNG draws as before"""
    torch.manual_seed(3)
    a = UNet(ch_mults=(1, 2, 4))
    torch.manual_seed(3)
    b = UNet(ch_mults=(1, 2, 4), use_temp_attn=True)
    assert not any("temporal_conv" in k for k in a.state_dict())
    for (k, u), (k2, v) in zip(a.state_dict().items(), b.state_dict().items()):
        assert k == k2 and torch.equal(u, v)


def test_rng_draws_follow_the_reference_order():
    """the reference's draws up to the time MLP, replayed by hand: stem Conv3d, the rel-pos table ONCE, the input
    op's Conv1d (drawn, then overwritten with the identity), then the first Linear of the time MLP"""
    import torch.nn as nn
    torch.manual_seed(5)
    sd = UNet(use_temp_attn=False, ch_mults=(1, 2, 4)).state_dict()
    torch.manual_seed(5)
    stem = nn.Conv3d(2, 64, (1, 7, 7), padding=(0, 3, 3))
    table = nn.Embedding(32, 8)
    nn.Conv1d(64, 64, 3, padding=1)
    lin = nn.Linear(64, 256)
    assert torch.equal(sd["net.input_conv.weight"], stem.weight)
    assert torch.equal(sd["net.time_rel_pos_bias.relative_attention_bias.weight"], table.weight)
    assert torch.equal(sd["net.time_mlp.1.weight"], lin.weight) and torch.equal(sd["net.time_mlp.1.bias"], lin.bias)


def test_dirac_and_zero_init():
    sd = UNet(use_temp_attn=False, ch_mults=(1, 2, 4, 8)).state_dict()
    for pre in KEYS[(1, 2, 4, 8)]:
        w, b = sd[f"{pre}.fn.fn.temporal_conv.weight"], sd[f"{pre}.fn.fn.temporal_conv.bias"]
        assert w.shape == (64, 64, 3) and b.shape == (64,)
        assert torch.equal(w[:, :, 1], torch.eye(64)) and not w[:, :, 0].any() and not w[:, :, 2].any()
        assert not b.any()


def test_unsupported_width_refused():
    with pytest.raises(NotImplementedError, match="64, 128, 256"):
        UNet(use_temp_attn=False, base_ch=96, ch_mults=(1, 2, 4))
    with pytest.raises(NotImplementedError, match="64, 128, 256"):
        UNet(use_temp_attn=False, base_ch=32, ch_mults=(1, 2, 4))


def test_other_refused_configurations_stay_refused():
    for kw in ({"use_mid_attn": True}, {"day_cond": True}, {"year_cond": True}, {"cond_map": False}):
        with pytest.raises(NotImplementedError):
            UNet(use_temp_attn=False, **kw)
        with pytest.raises(NotImplementedError):
            UNet(**kw)


def test_build_model_from_config():
    m = build_model_from_config({"use_temp_attn": False, "ch_mults": [1, 2, 4, 8], "base_ch": 64})
    assert sorted(k.rsplit(".fn.fn.temporal_conv.", 1)[0] for k in m.state_dict()
                  if k.endswith("temporal_conv.weight")) == sorted(KEYS[(1, 2, 4, 8)])
    assert m.ctor_kwargs["use_temp_attn"] is False
    d = build_model_from_config({"ch_mults": [1, 2, 4, 8], "base_ch": 64})
    assert not any("temporal_conv" in k for k in d.state_dict()) and d.ctor_kwargs["use_temp_attn"] is True


def test_flops_count():
    F, H, W = 3, 16, 24
    mults = (1, 2, 4, 8)
    attn = flops.unet_forward_macs(UNet(ch_mults=mults).net, F, H, W)
    conv = flops.unet_forward_macs(UNet(use_temp_attn=False, ch_mults=mults).net, F, H, W)
    v = 3 * 16 * 24  # voxels of a full-resolution block; the three replaced blocks are all C = 64
    attn_block = v * (768 * 64 + 256 * 64) + v * 8 * 2 * 3 * 32
    conv_block = v * 3 * 64 * 64
    assert conv == attn - 3 * attn_block + 3 * conv_block
    # the swapped oracle's module tree counts the same
    assert flops.unet_forward_macs(swapped_oracle(mults).net, F, H, W) == conv


def test_checkpoint_round_trip(tmp_path):
    from cesm_emulator_amd import checkpoint as CK
    cfg = {"unet": {"in_channels": 2, "out_channels": 1, "base_ch": 64, "ch_mults": [1, 2, 4, 8], "groups": 8,
                    "use_temp_attn": False},
           "train": {"timesteps": 1000, "beta_schedule": "linear"}}
    torch.manual_seed(3)
    src = Diffusion(randomize_tconv(UNet(use_temp_attn=False, ch_mults=(1, 2, 4, 8))))
    path = tmp_path / "tconv.pt"
    CK.save_checkpoint(path, src, None, 4, cfg)
    d, got_cfg = CK.load_diffusion_from_checkpoint(path, device="cpu")
    assert got_cfg == cfg
    assert list(d.state_dict().keys()) == list(src.state_dict().keys())
    for (k, a), (_, b) in zip(src.state_dict().items(), d.state_dict().items()):
        assert a.shape == b.shape and torch.equal(a, b), k
    torch.manual_seed(9)
    unet = UNet(use_temp_attn=False, ch_mults=(1, 2, 4, 8))
    diff = Diffusion(unet)
    assert CK.load_checkpoint(path, unet, diff, None, device="cpu") == 5
    for (k, a), (_, b) in zip(src.state_dict().items(), diff.state_dict().items()):
        assert torch.equal(a, b), k
    # the state dict alone round-trips strictly, and does not fit the attention variant
    sd = torch.load(path, weights_only=True)["model"]
    UNet(use_temp_attn=False, ch_mults=(1, 2, 4, 8)).load_state_dict(sd, strict=True)
    with pytest.raises(RuntimeError, match="temporal_conv"):
        UNet(ch_mults=(1, 2, 4, 8)).load_state_dict(sd, strict=True)
