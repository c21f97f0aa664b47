"""Host side of the weight EMA (cesm_emulator_amd/ema.py): the decay schedule, argument checks that need no GPU,
the "ema" checkpoint entry next to the reference-format keys, and make_ema's config handling."""
import types

import pytest
import torch

from cesm_emulator_amd import checkpoint as CK
from cesm_emulator_amd import kernels as K
from cesm_emulator_amd.ema import EMA, ema_decay
from cesm_emulator_amd.model import UNet, Diffusion
from cesm_emulator_amd.optim import FusedAdamW
from cesm_emulator_amd.train import make_ema
from oracle import ref_cpu as R

CFG = {"unet": {"in_channels": 2, "out_channels": 1, "base_ch": 64, "ch_mults": [1, 2, 4], "groups": 8},
       "train": {"timesteps": 1000, "beta_schedule": "linear"}}


def f32(x):
    return float(torch.tensor(x, dtype=torch.float32).item())


def test_ema_decay_known_answers():
    assert ema_decay(1, 0.9999) == 2.0 / 11.0
    assert ema_decay(90, 0.9999) == 0.91
    assert ema_decay(1, 0.125) == 0.125  # warm-up never raises the decay above beta
    # a large n clamps to beta -- the fp32 beta the kernel is given
    assert ema_decay(10 ** 9, 0.9999) == f32(0.9999)
    assert abs(ema_decay(10 ** 9, 0.9999) - 0.9999) <= 2.0 ** -24
    assert ema_decay(10 ** 9, 0.75) == 0.75
    assert ema_decay(1, 0.9999, warmup=False) == f32(0.9999)
    assert ema_decay(1, 0.5, warmup=False) == 0.5
    # either side of the crossover of the two branches for beta = 0.9999 ((1 + n) / (10 + n) = beta near n = 89980)
    assert ema_decay(80000, 0.9999) == 80001.0 / 80010.0 < f32(0.9999)
    assert ema_decay(100000, 0.9999) == f32(0.9999)
    seq = [ema_decay(n, 0.999) for n in range(1, 2000)]
    assert all(a <= b for a, b in zip(seq, seq[1:])) and seq[-1] < 1.0
    with pytest.raises(ValueError):
        ema_decay(0, 0.9)


@pytest.mark.parametrize("beta", [1.0, 1.5, -0.1, float("nan")])
def test_beta_out_of_range_raises(beta):
    with pytest.raises(ValueError, match="beta"):
        ema_decay(1, beta)
    with pytest.raises(ValueError, match="beta"):
        EMA(None, None, beta=beta)
    t = torch.zeros(4)
    with pytest.raises(ValueError, match="beta"):
        K.adamw_ema(t, t, t, t, torch.zeros(4), 0.0, 0.9, 0.999, 1e-8, 0.0, torch.zeros(1, dtype=torch.int32), False,
                    t, torch.zeros(1, dtype=torch.int32), torch.zeros(1), beta, 0)


def test_cpu_tensors_and_wrong_types_raise():
    t = torch.zeros(4)
    i = torch.zeros(1, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="device tensors"):
        K.adamw_ema(t, t, t, t, torch.zeros(4), 0.0, 0.9, 0.999, 1e-8, 0.0, i, False, t, i, torch.zeros(1), 0.5, 0)
    with pytest.raises(TypeError):
        K.adamw_ema(t, t, t, t, torch.zeros(4), 0.0, 0.9, 0.999, 1e-8, 0.0, i, False, None, i, torch.zeros(1), 0.5, 0)
    net = UNet(ch_mults=(1, 2))
    with pytest.raises(RuntimeError, match="GPU"):
        FusedAdamW(net.parameters())  # a CPU model never gets as far as an EMA
    with pytest.raises(TypeError):
        EMA(net, torch.optim.AdamW(net.parameters()))
    with pytest.raises(TypeError):
        EMA(torch.nn.Linear(2, 2), None)


def _host_optimizer(params):
    """a FusedAdamW as far as EMA's checks look at it, without the GPU its constructor needs"""
    params = [p for p in params if p.requires_grad]
    opt = object.__new__(FusedAdamW)
    opt.flat = types.SimpleNamespace(params=params, offsets=[0] * len(params), data=torch.zeros(1))
    opt.ema = None
    return opt


def test_optimizer_over_other_parameters_raises():
    net, other = UNet(ch_mults=(1, 2)), UNet(ch_mults=(1, 2))
    with pytest.raises(ValueError, match="trainable parameters"):
        EMA(net, _host_optimizer(other.parameters()))
    with pytest.raises(ValueError, match="trainable parameters"):
        EMA(net, _host_optimizer(list(net.parameters())[:-1]))
    opt = _host_optimizer(net.parameters())
    with pytest.raises(RuntimeError, match="GPU"):  # the right parameters, on the CPU
        EMA(net, opt)
    assert opt.ema is None


def test_make_ema_is_off_by_default():
    assert make_ema(None, None, {}) is None
    assert make_ema(None, None, {"optimizer": {"lr": 1e-4}, "ema": False}) is None
    assert make_ema(None, None, {"ema": None}) is None
    import os
    from cesm_emulator_amd.config import apply_overrides, load_config
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for name in ("baseline", "more_blocks"):
        cfg = load_config(os.path.join(root, "config", name))
        assert make_ema(None, None, cfg["train"]) is None
        apply_overrides(cfg, ["train.ema.beta=0.999", "train.ema.warmup=false"])  # how the setting arrives
        assert cfg["train"]["ema"] == {"beta": 0.999, "warmup": False}
        apply_overrides(cfg, ["train.ema=true"])
        assert cfg["train"]["ema"] is True
    with pytest.raises(TypeError):
        make_ema(None, None, {"ema": 0.999})
    with pytest.raises(ValueError, match="unknown"):
        make_ema(None, None, {"ema": {"decay": 0.999}})


class _StubEMA:
    """what save_checkpoint needs of an EMA: a state_dict() in EMA.state_dict()'s layout"""

    def __init__(self, model_sd):
        self.sd = {"model": {k: v.detach().clone() + 1.0 for k, v in model_sd.items()}, "beta": 0.9999,
                   "warmup": True, "num_updates": 17}

    def state_dict(self):
        return self.sd


def test_ema_entry_does_not_disturb_reference_format_readers(tmp_path):
    torch.manual_seed(5)
    diff = Diffusion(UNet(ch_mults=(1, 2, 4)))
    stub = _StubEMA(diff.model.state_dict())
    path = tmp_path / "with_ema.pt"
    CK.save_checkpoint(path, diff, None, 2, CFG, ema=stub)
    ck = torch.load(path, weights_only=True)
    assert set(ck) == {"epoch", "model", "diffusion_buffers", "optimizer", "config", "ema"}
    assert ck["ema"]["num_updates"] == 17 and ck["ema"]["beta"] == 0.9999 and ck["ema"]["warmup"] is True
    # the reference's reader (train.py:915-946 / tests/test_checkpoint.py): ckpt["model"] strict, buffers by .get
    torch.manual_seed(6)
    ref = R.Diffusion(R.UNet(ch_mults=(1, 2, 4)))
    ref.model.load_state_dict(ck["model"], strict=True)
    st = ref.state_dict()
    st.update(ck.get("diffusion_buffers", {}))
    ref.load_state_dict(st, strict=True)
    for (k, a), (_, b) in zip(diff.state_dict().items(), ref.state_dict().items()):
        assert torch.equal(a, b), k
    # this package's readers: the raw weights by default, the EMA's on request, both ignoring the other
    torch.manual_seed(7)
    unet = UNet(ch_mults=(1, 2, 4))
    assert CK.load_checkpoint(path, unet, Diffusion(unet), None, device="cpu") == 3
    for k, a in unet.state_dict().items():
        assert torch.equal(a, ck["model"][k]), k
    d_raw, cfg = CK.load_diffusion_from_checkpoint(path, device="cpu")
    d_ema, _ = CK.load_diffusion_from_checkpoint(path, device="cpu", use_ema=True)
    assert cfg == CFG
    for k, a in d_raw.model.state_dict().items():
        assert torch.equal(a, ck["model"][k]) and torch.equal(d_ema.model.state_dict()[k], ck["ema"]["model"][k]), k
    plain = tmp_path / "plain.pt"
    CK.save_checkpoint(plain, diff, None, 2, CFG)
    assert "ema" not in torch.load(plain, weights_only=True)
    with pytest.raises(KeyError, match="plain.pt"):
        CK.load_diffusion_from_checkpoint(plain, device="cpu", use_ema=True)
