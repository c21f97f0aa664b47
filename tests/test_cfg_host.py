"""Host side of classifier-free guidance (no GPU): the range checks of `p_uncond` and `guidance_scale` (each raises
before any kernel is called), the `guidance` block of the training config and its way through a checkpoint, the
unchanged checkpoint keys, and train_step's `keep=` pass-through."""
import inspect

import pytest
import torch

import cesm_emulator_amd as PKG
from cesm_emulator_amd import _lib, kernels as K, saliency, train as TR
from cesm_emulator_amd.checkpoint import load_diffusion_from_checkpoint
from cesm_emulator_amd.model import Diffusion, GraphSampleStep, UNet, check_guidance_scale
from cesm_emulator_amd.train import make_diffusion

BAD = [-0.5, -1e-9, float("nan"), float("inf"), float("-inf"), True, False, "2", None]
SHAPE = (2, 1, 4, 4)


def _diff(**kw):
    return Diffusion(torch.nn.Identity(), timesteps=10, **kw)


@pytest.fixture
def no_kernels(monkeypatch):
    """any library call fails the test: the checks under test come before the first one"""
    def boom(name, *a):
        raise AssertionError(f"{name} called before the argument check")
    for mod in (_lib, K):
        monkeypatch.setattr(mod, "call", boom)
    monkeypatch.setattr(_lib, "lib", lambda: boom("lib()"))


# ---------------------------------------------------------------------------------------------------- p_uncond
@pytest.mark.parametrize("p", [-0.1, 1.5, float("nan"), float("inf"), True, False, "0.1", None])
def test_p_uncond_out_of_range_raises(p):
    with pytest.raises(ValueError, match="p_uncond"):
        _diff(p_uncond=p)


def test_p_uncond_is_a_plain_attribute_and_the_checkpoint_keys_stay():
    keys = set(_diff().state_dict())
    assert len(keys) == 8
    for p in (0.0, 0.1, 1, 1.0):
        d = _diff(p_uncond=p)
        assert d.p_uncond == float(p) and isinstance(d.p_uncond, float)
        assert set(d.state_dict()) == keys
        assert "p_uncond" not in dict(d.named_buffers()) and "p_uncond" not in dict(d.named_parameters())
    assert _diff().p_uncond == 0.0
    assert inspect.signature(Diffusion.__init__).parameters["p_uncond"].default == 0.0


# ------------------------------------------------------------------------------------------------ guidance_scale
def test_guidance_scale_values():
    assert check_guidance_scale(None) is None
    assert check_guidance_scale(1.0) is None and check_guidance_scale(1) is None  # exactly 1: the unguided path
    for s in (0, 0.0, 0.3, 2, 7.5):
        got = check_guidance_scale(s)
        assert isinstance(got, float) and got == float(s)
    assert K.guidance_scale_arg(1.0) == 1.0  # the kernels themselves take 1 like any other scale


@pytest.mark.parametrize("s", BAD[:-1])
def test_guidance_scale_out_of_range_raises_before_any_kernel(no_kernels, s):
    d = _diff()
    cond, x = torch.zeros(SHAPE), torch.zeros(SHAPE)
    t = torch.tensor([5, 5])
    with pytest.raises(ValueError, match="guidance_scale"):
        check_guidance_scale(s)
    for use_graph in (False, True):
        for kw in ({}, {"steps": 3}, {"steps": 3, "ddim_eta": 0.5}, {"steps": 3, "solver": "dpmpp2m"}):
            with pytest.raises(ValueError, match="guidance_scale"):
                d.sample(cond, SHAPE, "cpu", use_graph=use_graph, guidance_scale=s, **kw)
            with pytest.raises(ValueError, match="guidance_scale"):
                d.sample_ensemble(cond, 2, steps=kw.get("steps"), use_graph=use_graph, guidance_scale=s)
    with pytest.raises(ValueError, match="guidance_scale"):
        d.p_sample(x, cond, t, guidance_scale=s)
    with pytest.raises(ValueError, match="guidance_scale"):
        d.ddim_step(x, cond, t, t - 2, guidance_scale=s)
    with pytest.raises(ValueError, match="guidance_scale"):
        d.dpmpp_step(x, cond, t, t - 2, t * 0 - 1, guidance_scale=s)
    with pytest.raises(ValueError, match="guidance_scale"):
        GraphSampleStep(d, cond, x, guidance_scale=s)
    with pytest.raises(ValueError, match="guidance_scale"):
        saliency.counterfactual_delta(d, cond, steps=3, guidance_scale=s)
    with pytest.raises(ValueError, match="guidance_scale"):
        saliency.counterfactual_delta(d, cond, steps=3, paired=True, guidance_scale=s)
    with pytest.raises(ValueError, match="guidance_scale"):
        TR.validate_ensemble(d, [(cond, x)], 2, steps=3, guidance_scale=s)


@pytest.mark.parametrize("s", BAD)
def test_kernel_bindings_reject_the_scale_before_the_call(no_kernels, s):
    x2, x = torch.zeros(4, 1, 4, 4), torch.zeros(SHAPE)
    t = torch.tensor([5, 5])
    tab = torch.ones(10)
    with pytest.raises(ValueError, match="scale"):
        K.ddpm_step_cfg(x2, x2, x, t, tab, tab, tab, tab, s)
    with pytest.raises(ValueError, match="scale"):
        K.ddim_step_cfg(x2, x2, x, t, t - 1, tab, 0.0, s)
    with pytest.raises(ValueError, match="scale"):
        K.dpmpp_step_cfg(x2, x2, x, t, t - 1, t * 0 - 1, tab, s)


def test_every_sampler_entry_takes_guidance_scale_and_the_old_kernels_do_not():
    for fn in (Diffusion.p_sample, Diffusion.ddim_step, Diffusion.dpmpp_step, Diffusion.sample,
               Diffusion.sample_ensemble, Diffusion._sample, Diffusion._sample_ensemble, GraphSampleStep.__init__,
               TR.validate_ensemble, saliency.counterfactual_delta, PKG.counterfactual_delta):
        assert inspect.signature(fn).parameters["guidance_scale"].default is None, fn
    for fn in (Diffusion._eps, Diffusion.loss, Diffusion.loss_components, TR.train_step, saliency.input_grads,
               saliency.saliency_wrt_cond):
        assert inspect.signature(fn).parameters["keep"].default is None, fn
    # the unguided bindings keep their parameter lists (bench.py's probe wraps them)
    assert list(inspect.signature(K.ddpm_step).parameters) == ["x", "eps", "z", "t", "sra", "betas", "s1a", "pv", "out"]
    assert list(inspect.signature(K.ddim_step).parameters) == ["x", "eps", "z", "t", "t_prev", "alphas_cumprod", "eta",
                                                               "out"]
    assert list(inspect.signature(K.dpmpp_step).parameters) == ["x", "eps", "x0_last", "t", "t_prev", "t_last",
                                                                "alphas_cumprod", "out", "x0_out"]
    for name in ("cond_mask", "ddpm_step_cfg", "ddim_step_cfg", "dpmpp_step_cfg"):
        assert callable(getattr(K, name))
        assert "cesm_" + name in _lib.parse_header()


# ------------------------------------------------------------------------------------------------ training config
def test_make_diffusion_reads_the_guidance_block():
    net = torch.nn.Identity()
    assert make_diffusion(net, {"timesteps": 20}).p_uncond == 0.0
    assert make_diffusion(net, {"guidance": {}}).p_uncond == 0.0
    assert make_diffusion(net, {"guidance": None}).p_uncond == 0.0
    d = make_diffusion(net, {"timesteps": 20, "guidance": {"p_uncond": 0.15}, "loss": {"lat_weight": 0.5}})
    assert d.p_uncond == 0.15 and d.lat_weight == 0.5 and d.T == 20
    with pytest.raises(ValueError, match="unknown keys"):
        make_diffusion(net, {"guidance": {"p_uncond": 0.1, "scale": 2.0}})
    with pytest.raises(ValueError, match="unknown keys"):
        make_diffusion(net, {"guidance": {"p": 0.1}})
    with pytest.raises(TypeError, match="train.guidance"):
        make_diffusion(net, {"guidance": [0.1]})
    with pytest.raises(TypeError, match="train.guidance"):
        make_diffusion(net, {"guidance": 0.1})
    with pytest.raises(ValueError, match="p_uncond"):
        make_diffusion(net, {"guidance": {"p_uncond": 1.5}})


@pytest.mark.parametrize("name", ["baseline", "more_blocks"])
def test_shipped_configs_do_not_set_guidance_until_overridden(name):
    import os
    from cesm_emulator_amd import config as C
    cfg = C.load_config(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "config", name))
    assert "guidance" not in cfg["train"]
    assert make_diffusion(torch.nn.Identity(), cfg["train"]).p_uncond == 0.0
    C.apply_overrides(cfg, ["train.guidance.p_uncond=0.1"])
    assert make_diffusion(torch.nn.Identity(), cfg["train"]).p_uncond == 0.1


def test_checkpoint_config_rebuilds_p_uncond(tmp_path):
    unet_cfg = {"ch_mults": (1, 2), "base_ch": 32}
    net = UNet(ch_mults=(1, 2), base_ch=32)
    for guidance, want in (({"p_uncond": 0.2}, 0.2), (None, 0.0)):
        train_cfg = {"timesteps": 10}
        if guidance is not None:
            train_cfg["guidance"] = guidance
        path = tmp_path / "c.pt"
        torch.save({"model": net.state_dict(), "config": {"unet": unet_cfg, "train": train_cfg}, "epoch": 1}, path)
        d, cfg = load_diffusion_from_checkpoint(str(path), device="cpu")
        assert d.p_uncond == want and not d.training
        assert len(d.state_dict()) - len(d.model.state_dict()) == 8
    torch.save({"model": net.state_dict(), "config": {"unet": unet_cfg, "train": {"guidance": {"drop": 0.2}}}}, path)
    with pytest.raises(ValueError, match="unknown keys"):
        load_diffusion_from_checkpoint(str(path), device="cpu")


# ------------------------------------------------------------------------------------------------ train_step
def test_train_step_passes_keep_through():
    seen = []

    class Opt:
        flat = None
        max_grad_norm = None

        def zero_grad(self, set_to_none=True):
            pass

        def step(self, loss=None):
            pass

    class D:
        weighted = False

        class model:
            net = None

        def loss(self, x0, cond, t=None, noise=None, row0=None, keep=None):
            seen.append(("loss", keep))
            return torch.zeros((), requires_grad=True)

        def loss_components(self, x0, cond, t=None, noise=None, row0=None, keep=None):
            seen.append(("components", keep))
            z = torch.zeros((), requires_grad=True)
            return {"mse_raw": z.detach(), "mse_lat": z.detach(), "cond_loss": z.detach(), "total": z}

    keep = torch.tensor([True, False])
    d = D()
    TR.train_step(d, Opt(), None, None, keep=keep)
    TR.train_step(d, Opt(), None, None, keep=keep, return_components=True)
    d.weighted = True
    TR.train_step(d, Opt(), None, None, keep=keep, return_components=True)
    TR.train_step(d, Opt(), None, None)
    assert [k for k, _ in seen] == ["loss", "loss", "components", "loss"]
    assert all(v is keep for _, v in seen[:3]) and seen[3][1] is None
