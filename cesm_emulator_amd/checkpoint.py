"""Reference-format checkpoints (§8(b) B2).

train.py:1154-1165 (DDP / single-GPU branch) writes
    {"epoch", "model": UNet state_dict, "diffusion_buffers": the 8 schedule buffers,
     "optimizer": torch.optim.AdamW state_dict, "config"}
and train.py:915-946 / inference.py:47-73 read it back.  The UNet / Diffusion here carry the same
state_dict keys and FusedAdamW.state_dict() is in torch.optim.AdamW layout, so a checkpoint written by
either side loads on the other.  Loading uses torch.load(weights_only=True): tensors, numbers and the
JSON config only.
"""
from __future__ import annotations

import torch

from .model import UNet, Diffusion
from .train import guidance_p_uncond


def _plain_norm(norm):
    """norm (data.load_fields) as plain lists of floats / strings: what torch.load(weights_only=True) reads back"""
    out = {}
    for k in ("cond_vars", "target_vars"):
        out[k] = [str(v) for v in norm.get(k, [])]
    for k in ("cond_mean", "cond_std", "target_mean", "target_std"):
        out[k] = [float(v) for v in norm[k]]
    return out


def save_checkpoint(path, diffusion, optimizer, epoch, config, ema=None, norm=None):
    """train.py:1154-1165.  ema (an ema.EMA): its state_dict() goes under a further top-level key "ema"; the
    reference's readers index ckpt["model"] / use .get(...) and ignore it.  norm (data.load_fields' statistics): stored
    under a further top-level key "norm", ignored by the reference's readers in the same way."""
    full = diffusion.state_dict()
    model_sd = {k[len("model."):]: v for k, v in full.items() if k.startswith("model.")}
    diff_buf = {k: v for k, v in full.items() if not k.startswith("model.")}
    ckpt = {"epoch": epoch, "model": model_sd, "diffusion_buffers": diff_buf,
            "optimizer": optimizer.state_dict() if optimizer is not None else {}, "config": config}
    if ema is not None:
        ckpt["ema"] = ema.state_dict()
    if norm is not None:
        ckpt["norm"] = _plain_norm(norm)
    torch.save(ckpt, path)


def load_checkpoint(ckpt_path, unet, diffusion, optimizer=None, device="cuda", ema=None):
    """train.py:915-946: weights (strict=False, missing/unexpected keys reported as the reference does),
    diffusion buffers, optimizer state; returns the epoch to resume at.  ema (an ema.EMA): restored from the
    checkpoint's "ema" entry; a checkpoint without one re-initialises it from the loaded weights, and says so."""
    ckpt = torch.load(ckpt_path, map_location=device, weights_only=True)
    missing, unexpected = unet.load_state_dict(ckpt["model"], strict=False)
    if missing or unexpected:
        print("[UNet] missing keys:", missing)
        print("[UNet] unexpected keys:", unexpected)
    diff_state = diffusion.state_dict()
    diff_state.update(ckpt.get("diffusion_buffers", {}))
    diffusion.load_state_dict(diff_state, strict=False)
    if optimizer is not None and ckpt.get("optimizer"):
        optimizer.load_state_dict(ckpt["optimizer"])
    if ema is not None:
        if ckpt.get("ema"):
            ema.load_state_dict(ckpt["ema"])
        else:
            ema.reset_from_model()
            print(f"[EMA] {ckpt_path} holds no EMA: re-initialised from the loaded weights.")
    start_epoch = int(ckpt.get("epoch", 0)) + 1
    print(f"[Resume] Loaded {ckpt_path}. Resuming at epoch {start_epoch}.")
    return start_epoch


def build_from_config(cfg, device):
    """inference.py:25-45 (_build_model_from_ckpt_config)."""
    unet_cfg, train_cfg = cfg.get("unet", {}), cfg.get("train", {})
    unet = UNet(in_channels=unet_cfg.get("in_channels", 2), out_channels=unet_cfg.get("out_channels", 1),
                base_ch=unet_cfg.get("base_ch", 64), ch_mults=tuple(unet_cfg.get("ch_mults", (1, 2, 4))),
                num_res_blocks=unet_cfg.get("num_res_blocks", 2), time_dim=unet_cfg.get("time_dim", 256),
                groups=unet_cfg.get("groups", 8), dropout=unet_cfg.get("dropout", 0.0),
                use_temp_attn=unet_cfg.get("use_temp_attn", True),
                cond_channels=unet_cfg.get("cond_channels")).to(device)
    diffusion = Diffusion(unet, img_channels=1, timesteps=train_cfg.get("timesteps", 1000),
                          beta_schedule=train_cfg.get("beta_schedule", "linear"),
                          p_uncond=guidance_p_uncond(train_cfg)).to(device)
    return unet, diffusion


def load_diffusion_from_checkpoint(ckpt_path, device="cuda", use_ema=False):
    """inference.py:47-73: returns (diffusion in eval mode with frozen parameters, config).  use_ema=True loads the
    EMA of the weights (ckpt["ema"]["model"]) instead of the raw ones; KeyError if the checkpoint has none.  A
    checkpoint saved with norm= hands the statistics back as config["norm"] (for data.denormalize, summarize(scale=))."""
    dev = torch.device(device)
    ckpt = torch.load(ckpt_path, map_location=dev, weights_only=True)
    cfg = ckpt.get("config", {})
    if ckpt.get("norm") is not None:
        cfg = dict(cfg)
        cfg["norm"] = ckpt["norm"]
    if use_ema:
        if not ckpt.get("ema") or "model" not in ckpt["ema"]:
            raise KeyError(f"{ckpt_path} holds no EMA of the weights (saved without ema=)")
        weights = ckpt["ema"]["model"]
    else:
        weights = ckpt["model"]
    unet, diffusion = build_from_config(cfg, dev)
    missing, unexpected = unet.load_state_dict(weights, strict=False)
    if missing or unexpected:
        print("[UNet] missing keys:", missing)
        print("[UNet] unexpected keys:", unexpected)
    diff_state = diffusion.state_dict()
    diff_state.update(ckpt.get("diffusion_buffers", {}))
    diffusion.load_state_dict(diff_state, strict=False)
    diffusion.eval()
    for p in diffusion.parameters():
        p.requires_grad_(False)
    return diffusion, cfg
