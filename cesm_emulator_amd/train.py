"""Training step / epoch on the HIP path — mirrors train.py:808-911 (train_one_epoch, DDP branch).

Differences from the reference, all deliberate:
  * bf16 kernels instead of fp16 autocast + GradScaler (BASELINE.json asks for bf16; no loss
    scaling is needed) — `use_amp=False` selects the fp32 kernels;
  * the isfinite(loss) guard runs on device (the AdamW kernel skips a non-finite step) and is
    raised on the host when the loss is read, instead of forcing a sync before backward;
  * data-parallel gradient averaging is actually performed (the reference's DDP reducer is never
    armed): bucketed all-reduces overlapped with the backward (`dp.arm` /
    `dp.finish`, distributed.py).
"""
from __future__ import annotations

import contextlib

import torch

from .model import UNet, Diffusion, check_guidance_scale
from .optim import FusedAdamW
from .ema import EMA
from .ensemble import EnsembleVerifier


def build_model_from_config(cfg_unet):
    """train.py:669-680."""
    return UNet(in_channels=cfg_unet.get("in_channels", 2), out_channels=cfg_unet.get("out_channels", 1),
                base_ch=cfg_unet.get("base_ch", 64), ch_mults=tuple(cfg_unet.get("ch_mults", (1, 2, 4))),
                num_res_blocks=cfg_unet.get("num_res_blocks", 2), time_dim=cfg_unet.get("time_dim", 256),
                groups=cfg_unet.get("groups", 8), use_checkpoint=cfg_unet.get("use_checkpoint", True),
                dropout=cfg_unet.get("dropout", 0.0), use_temp_attn=cfg_unet.get("use_temp_attn", True),
                cond_channels=cfg_unet.get("cond_channels"))


def rank_generator(device, seed=2, rank=0):
    """per-rank t / eps stream for Diffusion.generator: seed + rank (SURVEY.md §8(e) E1 — the reference
    draws from the default generator, model.py:205-206, which is identical on every rank after the same
    manual_seed)."""
    g = torch.Generator(device=device)
    g.manual_seed(int(seed) + int(rank))
    return g


def dp_generator(device, dp, seed=None):
    """the per-rank t / eps stream of a data-parallel run: base seed `seed` (e.g. the training config's), or
    one drawn on rank 0 from the default generator and broadcast, so every rank agrees on it whatever its
    default generator state; the rank is the all-reducer's own (dp.rank), not a global lookup"""
    if seed is None:
        s = torch.randint(0, 2**31 - 1, (1,), dtype=torch.int64)
        if getattr(dp, "world", 1) > 1 and torch.distributed.is_initialized():
            dev = device if torch.distributed.get_backend() == "nccl" else torch.device("cpu")
            s = s.to(dev)
            torch.distributed.broadcast(s, src=0)
        seed = int(s.item())
    return rank_generator(device, seed, getattr(dp, "rank", 0))


def make_optimizer(diffusion, train_cfg):
    """train.py:1077-1083 (+ the clip of :865 folded into the fused step)."""
    opt = train_cfg.get("optimizer", {})
    return FusedAdamW(diffusion.parameters(), lr=opt.get("lr", 2e-4), betas=tuple(opt.get("betas", (0.9, 0.999))),
                      weight_decay=opt.get("weight_decay", 1e-4), max_grad_norm=train_cfg.get("max_grad_norm", 1.0))


def make_ema(diffusion, optimizer, train_cfg):
    """The EMA of the weights the reference's loop expects (train.py:819, `ema=`), or None unless train_cfg["ema"] is
    set: true for the defaults, or a dict with `beta` / `warmup`.  The shipped configs do not set it; it comes by
    override or from the caller's dict.  The EMA attaches itself to the optimizer, whose step then updates it."""
    cfg = train_cfg.get("ema")
    if not cfg:
        return None
    if cfg is True:
        cfg = {}
    if not isinstance(cfg, dict):
        raise TypeError(f"train.ema must be true or a mapping with beta / warmup, got {cfg!r}")
    unknown = sorted(set(cfg) - {"beta", "warmup"})
    if unknown:
        raise ValueError(f"train.ema: unknown keys {unknown} (beta, warmup)")
    return EMA(diffusion.model, optimizer, beta=cfg.get("beta", 0.9999), warmup=cfg.get("warmup", True))


def guidance_p_uncond(train_cfg):
    """p_uncond of train_cfg["guidance"] = {"p_uncond": p} (0.0 without the block); strict keys"""
    cfg = train_cfg.get("guidance") or {}
    if not isinstance(cfg, dict):
        raise TypeError(f"train.guidance must be a mapping with p_uncond, got {cfg!r}")
    unknown = sorted(set(cfg) - {"p_uncond"})
    if unknown:
        raise ValueError(f"train.guidance: unknown keys {unknown} (p_uncond)")
    return cfg.get("p_uncond", 0.0)


def make_diffusion(unet, train_cfg, lat=None):
    """The Diffusion of a training config: `timesteps`, `beta_schedule`, an optional
    train_cfg["loss"] = {"lat_weight": …, "min_snr_gamma": …} (the weighted loss) and an optional
    train_cfg["guidance"] = {"p_uncond": p} (condition dropout for classifier-free guidance; Diffusion's `p_uncond`).
    The shipped configs set neither.  lat: latitudes in degrees of the full grid's rows, from the data (Diffusion's
    `lat`)."""
    cfg = train_cfg.get("loss") or {}
    if not isinstance(cfg, dict):
        raise TypeError(f"train.loss must be a mapping with lat_weight / min_snr_gamma, got {cfg!r}")
    unknown = sorted(set(cfg) - {"lat_weight", "min_snr_gamma"})
    if unknown:
        raise ValueError(f"train.loss: unknown keys {unknown} (lat_weight, min_snr_gamma)")
    return Diffusion(unet, img_channels=1, timesteps=train_cfg.get("timesteps", 1000),
                     beta_schedule=train_cfg.get("beta_schedule", "linear"), lat_weight=cfg.get("lat_weight", 0.0),
                     min_snr_gamma=cfg.get("min_snr_gamma"), lat=lat, p_uncond=guidance_p_uncond(train_cfg))


def train_step(diffusion, optimizer, x0, cond, max_grad_norm=1.0, dp=None, t=None, noise=None, row0=None,
               return_components=False, keep=None):
    """One optimizer step; returns the loss as a device tensor (no host sync).  row0: the batch's crop row offsets
    for a weighted loss (Diffusion.loss_components).  return_components=True returns (loss, comps) instead, comps a
    [4] device tensor ordered mse_raw, mse_lat, cond_loss, total (the plain loss: loss, loss, 0, loss); the step is
    taken on total either way.  keep: the condition dropout of Diffusion.loss (bool [B]; None: drawn there when the
    diffusion has p_uncond > 0)."""
    optimizer.zero_grad(set_to_none=True)
    net = diffusion.model.net
    overlap = dp is not None and getattr(dp, "overlap", True)
    if overlap:
        dp.arm(net, optimizer.flat)  # bucket all-reduces issued during the backward
    comps = None
    if not return_components:
        loss = diffusion.loss(x0, cond, t=t, noise=noise, row0=row0, keep=keep)
    elif diffusion.weighted:
        c = diffusion.loss_components(x0, cond, t=t, noise=noise, row0=row0, keep=keep)
        loss = c["total"]
        comps = torch.stack([c["mse_raw"], c["mse_lat"], c["cond_loss"], loss.detach()])
    else:
        loss = diffusion.loss(x0, cond, t=t, noise=noise, keep=keep)
        comps = torch.stack([loss.detach(), loss.detach(), torch.zeros_like(loss), loss.detach()])
    loss.backward()
    if overlap:
        dp.finish(net)
    elif dp is not None:
        dp.allreduce_grads(optimizer.flat.grad)
    optimizer.max_grad_norm = max_grad_norm
    optimizer.step(loss=loss.detach())
    return (loss.detach(), comps) if return_components else loss.detach()


def train_one_epoch(diffusion, dl, optimizer, device, max_grad_norm=1.0, use_amp=True, epoch=1, dp=None, seed=None,
                    ema=None, metric_logger=None):
    """train.py:808-911; returns the epoch's mean loss.  With dp (world > 1) and no generator set yet, each rank
    draws t / eps from its own stream (dp_generator: base `seed`, or one broadcast from rank 0).

    ema (train.py:819): an ema.EMA attached to `optimizer`.  Its update happens inside optimizer.step(), in the AdamW
    launch and only for an applied step, so this loop has no `ema.update()` to call; the argument is checked, and
    ema_model follows use_amp.  Data-parallel runs need nothing more: after the gradient all-reduce every rank applies
    the same step to the same weights, so the ranks' EMAs stay equal.

    A weighted loss (diffusion.weighted) gets the crop row offsets of each batch from the loader's `last_row0`
    (data.DeviceWindowLoader / PinnedWindowLoader; a loader without it: no crop).  metric_logger (train.py:83-96, :898):
    its log(epoch, step, mse_raw, mse_lat, cond_loss, total) is called once per step with host floats."""
    if ema is not None and getattr(optimizer, "ema", None) is not ema:
        raise ValueError("ema is not attached to this optimizer (EMA(model, optimizer) attaches it; was it detached, "
                         "or built for another optimizer?)")
    diffusion.train()
    diffusion.model.compute_dtype = torch.bfloat16 if use_amp else torch.float32
    if ema is not None and ema.ema_model.compute_dtype != diffusion.model.compute_dtype:
        ema.ema_model.compute_dtype = diffusion.model.compute_dtype
    if dp is not None and getattr(dp, "world", 1) > 1 and diffusion.generator is None:
        diffusion.generator = dp_generator(device, dp, seed)
    weighted = getattr(diffusion, "weighted", False)
    total, steps = 0.0, 0
    for step, (cond, x0) in enumerate(dl, start=1):
        cond = cond.to(device, non_blocking=True)
        x0 = x0.to(device, non_blocking=True)
        row0 = getattr(dl, "last_row0", None) if weighted else None  # the offsets of the batch just yielded
        if metric_logger is None:
            row = None
            val = float(train_step(diffusion, optimizer, x0, cond, max_grad_norm, dp, row0=row0).item())
        else:
            _, comps = train_step(diffusion, optimizer, x0, cond, max_grad_norm, dp, row0=row0,
                                  return_components=True)
            row = comps.tolist()  # mse_raw, mse_lat, cond_loss, total: the step's one device-to-host copy
            val = row[3]
        if not torch.isfinite(torch.tensor(val)):
            raise RuntimeError(f"Non-finite loss at epoch {epoch} step {step}: {val}")
        if row is not None:
            metric_logger.log(epoch, step, *row)
        total += val
        steps += 1
    return total / max(1, steps)


def validate_ensemble(diffusion, loader, members, steps=None, ddim_eta=0.0, member_batch=None, max_batches=None,
                      ema=None, norm=None, solver="ddim", spacing=None, guidance_scale=None):
    """Ensemble verification over a loader of (cond, target) batches: per batch, `members` samples per condition
    (Diffusion.sample_ensemble with steps / ddim_eta / member_batch / solver / spacing / guidance_scale) are judged
    against the loader's target with the batch's crop row offsets (`loader.last_row0`; a loader without it: no crop), all batches accumulated on the device
    (ensemble.EnsembleVerifier, one kernel call per batch, no host synchronisation).  Returns the verifier's result():
    per-variable mse, rmse, var, spread, ssr, crps and rank_hist, area-weighted with the diffusion's `lat` (uniform
    weights without one).  ema: an ema.EMA; sampling then runs under ema.applied(diffusion).  max_batches: stop after
    that many batches.  RNG use is sample_ensemble's, batch after batch.  norm (data.load_fields' statistics): the
    per-variable results in physical units (EnsembleVerifier.result(norm=))."""
    check_guidance_scale(guidance_scale)  # before the loader is touched
    verifier = None
    with (ema.applied(diffusion) if ema is not None else contextlib.nullcontext()):
        for k, (cond, x0) in enumerate(loader):
            if max_batches is not None and k >= max_batches:
                break
            row0 = getattr(loader, "last_row0", None)  # the offsets of the batch just yielded
            device = next(diffusion.parameters()).device
            cond, x0 = cond.to(device), x0.to(device).float().contiguous()
            if verifier is None:
                verifier = EnsembleVerifier(members, x0.shape[1], lat=diffusion._lat, device=device)
            ens = diffusion.sample_ensemble(cond, members, steps=steps, ddim_eta=ddim_eta, member_batch=member_batch,
                                            solver=solver, spacing=spacing, guidance_scale=guidance_scale)
            verifier.update(ens, x0, row0=row0)
    if verifier is None:
        raise ValueError("validate_ensemble: the loader gave no batch")
    return verifier.result(norm=norm)
