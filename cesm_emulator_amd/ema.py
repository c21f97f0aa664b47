"""Exponential moving average (EMA) of the weights, updated inside the fused AdamW launch.

The reference's training loop takes an optional `ema` object, calls `ema.update()` after every optimizer step
(train.py:819, 893-894) and samples from `ema.ema_model` (train.py:485-507).  Here the parameters live in
FusedAdamW's flat fp32 buffer, and whether a step was applied at all (finite loss and gradient) is known only on the
device, inside the AdamW launch.  So the average is kept by that launch (csrc/misc.hip, cesm_adamw_ema): for an
applied step, and only then,

    n <- n + 1;  decay = min(beta, (1 + n) / (10 + n))  (warm-up)  or  beta;  ema <- ema + (1 - decay) (p_new - ema)

in fp32 from the parameter value just written; `1 - decay` is formed in double from the fp32 beta and rounded to fp32
once.  `EMA.update()` is therefore a no-op kept for the reference's loop.

Data-parallel runs need nothing more: after the gradient all-reduce every rank applies the same step to the same
weights, so every rank's EMA stays equal to the others' (as the weights themselves do).
"""
from __future__ import annotations

import contextlib

import torch

from .model import UNet
from .optim import FusedAdamW


def _check_beta(beta):
    beta = float(beta)
    if not 0.0 <= beta < 1.0:
        raise ValueError(f"beta must be in [0, 1), got {beta}")
    return beta


def ema_decay(n, beta, warmup=True) -> float:
    """Decay of the n-th EMA update (n counts from 1), in float64 as the device forms it: beta is first rounded to fp32
    (the kernel takes it as a float), then decay = min(beta, (1 + n) / (10 + n)) with warm-up, beta without.  The
    device blends with float32(1 - ema_decay(n, beta, warmup))."""
    n = int(n)
    if n < 1:
        raise ValueError(f"n counts EMA updates from 1, got {n}")
    beta = float(torch.tensor(_check_beta(beta), dtype=torch.float32).item())
    if not warmup:
        return beta
    return min(beta, (1.0 + n) / (10.0 + n))


class EMA:
    """EMA of `model`'s trainable parameters, kept by `optimizer`'s step.

    Owns one flat fp32 buffer with the layout of `optimizer.flat` (same offsets and padding), initialised from the
    current parameters.  `ema_model` is a second UNet of the same shape whose trainable parameters are views into
    that buffer (frozen parameters and buffers are copies), in eval mode and without gradients: use it wherever a
    UNet is used, e.g. as `diffusion.model` (`with ema.applied(diffusion): diffusion.sample(...)`).  Its packed
    (bf16 / GEMM-layout) weight copies are refreshed by the same parameter-epoch bump that follows every optimizer
    step."""

    def __init__(self, model, optimizer, beta=0.9999, warmup=True):
        self.beta = _check_beta(beta)
        self.warmup = bool(warmup)
        if not isinstance(model, UNet):
            raise TypeError(f"EMA needs a cesm_emulator_amd UNet, got {type(model).__name__}")
        if not isinstance(optimizer, FusedAdamW):
            raise TypeError(f"EMA is updated inside FusedAdamW.step(), got {type(optimizer).__name__}")
        flat = optimizer.flat
        named = [(k, p) for k, p in model.named_parameters() if p.requires_grad]
        if len(named) != len(flat.params) or {id(p) for _, p in named} != {id(p) for p in flat.params}:
            raise ValueError("the optimizer's flat buffer does not hold exactly the trainable parameters of the model "
                             f"({len(flat.params)} in the optimizer, {len(named)} in the model)")
        if getattr(optimizer, "ema", None) is not None:
            raise RuntimeError("the optimizer already has an EMA attached (detach() it first)")
        dev = flat.data.device
        if dev.type != "cuda":
            raise RuntimeError("EMA needs the model on the GPU")
        self.model, self.optimizer = model, optimizer
        self.flat = flat.data.clone()  # padding is zero in flat.data and stays zero under the update
        self._n_dev = torch.zeros(1, dtype=torch.int32, device=dev)
        self._omd_dev = torch.zeros(1, dtype=torch.float32, device=dev)
        offset = {id(p): off for p, off in zip(flat.params, flat.offsets)}
        with torch.random.fork_rng(devices=[]):  # the second UNet's init draws must not move the caller's RNG
            ema_model = UNet(**model.ctor_kwargs)
        ema_model = ema_model.to(dev)
        ema_model.load_state_dict(model.state_dict())
        ema_model.compute_dtype = model.compute_dtype
        own = dict(ema_model.named_parameters())
        with torch.no_grad():
            for k, p in named:
                off, n = offset[id(p)], p.numel()
                own[k].data = self.flat[off:off + n].view_as(p)
        ema_model.eval()
        for q in ema_model.parameters():
            q.requires_grad_(False)
        self.ema_model = ema_model
        optimizer.ema = self

    def detach(self):
        """Stop updating: the optimizer's step is the plain AdamW launch again; the buffer and ema_model stay."""
        if getattr(self.optimizer, "ema", None) is self:
            self.optimizer.ema = None

    def update(self):
        """No-op, kept so the reference's loop (`ema.update()` after `optimizer.step()`) runs unchanged: the update
        already happened inside the optimizer step, and only if that step was applied."""

    @property
    def num_updates(self):
        """number of EMA updates (= optimizer steps applied while attached); reading it synchronises with the device"""
        return int(self._n_dev.item())

    @num_updates.setter
    def num_updates(self, n):
        self._n_dev.fill_(int(n))

    @contextlib.contextmanager
    def applied(self, diffusion):
        """`with ema.applied(diffusion):` — diffusion.model is ema_model inside the block and what it was before
        afterwards, also when the block raises (the reference's _sample_with_optional_ema)."""
        saved = diffusion.model
        diffusion.model = self.ema_model
        try:
            yield diffusion
        finally:
            diffusion.model = saved

    def state_dict(self):
        return {"model": {k: v.detach().clone() for k, v in self.ema_model.state_dict().items()},
                "beta": self.beta, "warmup": self.warmup, "num_updates": self.num_updates}

    def load_state_dict(self, sd):
        """Copies sd["model"] into the flat buffer (and the frozen copies) and restores beta, warmup and the update
        count; a key or shape that does not match ema_model raises."""
        own = self.ema_model.state_dict()
        theirs = sd["model"]
        missing, unexpected = sorted(set(own) - set(theirs)), sorted(set(theirs) - set(own))
        if missing or unexpected:
            raise KeyError(f"EMA state does not match the model: missing {missing}, unexpected {unexpected}")
        for k, v in own.items():
            if tuple(theirs[k].shape) != tuple(v.shape):
                raise ValueError(f"EMA state {k}: shape {tuple(theirs[k].shape)}, the model has {tuple(v.shape)}")
        beta = _check_beta(sd.get("beta", self.beta))
        self.ema_model.load_state_dict(theirs)  # in place: the trainable entries are views into self.flat
        self.beta = beta
        self.warmup = bool(sd.get("warmup", self.warmup))
        self.num_updates = int(sd.get("num_updates", 0))

    def reset_from_model(self):
        """Start over from the model's current weights with a zero update count."""
        self.ema_model.load_state_dict(self.model.state_dict())
        self.num_updates = 0
