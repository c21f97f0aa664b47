"""Drop-in replacement for the reference's model.py (UNet wrapper + DDPM Diffusion).

Same constructor kwargs (model.py:44-64), same `net.*` state_dict keys and the same 8 Diffusion
buffers (model.py:158-165), so train.py / inference.py / plot_*.py can import this module
unchanged.  Compute runs on libcesm_hip.so; there is no CPU path — call `.to("cuda")` first.

Precision: `UNet.compute_dtype` selects the activation storage type of the kernels —
torch.bfloat16 (default, training/throughput) or torch.float32 (parity mode: forward matches
the CPU fp32 reference within 1e-5 relative L2).
"""
from __future__ import annotations

import numbers
import os

import torch
import torch.nn as nn

from . import kernels as K
from .video_net import UNetModel3D, net_apply


class UNet(nn.Module):
    """model.py:37-134."""

    def __init__(self, in_channels: int = 2, out_channels: int = 1, base_ch: int = 64, ch_mults=(1, 2, 4),
                 num_res_blocks: int = 2, time_dim: int = 256, groups: int = 8, dropout: float = 0.0,
                 attn_heads: int = 8, attn_dim_head: int = 32, use_sparse_linear_attn: bool = True,
                 use_mid_attn: bool = False, init_kernel_size: int = 7, use_checkpoint: bool = False,
                 use_temp_attn: bool = True, day_cond: bool = False, year_cond: bool = False,
                 cond_map: bool = True, cond_channels=None):
        super().__init__()
        # what an identically shaped second instance is built from (ema.EMA's ema_model)
        self.ctor_kwargs = dict(in_channels=in_channels, out_channels=out_channels, base_ch=base_ch,
                                ch_mults=tuple(ch_mults), num_res_blocks=num_res_blocks, time_dim=time_dim,
                                groups=groups, dropout=dropout, attn_heads=attn_heads, attn_dim_head=attn_dim_head,
                                use_sparse_linear_attn=use_sparse_linear_attn, use_mid_attn=use_mid_attn,
                                init_kernel_size=init_kernel_size, use_checkpoint=use_checkpoint,
                                use_temp_attn=use_temp_attn, day_cond=day_cond, year_cond=year_cond,
                                cond_map=cond_map, cond_channels=cond_channels)
        self.net = UNetModel3D(n_vars=out_channels, model_dim=base_ch, dim_mults=tuple(ch_mults),
                               attn_heads=attn_heads, attn_dim_head=attn_dim_head,
                               use_sparse_linear_attn=use_sparse_linear_attn, use_mid_attn=use_mid_attn,
                               init_kernel_size=init_kernel_size, resnet_groups=groups,
                               use_checkpoint=use_checkpoint, use_temp_attn=use_temp_attn, day_cond=day_cond,
                               year_cond=year_cond, cond_map=cond_map, cond_channels=cond_channels)

    @property
    def compute_dtype(self):
        return self.net.compute_dtype

    @compute_dtype.setter
    def compute_dtype(self, dt):
        if dt not in (torch.float32, torch.bfloat16):
            raise ValueError("compute_dtype must be torch.float32 or torch.bfloat16")
        self.net.compute_dtype = dt
        self.net.invalidate_packed()

    def forward(self, x_t, cond, t):
        if x_t.ndim == 4:
            x_t = x_t.unsqueeze(2)
        elif x_t.ndim != 5:
            raise ValueError(f"x_t must be 4D or 5D, got {x_t.ndim}D")
        if cond is None:
            raise ValueError("cond must be provided")
        if cond.ndim == 4:
            cond = cond.unsqueeze(2)
        elif cond.ndim != 5:
            raise ValueError(f"cond must be 4D or 5D, got {cond.ndim}D")
        Fx, Fc = x_t.shape[2], cond.shape[2]
        if Fx != Fc and not (Fx == 1 or Fc == 1):
            raise ValueError(f"Frame mismatch: x_t F={Fx}, cond F={Fc}")
        V, Cc = self.net.n_vars, self.net.n_cond
        if Cc == V:
            if x_t.shape[1] != V or cond.shape[1] != V:
                raise ValueError(f"model with {V} target variable(s): x_t has {x_t.shape[1]} channels and cond "
                                 f"{cond.shape[1]}, both need {V}")
        elif x_t.shape[1] != V or cond.shape[1] != Cc:
            raise ValueError(f"model with {V} target variable(s) and {Cc} conditioning map(s) (cond_channels): x_t has "
                             f"{x_t.shape[1]} channels and cond {cond.shape[1]}; they need {V} and {Cc}")
        if not x_t.is_cuda:
            raise RuntimeError("cesm_emulator_amd.UNet runs on the GPU only (move model and inputs to 'cuda')")
        if not torch.is_tensor(t):
            t = torch.tensor([t], dtype=torch.long, device=x_t.device)
        elif t.ndim == 0:
            t = t[None]
        t = t.to(device=x_t.device, dtype=torch.long).contiguous()
        if t.shape[0] == 1 and x_t.shape[0] > 1:
            t = t.expand(x_t.shape[0]).contiguous()
        # frame-broadcast of model.py:111-118 happens inside the stem kernel (stride-0 read)
        # the network's output is [B,V,F,H,W]; only frame F//2 is kept (model.py:124-130), so
        # the 1x1 head conv is evaluated on that frame only.
        return net_apply(self.net, x_t.float().contiguous(), cond.float().contiguous(), t)


class _MSE(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, noise):
        ctx.save_for_backward(pred, noise)
        return K.mse(pred, noise)

    @staticmethod
    def backward(ctx, g):
        pred, noise = ctx.saved_tensors
        return K.mse_bwd(pred, noise, g.reshape(1).contiguous()), None


class _WLoss(torch.autograd.Function):
    """K.wloss as three 0-d outputs (mse_raw, mse_lat, total); only total is differentiable, and only in pred"""

    @staticmethod
    def forward(ctx, pred, noise, w, row0, a, lam):
        ctx.save_for_backward(pred, noise, w, row0, a)
        ctx.lam = lam
        out = K.wloss(pred, noise, w, row0, a, lam)
        raw, lat, total = out[0], out[1], out[2]
        ctx.mark_non_differentiable(raw, lat)
        return raw, lat, total

    @staticmethod
    def backward(ctx, g_raw, g_lat, g):
        pred, noise, w, row0, a = ctx.saved_tensors
        d = K.wloss_bwd(pred, noise, w, row0, a, ctx.lam, g.reshape(1).contiguous())
        return d, None, None, None, None, None


class _CondMask(torch.autograd.Function):
    """K.cond_mask: cond with the dropped samples (keep False) set to zero; the backward applies the same kernel to the
    incoming gradient, so a dropped sample's d cond is exactly zero"""

    @staticmethod
    def forward(ctx, cond, keep):
        ctx.save_for_backward(keep)
        return K.cond_mask(cond, keep)

    @staticmethod
    def backward(ctx, g):
        keep, = ctx.saved_tensors
        return K.cond_mask(g.float().contiguous(), keep), None


def check_guidance_scale(guidance_scale):
    """a sampler's guidance_scale as None (unguided: None or exactly 1.0) or a float (a finite number >= 0, else
    ValueError)"""
    if guidance_scale is None:
        return None
    s = K.guidance_scale_arg(guidance_scale, "guidance_scale")
    return None if s == 1.0 else s


def latitude_weights(lat):
    """Row weights of a regular lat-lon grid from its latitudes in degrees: clamp_min(cos(lat), 0) / (mean + 1e-8),
    in float64 on the host, rounded to fp32 once (a CPU tensor [Hg])."""
    lat = torch.as_tensor(lat, dtype=torch.float64, device="cpu").reshape(-1)
    w = torch.cos(torch.deg2rad(lat)).clamp_min(0.0)
    return (w / (w.mean() + 1e-8)).float()


def min_snr_weights(alphas_cumprod, gamma):
    """Min-SNR-gamma weights of an eps-prediction loss (Hang et al. 2023): a_t = min(SNR_t, gamma) / SNR_t =
    min(1, gamma (1 - ac_t) / ac_t), in float64 from the fp32 alphas_cumprod entries, rounded to fp32 once."""
    ac = alphas_cumprod.double()
    return (gamma * (1.0 - ac) / ac).clamp_max(1.0).float()


def check_row0(row0, B, H, Hg, device, has_lat=True):
    """Crop row offsets as a device int64 [B] tensor (None stays None): the check of Diffusion.loss_components and of
    ensemble.ensemble_stats.  A list or CPU tensor is range-checked (0 <= row0, row0 + H <= Hg, else ValueError); a
    device tensor is NOT read back (no synchronisation): the kernels clamp the row index, so a wrong device row0 gives
    a wrong number, never a fault.  has_lat=False only words the error (no latitudes: the batch is the whole grid)."""
    if row0 is None:
        return None
    if torch.is_tensor(row0) and row0.is_cuda:
        return row0.to(device=device, dtype=torch.long).contiguous()
    r = torch.as_tensor(row0, dtype=torch.long).reshape(-1)
    if r.numel() != B:
        raise ValueError(f"row0 needs one entry per sample ({B}), got {r.numel()}")
    if bool(((r < 0) | (r + H > Hg)).any()):
        hint = "" if has_lat else " (no `lat` given: the batch is the whole grid, so row0 must be 0)"
        raise ValueError(f"row0 must satisfy 0 <= row0 and row0 + H <= Hg with H = {H}, Hg = {Hg}, got "
                         f"{r.tolist()}{hint}")
    return r.to(device)


class Diffusion(nn.Module):
    """model.py:141-208 — linear β schedule (1e-4 → 2e-2), ε-prediction MSE.

    Weighted loss (both off by default, which leaves loss() as it was):
      lat_weight   lam in [0, 1]: every grid row h weighs (1 - lam) + lam w[h], w = latitude_weights(lat);
      min_snr_gamma   None or gamma > 0: sample b weighs min(1, gamma (1 - ac_t) / ac_t) at its timestep t;
      lat   latitudes in degrees of the FULL grid's rows (length Hg), or None: then the tensor's own H rows span
            linspace(-90, 90, H), as the reference's _latitude_weights, and a crop offset makes no sense.
    The weights are normalised over the full grid, so an equatorial crop weighs more than a polar one.

    Classifier-free guidance (Ho & Salimans 2022; off by default): the null condition is the all-zero cond (the data
    path z-scores emissions, so zero is the climatological mean); there is no learned null token and no new parameter.
      p_uncond   in [0, 1]: in training mode every sample's cond is dropped (zeroed) with this probability, so the one
                 network learns eps(x, cond) and eps(x, 0).  A plain attribute: state_dict() keeps the 8 buffers.
      guidance_scale (the samplers' argument)   None or 1.0: the conditional sampler, as without it; another finite
                 s >= 0: eps = eps(x, 0) + s (eps(x, cond) - eps(x, 0)) from ONE network evaluation per step on 2 B
                 rows and a fused update kernel; s = 0 is the unconditional sampler.  A model trained with
                 p_uncond = 0 may be sampled with guidance too, but its unconditional branch was never trained."""

    def __init__(self, model, img_channels=1, timesteps=1000, beta_schedule="linear", lat_weight=0.0,
                 min_snr_gamma=None, lat=None, p_uncond=0.0):
        super().__init__()
        self.model = model
        self.img_channels = img_channels
        self.T = timesteps
        if beta_schedule != "linear":
            raise ValueError("Only 'linear' beta_schedule implemented")
        self.lat_weight = float(lat_weight)
        if not 0.0 <= self.lat_weight <= 1.0:
            raise ValueError(f"lat_weight must be in [0, 1], got {lat_weight}")
        if min_snr_gamma is not None:
            if isinstance(min_snr_gamma, bool) or not isinstance(min_snr_gamma, numbers.Real) or not min_snr_gamma > 0:
                raise ValueError(f"min_snr_gamma must be None or a number > 0, got {min_snr_gamma!r}")
            min_snr_gamma = float(min_snr_gamma)
        self.min_snr_gamma = min_snr_gamma
        if isinstance(p_uncond, bool) or not isinstance(p_uncond, numbers.Real) or not 0.0 <= p_uncond <= 1.0:
            raise ValueError(f"p_uncond must be a probability in [0, 1], got {p_uncond!r}")
        self.p_uncond = float(p_uncond)  # a plain attribute, not a buffer
        self._lat = None if lat is None else torch.as_tensor(lat, dtype=torch.float64, device="cpu").reshape(-1)
        if self._lat is not None and self._lat.numel() < 1:
            raise ValueError("lat must hold the latitude of every grid row")
        self._lat_w = {}  # (Hg, device) -> fp32 row weights
        betas = torch.linspace(1e-4, 2e-2, timesteps)
        alphas = 1.0 - betas
        ac = torch.cumprod(alphas, dim=0)
        acp = torch.cat([torch.tensor([1.0]), ac[:-1]], dim=0)
        self.register_buffer("betas", betas)
        self.register_buffer("alphas", alphas)
        self.register_buffer("alphas_cumprod", ac)
        self.register_buffer("alphas_cumprod_prev", acp)
        self.register_buffer("sqrt_alphas_cumprod", torch.sqrt(ac))
        self.register_buffer("sqrt_one_minus_alphas_cumprod", torch.sqrt(1.0 - ac))
        self.register_buffer("sqrt_recip_alphas", torch.sqrt(1.0 / alphas))
        self.register_buffer("posterior_variance", betas * (1.0 - acp) / (1.0 - ac))
        # not part of state_dict(): checkpoints keep the reference's 8 buffers
        self.register_buffer("min_snr_weight", None if min_snr_gamma is None else min_snr_weights(ac, min_snr_gamma),
                             persistent=False)
        # draws of t / eps in loss(): None = the default generator (as model.py:205-206); data-parallel
        # training gives every rank its own stream (train.rank_generator) so ranks do not draw identical
        # t / eps for their different samples
        self.generator = None

    @property
    def weighted(self):
        """whether loss() is the weighted loss (loss_components()['total']) and not the plain mean"""
        return self.lat_weight != 0.0 or self.min_snr_gamma is not None

    def q_sample(self, x0, t, noise=None):
        if noise is None:
            noise = torch.randn_like(x0)
        xt = K.q_sample(x0.float().contiguous(), noise.float().contiguous(), t.long().contiguous(),
                        self.sqrt_alphas_cumprod, self.sqrt_one_minus_alphas_cumprod)
        return xt, noise

    def _eps(self, x0, cond, t, noise, keep=None):
        """the draws of loss() (t, then noise, then -- only in training mode with p_uncond > 0 and no keep given -- the
        condition dropout keep = rand(B) >= p_uncond, all on self.generator) and the network's eps for them.  keep:
        bool [B], True = the sample keeps its cond; the others see the null condition (cond zeroed by cesm_cond_mask,
        whose backward zeroes their d cond).  keep None and nothing drawn: cond goes to the network untouched."""
        B = x0.size(0)
        g = self.generator
        if t is None:
            t = torch.randint(0, self.T, (B,), device=x0.device, generator=g).long()
        if noise is None:
            noise = torch.randn(x0.shape, device=x0.device, dtype=x0.dtype, generator=g)
        if keep is None and self.p_uncond > 0.0 and self.training:
            keep = torch.rand(B, device=x0.device, generator=g) >= self.p_uncond
        if keep is not None:
            keep = torch.as_tensor(keep, dtype=torch.bool, device=x0.device).contiguous()
            if tuple(keep.shape) != (B,):
                raise ValueError(f"keep needs one entry per sample ({B}), got {tuple(keep.shape)}")
            cond = _CondMask.apply(cond.to(x0.device).float().contiguous(), keep)
        x_t, noise = self.q_sample(x0, t, noise)
        return self.model(x_t, cond, t), noise.float().contiguous(), t

    def loss(self, x0, cond, t=None, noise=None, row0=None, keep=None):
        """model.py:203-208; optional t / noise / keep make the draw reproducible for parity tests (keep: _eps).  With
        lat_weight or min_snr_gamma set this is loss_components(...)['total'] (row0: see there), else the plain mean."""
        if self.weighted:
            return self.loss_components(x0, cond, t=t, noise=noise, row0=row0, keep=keep)["total"]
        eps, noise, _ = self._eps(x0, cond, t, noise, keep)
        return _MSE.apply(eps, noise)

    def lat_weights(self, H, device):
        """fp32 row weights [Hg] on `device` (latitude_weights of `lat`, or of linspace(-90, 90, H) without one),
        cached per (Hg, device)"""
        if self._lat is not None and self._lat.numel() < H:
            raise ValueError(f"lat has {self._lat.numel()} rows, the batch {H}")
        Hg = H if self._lat is None else self._lat.numel()
        key = (Hg, torch.device(device))
        w = self._lat_w.get(key)
        if w is None:
            lat = torch.linspace(-90.0, 90.0, Hg, dtype=torch.float64) if self._lat is None else self._lat
            w = self._lat_w[key] = latitude_weights(lat).to(device)
        return w

    def _row0(self, row0, B, H, Hg, device):
        """row0 as a device int64 [B] tensor (None stays None).  A list or CPU tensor is range-checked here; a device
        tensor is NOT read back (no synchronisation): the kernel's clamp of the row index is its only guard, so a
        wrong device row0 gives a wrong loss, never a fault."""
        return check_row0(row0, B, H, Hg, device, has_lat=self._lat is not None)

    def loss_components(self, x0, cond, t=None, noise=None, row0=None, keep=None):
        """The reference training loop's hook (train.py:836-841): {'mse_raw', 'mse_lat', 'cond_loss', 'total'} as 0-d
        device tensors from one weighted-loss kernel (csrc/misc.hip cesm_wloss; formulas in include/cesm_hip.h).
        `total` is differentiable; the others are detached, cond_loss is a zero.  RNG use is that of loss(); keep: the
        condition dropout of loss().

        row0: the grid row of each sample's row 0 (crops; DeviceWindowLoader.last_row0), [B]; None: 0.  A list or CPU
        tensor is validated (0 <= row0, row0 + H <= Hg, else ValueError before anything is launched); a CUDA int64
        tensor is not synchronised on (see _row0)."""
        if x0.ndim != 4:
            raise ValueError(f"x0 must be [B, V, H, W], got {tuple(x0.shape)}")
        B, H = x0.shape[0], x0.shape[2]
        w = self.lat_weights(H, x0.device)
        row0 = self._row0(row0, B, H, w.numel(), x0.device)
        eps, noise, t = self._eps(x0, cond, t, noise, keep)
        a = None if self.min_snr_weight is None else self.min_snr_weight[t]
        raw, lat, total = _WLoss.apply(eps, noise, w, row0, a, self.lat_weight)
        return {"mse_raw": raw, "mse_lat": lat, "cond_loss": torch.zeros((), device=x0.device), "total": total}

    def _coefs(self):
        return self.sqrt_recip_alphas, self.betas, self.sqrt_one_minus_alphas_cumprod, self.posterior_variance

    def _guided_eps(self, x_t, cond, t):
        """the one network evaluation of a guided step: (x2, eps2) on 2 B rows -- x_t twice, [cond, 0], t twice; rows
        [0, B) of eps2 are eps(x, cond), rows [B, 2B) eps(x, 0)"""
        cond = cond.to(x_t.device).float()
        x2 = torch.cat([x_t, x_t], dim=0)
        eps2 = self.model(x2, torch.cat([cond, torch.zeros_like(cond)], dim=0), torch.cat([t, t], dim=0))
        return x2, eps2.float().contiguous()

    @torch.no_grad()
    def p_sample(self, x_t, cond, t, noise=None, guidance_scale=None):
        """model.py:168-183 (DDPM ancestral step): model evaluation + one fused update kernel.  guidance_scale: see
        the class docstring (None / 1.0: this step as it was; else one evaluation on 2 B rows and the guided kernel;
        RNG use does not change)."""
        gs = check_guidance_scale(guidance_scale)
        with torch.inference_mode():
            x_t = x_t.float().contiguous()
            t = t.to(device=x_t.device, dtype=torch.long).contiguous()
            if gs is not None:
                B = x_t.shape[0]
                t = t.expand(B).contiguous()
                x2, eps2 = self._guided_eps(x_t, cond, t)
                if (t == 0).all():
                    return K.ddpm_step_cfg(x2, eps2, None, t, *self._coefs(), gs)[:B]
                if noise is None:
                    noise = torch.randn_like(x_t)
                return K.ddpm_step_cfg(x2, eps2, noise.float().contiguous(), t, *self._coefs(), gs)[:B]
            eps = self.model(x_t, cond, t).float().contiguous()
            if (t == 0).all():
                return K.ddpm_step(x_t, eps, None, t, *self._coefs())
            if noise is None:
                noise = torch.randn_like(x_t)
            return K.ddpm_step(x_t, eps, noise.float().contiguous(), t, *self._coefs())

    def sample_schedule(self, steps, spacing="uniform"):
        """The `steps` time indices tau of a strided sampling run: an increasing sub-sequence of 0 … T-1 that ends at
        T-1 and (for steps >= 2) starts at 0.  Sampling walks it from the back; the t_prev of tau_0 is -1.

        spacing="uniform": tau_i = round(i (T-1) / (steps-1)) in exact integer arithmetic (halves round up).
        spacing="logsnr": uniform in lambda_t = log(ac_t / (1 - ac_t)) / 2 (float64 from the fp32 alphas_cumprod):
        tau_i is the index whose lambda is nearest lambda_0 + i (lambda_{T-1} - lambda_0) / (steps-1), ties to the
        smaller index; then tau_0 = 0 and tau_last = T-1 are set and one forward pass (tau_i >= tau_{i-1} + 1) and one
        backward pass from T-1 (tau_i <= tau_{i+1} - 1) make the sequence strictly increasing for every steps <= T.
        The multistep solver needs this grid: on the uniform one its penultimate step spans most of the log-SNR range
        and the extrapolation overshoots."""
        steps, T = int(steps), self.T
        if spacing not in ("uniform", "logsnr"):
            raise ValueError(f"spacing must be 'uniform' or 'logsnr', got {spacing!r}")
        if not 1 <= steps <= T:
            raise ValueError(f"steps must be in 1 … T = {T}, got {steps}")
        if steps == 1:
            return [T - 1]
        if spacing == "uniform":
            return [(2 * i * (T - 1) + (steps - 1)) // (2 * (steps - 1)) for i in range(steps)]
        lam = self._lambda(self.alphas_cumprod.detach().cpu())
        l0, l1 = lam[0].item(), lam[-1].item()
        target = torch.tensor([l0 + i * (l1 - l0) / (steps - 1) for i in range(steps)], dtype=torch.float64)
        # argmin returns the first of equal minima: ties go to the smaller index
        tau = torch.argmin((lam[None, :] - target[:, None]).abs(), dim=1).tolist()
        tau[0], tau[-1] = 0, T - 1
        for i in range(1, steps):
            tau[i] = max(tau[i], tau[i - 1] + 1)
        tau[-1] = T - 1
        for i in range(steps - 2, -1, -1):
            tau[i] = min(tau[i], tau[i + 1] - 1)
        return tau

    @staticmethod
    def _lambda(ac):
        """half log-SNR lambda = log(ac / (1 - ac)) / 2 in float64 from fp32 alphas_cumprod entries"""
        ac = ac.double()
        return 0.5 * torch.log(ac / (1.0 - ac))

    def _ddim_args(self, t, t_prev, eta):
        """t, t_prev as broadcast int64 tensors on the schedule's device and eta as a float, range-checked (the update
        kernel checks nothing): -1 <= t_prev < t < T, eta >= 0"""
        dev = self.alphas_cumprod.device
        t = torch.as_tensor(t, device=dev).long()
        t_prev = torch.as_tensor(t_prev, device=dev).long()
        t, t_prev = torch.broadcast_tensors(t, t_prev)
        eta = float(eta)
        if not eta >= 0.0:
            raise ValueError(f"eta must be >= 0, got {eta}")
        if bool(((t < 0) | (t >= self.T) | (t_prev < -1) | (t_prev >= t)).any()):
            raise ValueError(f"DDIM step needs -1 <= t_prev < t < T = {self.T}, got t = {t.tolist()}, "
                             f"t_prev = {t_prev.tolist()}")
        return t.contiguous(), t_prev.contiguous(), eta

    def ddim_coefs(self, t, t_prev, eta=0.0):
        """(a, b, sigma) of the generalized DDIM step x_prev = a x_t + b eps + sigma z (Song et al. 2021, eq. 12) from
        t to t_prev < t, as float64 tensors of t's shape; t, t_prev: ints or integer tensors, t_prev = -1 means
        alphas_cumprod_prev = 1 (the step returns the x0 estimate).  Computed in float64 from the fp32 alphas_cumprod
        entries; the update kernel (csrc/misc.hip ddim_step_kernel) does the same arithmetic and rounds each of the
        three to fp32 once.  eta = 0: deterministic DDIM; eta = 1 with t_prev = t - 1: the DDPM step."""
        t, t_prev, eta = self._ddim_args(t, t_prev, eta)
        ac = self.alphas_cumprod
        at = ac[t].double()
        ap = torch.where(t_prev < 0, torch.ones_like(at), ac[t_prev.clamp_min(0)].double())
        sigma = eta * torch.sqrt((1.0 - ap) / (1.0 - at)) * torch.sqrt(1.0 - at / ap)
        a = torch.sqrt(ap / at)
        b = torch.sqrt((1.0 - ap - sigma * sigma).clamp_min(0.0)) - torch.sqrt(ap * (1.0 - at) / at)
        return a, b, sigma

    @torch.no_grad()
    def ddim_step(self, x_t, cond, t, t_prev, eta=0.0, noise=None, guidance_scale=None):
        """One generalized DDIM step t -> t_prev (per sample; ddim_coefs has the formula): model evaluation + one
        fused update kernel, the few-step counterpart of p_sample.  Step noise is used (and, without `noise`, drawn
        with randn_like) only when eta > 0 and some t_prev >= 0.  guidance_scale: as p_sample."""
        gs = check_guidance_scale(guidance_scale)
        with torch.inference_mode():
            x_t = x_t.float().contiguous()
            B = x_t.shape[0]
            t, t_prev, eta = self._ddim_args(t, t_prev, eta)
            t = t.to(x_t.device).expand(B).contiguous()
            t_prev = t_prev.to(x_t.device).expand(B).contiguous()
            if gs is None:
                eps = self.model(x_t, cond, t).float().contiguous()
            else:
                x2, eps2 = self._guided_eps(x_t, cond, t)
            z = None
            if eta > 0.0 and bool((t_prev >= 0).any()):
                z = (torch.randn_like(x_t) if noise is None else noise.to(x_t.device)).float().contiguous()
            if gs is not None:
                return K.ddim_step_cfg(x2, eps2, z, t, t_prev, self.alphas_cumprod, eta, gs)[:B]
            return K.ddim_step(x_t, eps, z, t, t_prev, self.alphas_cumprod, eta)

    def _dpmpp_args(self, t, t_prev, t_last):
        """t, t_prev, t_last as broadcast int64 tensors on the schedule's device, range-checked (the update kernel only
        clamps its table indices): -1 <= t_prev < t < T and t_last == -1 (no history) or t < t_last < T"""
        dev = self.alphas_cumprod.device
        t, t_prev, t_last = torch.broadcast_tensors(*(torch.as_tensor(v, device=dev).long()
                                                      for v in (t, t_prev, t_last)))
        bad = (t < 0) | (t >= self.T) | (t_prev < -1) | (t_prev >= t) | ((t_last != -1) & ((t_last <= t) |
                                                                                            (t_last >= self.T)))
        if bool(bad.any()):
            raise ValueError(f"DPM-Solver++ step needs -1 <= t_prev < t < T = {self.T} and t_last = -1 or "
                             f"t < t_last < T, got t = {t.tolist()}, t_prev = {t_prev.tolist()}, "
                             f"t_last = {t_last.tolist()}")
        return t.contiguous(), t_prev.contiguous(), t_last.contiguous()

    def dpmpp_coefs(self, t, t_prev, t_last):
        """(a, b, c, c1, c2) of the DPM-Solver++(2M) step (Lu et al. 2022) from t to t_prev < t,
            x_prev = a x_t + b eps + c x0_last,   x0 = c1 x_t + c2 eps,
        as float64 tensors of the broadcast shape; t, t_prev, t_last: ints or integer tensors.  x0 is this step's data
        prediction (the next step's history), x0_last the one of the previous executed step, taken at t_last > t;
        t_last = -1: no history.  With alpha_u = sqrt(ac_u), sigma_u = sqrt(1 - ac_u) and
        lambda_u = log(ac_u / (1 - ac_u)) / 2 in float64 from the fp32 alphas_cumprod entries:
            c1 = 1 / alpha_t,  c2 = -sigma_t / alpha_t;
            t_prev >= 0:  h = lambda_prev - lambda_t,  G = -alpha_prev expm1(-h),
                          w_c = 1, w_p = 0 without history, else r = (lambda_t - lambda_last) / h,
                          w_c = 1 + 1 / (2 r), w_p = -1 / (2 r);
                          a = sigma_prev / sigma_t + G w_c / alpha_t,  b = -G w_c sigma_t / alpha_t,  c = G w_p;
            t_prev = -1 (the last step: returns the x0 estimate, never extrapolates):  a = c1, b = c2, c = 0.
        Without history the step is the DDIM step at eta = 0.  The update kernel (csrc/misc.hip dpmpp_step_kernel) does
        the same arithmetic and rounds each of the five to fp32 once."""
        t, t_prev, t_last = self._dpmpp_args(t, t_prev, t_last)
        ac = self.alphas_cumprod
        at, ap, al = ac[t].double(), ac[t_prev.clamp_min(0)].double(), ac[t_last.clamp_min(0)].double()
        alpha_t, sigma_t, lam_t = at.sqrt(), (1.0 - at).sqrt(), self._lambda(at)
        c1, c2 = 1.0 / alpha_t, -sigma_t / alpha_t
        h = self._lambda(ap) - lam_t
        G = -ap.sqrt() * torch.expm1(-h)
        r = (lam_t - self._lambda(al)) / h
        hist = t_last >= 0
        w_c = torch.where(hist, 1.0 + 1.0 / (2.0 * r), torch.ones_like(r))
        w_p = torch.where(hist, -1.0 / (2.0 * r), torch.zeros_like(r))
        last = t_prev < 0
        a = torch.where(last, c1, (1.0 - ap).sqrt() / sigma_t + G * w_c / alpha_t)
        b = torch.where(last, c2, -G * w_c * sigma_t / alpha_t)
        c = torch.where(last, torch.zeros_like(G), G * w_p)
        return a, b, c, c1, c2

    @torch.no_grad()
    def dpmpp_step(self, x_t, cond, t, t_prev, t_last, x0_last=None, guidance_scale=None):
        """One DPM-Solver++(2M) step t -> t_prev (per sample; dpmpp_coefs has the formula): model evaluation + one
        fused update kernel, the eager counterpart of ddim_step.  Returns (x_prev, x0): x0 is the step's data
        prediction, to be passed as x0_last, with this t as t_last, to the next step.  x0_last is needed where
        t_last >= 0 and is not read elsewhere; deterministic, draws nothing.  guidance_scale: as p_sample."""
        gs = check_guidance_scale(guidance_scale)
        with torch.inference_mode():
            x_t = x_t.float().contiguous()
            B = x_t.shape[0]
            t, t_prev, t_last = (v.to(x_t.device).expand(B).contiguous() for v in self._dpmpp_args(t, t_prev, t_last))
            if x0_last is None and bool(((t_last >= 0) & (t_prev >= 0)).any()):
                raise ValueError("dpmpp_step: t_last >= 0 needs x0_last, the previous step's x0 estimate")
            if x0_last is not None:
                x0_last = x0_last.to(x_t.device).float().contiguous()
            if gs is not None:
                x2, eps2 = self._guided_eps(x_t, cond, t)
                x_prev, x0 = K.dpmpp_step_cfg(x2, eps2, x0_last, t, t_prev, t_last, self.alphas_cumprod, gs)
                return x_prev[:B], x0
            eps = self.model(x_t, cond, t).float().contiguous()
            return K.dpmpp_step(x_t, eps, x0_last, t, t_prev, t_last, self.alphas_cumprod)

    def _sample_grid(self, steps, ddim_eta, solver, spacing):
        """the checks of sample()'s solver arguments, before anything is captured: (tau, ddim_eta), tau = None for
        steps=None (the ancestral loop, which has no grid: solver and spacing are only checked)"""
        if solver not in ("ddim", "dpmpp2m"):
            raise ValueError(f"solver must be 'ddim' or 'dpmpp2m', got {solver!r}")
        if spacing is None:
            spacing = "uniform" if solver == "ddim" else "logsnr"
        if spacing not in ("uniform", "logsnr"):
            raise ValueError(f"spacing must be 'uniform' or 'logsnr', got {spacing!r}")
        if solver == "dpmpp2m":
            if steps is None:
                raise ValueError("solver='dpmpp2m' needs steps")
            if float(ddim_eta) != 0.0:
                raise ValueError(f"solver='dpmpp2m' is deterministic: ddim_eta must be 0, got {ddim_eta}")
        if steps is None:
            return None, ddim_eta
        ddim_eta = float(ddim_eta)
        if not ddim_eta >= 0.0:
            raise ValueError(f"ddim_eta must be >= 0, got {ddim_eta}")
        return self.sample_schedule(steps, spacing), ddim_eta

    @torch.no_grad()
    def sample(self, cond, shape, device, use_graph=None, x_T=None, noise_seq=None, steps=None, ddim_eta=0.0,
               solver="ddim", spacing=None, guidance_scale=None):
        """model.py:186-194.  On the GPU every p_sample step is ONE replay of a captured HIP graph (the
        F=1 network forward + the fused update); the host only sets t and draws the step noise.  RNG use
        is the reference's: randn(shape) for x_T, then randn_like(x) for every step with t > 0, drawn
        outside the graph on the default generator, so the result equals the eager loop.  Test hooks:
        x_T (initial state) and noise_seq ([T, *shape], noise of step i = noise_seq[i], i = 0 for t = T-1)
        replace the draws.  use_graph=False (or CESM_SAMPLE_GRAPH=0) runs the eager loop.

        steps=N (1 <= N <= T) samples in N generalized DDIM steps over sample_schedule(N) instead (ddim_eta = 0:
        deterministic; > 0: stochastic, 1 on the full grid is DDPM); steps=None is the ancestral loop above whatever
        ddim_eta is.  RNG use then: randn(shape) for x_T unless given, and only for ddim_eta > 0 one randn_like per
        executed step except the last, in step order, outside the graph on the default generator; noise_seq is
        [N, *shape] (entry k for executed step k, the last one unused).  ddim_eta = 0 with x_T draws nothing.

        solver="dpmpp2m" takes the N steps with DPM-Solver++(2M) instead (dpmpp_coefs; second order: every step but
        the first and the last also uses the previous step's x0 estimate, at no further network evaluation).  It
        needs steps and ddim_eta == 0, is deterministic (randn(shape) for x_T unless given, nothing else; noise_seq is
        unused), and for executed step k its t_last is the t of step k-1, -1 at k = 0.  spacing picks the time grid
        (sample_schedule): None means "uniform" for ddim and "logsnr" for dpmpp2m; either may be given to either.

        guidance_scale=s (classifier-free guidance, every solver, graph and eager): None or exactly 1.0 is the code
        path above, unchanged; another finite s >= 0 (else ValueError, before anything is captured or launched)
        evaluates the network once per step on 2 B rows -- x twice, [cond, 0], t twice -- and takes the step with
        eps(x, 0) + s (eps(x, cond) - eps(x, 0)) in the guided update kernel (cesm_*_step_cfg); s = 0 is the
        unconditional sampler.  The shapes of x_T, noise_seq and the result and the RNG use are those of the unguided
        call.  A model trained with p_uncond = 0 never trained its unconditional branch; it is sampled all the same."""
        return self._sample(cond, shape, device, use_graph, x_T, noise_seq, steps, ddim_eta, False, solver=solver,
                            spacing=spacing, guidance_scale=guidance_scale)

    @torch.no_grad()
    def sample_ensemble(self, cond, members, device=None, steps=None, ddim_eta=0.0, member_batch=None, x_T=None,
                        noise_seq=None, use_graph=None, solver="ddim", spacing=None, guidance_scale=None):
        """`members` samples for every row of cond: [B, M, V, H, W] fp32 (cond [B, V, H, W] or a window
        [B, V, Fc, H, W]).  The B M jobs, b-major (job b M + m is member m of cond[b]), run in chunks of at most
        member_batch network samples (default: all in one chunk); each chunk goes through sample()'s loop with
        cond[b_idx] of its jobs and is written straight into its slice of the result, so no [M, B, ...] stack is built.
        On the graph path one GraphSampleStep is captured per distinct chunk size of the call (at most two: the full
        chunks and a shorter last one); later chunks of that size load their cond and x_T into its static buffers.

        steps / ddim_eta / use_graph / solver / spacing: as sample().  RNG use, chunk by chunk: randn for the chunk's
        x_T, then that chunk's step noise exactly as sample() documents, then the next chunk.  Test hooks: x_T [B, M, V, H, W] and
        noise_seq [N, B, M, V, H, W] replace the draws, sliced per chunk; with them a chunk equals, bit for bit,
        sample(cond.repeat_interleave(M, 0)[chunk], ..., x_T=..., noise_seq=...) on the same rows.

        guidance_scale: as sample().  member_batch still counts fields; with guidance the network batch of a chunk is
        twice that."""
        return self._sample_ensemble(cond, members, device, steps, ddim_eta, member_batch, x_T, noise_seq, use_graph,
                                     False, solver=solver, spacing=spacing, guidance_scale=guidance_scale)

    def _n_vars(self, cond):
        """target variables of a sample: the network's n_vars (a model without one, e.g. a test double: cond's)"""
        net = getattr(self.model, "net", None)
        return int(getattr(net, "n_vars", cond.shape[1]))

    def _sample_ensemble(self, cond, members, device, steps, ddim_eta, member_batch, x_T, noise_seq, use_graph, paired,
                         solver="ddim", spacing=None, guidance_scale=None):
        """sample_ensemble(); paired: cond is two halves [cond, cond2] whose jobs b M + m get the same x_T and step
        noise (one chunk only: counterfactual_delta)"""
        if cond.ndim not in (4, 5):
            raise ValueError(f"cond must be [B, Cc, H, W] or [B, Cc, Fc, H, W], got {tuple(cond.shape)}")
        M = int(members)
        if M < 1:
            raise ValueError(f"members must be >= 1, got {members}")
        device = cond.device if device is None else torch.device(device)
        # V is the network's: cond carries cond_channels maps, which need not be V
        B, V, H, W = cond.shape[0], self._n_vars(cond), cond.shape[-2], cond.shape[-1]
        jobs = B * M
        mb = jobs if member_batch is None else int(member_batch)
        if mb < 1:
            raise ValueError(f"member_batch must be >= 1, got {member_batch}")
        if paired and mb < jobs:
            raise ValueError("paired ensembles run in one chunk")
        if x_T is not None and tuple(x_T.shape) != (B, M, V, H, W):
            raise ValueError(f"x_T must be {(B, M, V, H, W)}, got {tuple(x_T.shape)}")
        if noise_seq is not None and tuple(noise_seq.shape[1:]) != (B, M, V, H, W):
            raise ValueError(f"noise_seq must be [N, {B}, {M}, {V}, {H}, {W}], got {tuple(noise_seq.shape)}")
        if use_graph is None:
            use_graph = os.environ.get("CESM_SAMPLE_GRAPH", "1") != "0"
        self._sample_grid(steps, ddim_eta, solver, spacing)  # range checks before anything is captured
        check_guidance_scale(guidance_scale)
        eta = None if steps is None else float(ddim_eta)
        with torch.inference_mode():
            cond = cond.to(device)
            out = torch.empty((B, M, V, H, W), dtype=torch.float32, device=device)
            flat = out.view(jobs, V, H, W)
            xT = None if x_T is None else x_T.reshape(jobs, V, H, W)
            ns = None if noise_seq is None else noise_seq.reshape(noise_seq.shape[0], jobs, V, H, W)
            captured = {}  # chunk size -> GraphSampleStep
            for j0 in range(0, jobs, mb):
                j1 = min(j0 + mb, jobs)
                n = j1 - j0
                c = cond[torch.arange(j0, j1, device=device) // M]
                step = None
                if use_graph:
                    step = captured.get(n)
                    if step is None:
                        step = captured[n] = GraphSampleStep(self, c, torch.zeros((n, V, H, W), device=device),
                                                             ddim_eta=eta, solver=solver,
                                                             guidance_scale=guidance_scale)
                x = self._sample(c, (n, V, H, W), device, use_graph, None if xT is None else xT[j0:j1],
                                 None if ns is None else ns[:, j0:j1], steps, ddim_eta, paired, step=step,
                                 solver=solver, spacing=spacing, guidance_scale=guidance_scale)
                flat[j0:j1].copy_(x)
            return out

    def _sample(self, cond, shape, device, use_graph, x_T, noise_seq, steps, ddim_eta, paired, step=None,
                solver="ddim", spacing=None, guidance_scale=None):
        """sample(); paired: the batch is two halves that get the same x_T and the same step noise (drawn for one
        half, copied to the other: counterfactual_delta).  step: a GraphSampleStep captured earlier for this batch
        size, ddim_eta, solver and guidance_scale (sample_ensemble); the graph path then loads cond and x_T into its
        static buffers instead of capturing a new one, and the result is that step's x buffer (valid until the step
        runs again).  guidance_scale: sample(); the guidance halves stay inside the steps, the paired halves are rows
        of the B-row batch."""
        tau, ddim_eta = self._sample_grid(steps, ddim_eta, solver, spacing)
        gs = check_guidance_scale(guidance_scale)
        if paired and shape[0] % 2:
            raise ValueError("paired sampling needs an even batch")

        def randn():
            if not paired:
                return torch.randn(shape, device=device)
            return torch.randn((shape[0] // 2, *shape[1:]), device=device).repeat(2, *([1] * (len(shape) - 1)))

        def fill(z):
            if paired:
                h = z.shape[0] // 2
                z[:h].normal_()
                z[h:].copy_(z[:h])
            else:
                z.normal_()

        with torch.inference_mode():
            B = shape[0]
            x = randn() if x_T is None else x_T.to(device).float().clone()
            if use_graph is None:
                use_graph = os.environ.get("CESM_SAMPLE_GRAPH", "1") != "0"
            if steps is not None:
                # executed step k: t = tau[-1-k] -> t_prev = tau[-2-k], -1 after tau[0]
                pairs = list(zip(reversed(tau), reversed([-1] + tau[:-1])))
                if solver == "dpmpp2m":
                    # the history of executed step k is step k-1's x0 estimate, taken at its t
                    lasts = [-1] + [tt for tt, _ in pairs[:-1]]
                    if not use_graph:
                        x0 = None
                        for (tt, tp), tl in zip(pairs, lasts):
                            tt, tp, tl = (torch.full((B,), v, device=device, dtype=torch.long) for v in (tt, tp, tl))
                            x, x0 = self.dpmpp_step(x, cond, tt, tp, tl, x0, guidance_scale=gs)
                        return x
                    if step is None:
                        step = GraphSampleStep(self, cond, x, ddim_eta=0.0, solver=solver, guidance_scale=gs)
                    else:
                        step.load(cond, x)
                    for (tt, tp), tl in zip(pairs, lasts):
                        step.run(tt, tp, tl)
                    return step.x
                noisy = ddim_eta > 0.0
                if not use_graph:
                    for k, (tt, tp) in enumerate(pairs):
                        t_tensor = torch.full((B,), tt, device=device, dtype=torch.long)
                        tp_tensor = torch.full((B,), tp, device=device, dtype=torch.long)
                        nz = None
                        if noisy and tp >= 0:
                            nz = noise_seq[k].to(device) if noise_seq is not None else randn()
                        x = self.ddim_step(x, cond, t_tensor, tp_tensor, ddim_eta, noise=nz, guidance_scale=gs)
                    return x
                if step is None:
                    step = GraphSampleStep(self, cond, x, ddim_eta=ddim_eta, guidance_scale=gs)
                else:
                    step.load(cond, x)
                for k, (tt, tp) in enumerate(pairs):
                    if noisy and tp >= 0:  # the last step's sigma is exactly 0: z stays as it is
                        if noise_seq is not None:
                            step.z.copy_(noise_seq[k])
                        else:
                            fill(step.z)
                    step.run(tt, tp)
                return step.x
            if not use_graph:
                for i, tt in enumerate(reversed(range(self.T))):
                    t_tensor = torch.full((B,), tt, device=device, dtype=torch.long)
                    nz = None if noise_seq is None or tt == 0 else noise_seq[i].to(device)
                    if paired and nz is None and tt != 0:
                        nz = randn()
                    x = self.p_sample(x, cond, t_tensor, noise=nz, guidance_scale=gs)
                return x
            if step is None:
                step = GraphSampleStep(self, cond, x, guidance_scale=gs)
            else:
                step.load(cond, x)
            for i, tt in enumerate(reversed(range(self.T))):
                if tt == 0:
                    step.z.zero_()
                elif noise_seq is not None:
                    step.z.copy_(noise_seq[i])
                else:
                    fill(step.z)
                step.run(tt)
            return step.x


class GraphSampleStep:
    """One DDPM sampling step (model eval + fused update, in place on a static x) captured as a HIP graph
    (torch.cuda.graph drives hipStreamBeginCapture; every kernel launches on the capturing stream).
    Static inputs: x [B,V,H,W] fp32 (updated in place), cond, t [B] int64, z (step noise; zero at t=0,
    where posterior_variance[0] = 0 makes the noise term vanish as in the reference's t=0 branch).

    ddim_eta=None is that DDPM step.  With ddim_eta >= 0 the captured update is the generalized DDIM step instead
    (Diffusion.ddim_step): t_prev [B] int64 is a further static input, run(tt, tt_prev) sets both, and z exists only
    for ddim_eta > 0 (None at 0: the graph holds no noise buffer).

    solver="dpmpp2m" (ddim_eta None or 0) captures the DPM-Solver++(2M) step (Diffusion.dpmpp_step) in place on x and
    on a static history buffer x0_last, which every replay overwrites with its x0 estimate: t_prev and t_last are
    static inputs, run(tt, tt_prev, tt_last) sets all three, and there is no noise buffer.  A step with tt_last = -1
    does not read the history, so load() leaves it as it is.

    guidance_scale (None or 1.0: everything above, unchanged) captures the guided step instead: the step owns
    x2 [2B, ...], cond2 [2B, ...] and t2 [2B]; x, cond and t are their leading-B views, so callers read step.x as ever.
    The network runs once on the 2B rows and the guided update kernel writes x_prev into both halves of x2.  cond2's
    second half (the null condition) is zero from construction and never written again; load() writes x into both
    halves; z, x0_last, t_prev and t_last stay B-sized.  The scale is passed by value and fixed at capture."""

    def __init__(self, diffusion, cond, x, ddim_eta=None, solver="ddim", guidance_scale=None):
        self.d = diffusion
        self.scale = check_guidance_scale(guidance_scale)
        if solver not in ("ddim", "dpmpp2m"):
            raise ValueError(f"solver must be 'ddim' or 'dpmpp2m', got {solver!r}")
        self.multistep = solver == "dpmpp2m"
        if self.multistep:
            if ddim_eta is not None and float(ddim_eta) != 0.0:
                raise ValueError(f"solver='dpmpp2m' is deterministic: ddim_eta must be None or 0, got {ddim_eta}")
            ddim_eta = 0.0
        self.eta = None if ddim_eta is None else float(ddim_eta)
        if self.eta is not None and not self.eta >= 0.0:
            raise ValueError(f"ddim_eta must be >= 0, got {ddim_eta}")
        if self.scale is None:
            self.x = x.float().contiguous()
            self.cond = cond.float().contiguous()
            self.t = torch.zeros(x.shape[0], dtype=torch.long, device=x.device)
            self.x2 = self.cond2 = self.t2 = None
        else:
            B = x.shape[0]
            x, cond = x.float(), cond.to(x.device).float()
            self.x2 = torch.cat([x, x], dim=0)
            self.cond2 = torch.cat([cond, torch.zeros_like(cond)], dim=0)
            self.t2 = torch.zeros(2 * B, dtype=torch.long, device=x.device)
            self.x, self.cond, self.t = self.x2[:B], self.cond2[:B], self.t2[:B]
        self.t_prev = None if self.eta is None else torch.full_like(self.t, -1)
        self.t_last = torch.full_like(self.t, -1) if self.multistep else None
        self.x0_last = torch.zeros_like(self.x) if self.multistep else None
        self.z = torch.zeros_like(self.x) if self.eta is None or self.eta > 0.0 else None
        x0 = self.x.clone()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):  # warm-up: weight packs, lazily built tables, allocator pools
            for _ in range(2):
                self._step()
        torch.cuda.current_stream().wait_stream(side)
        self._put_x(x0)
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            self._step()

    def load(self, cond, x):
        """copy a new cond and a new state x into the static buffers: the captured graph then steps them (shapes as at
        capture)"""
        if tuple(x.shape) != tuple(self.x.shape) or tuple(cond.shape) != tuple(self.cond.shape):
            raise ValueError(f"GraphSampleStep captured for x {tuple(self.x.shape)} and cond {tuple(self.cond.shape)}, "
                             f"got {tuple(x.shape)} and {tuple(cond.shape)}")
        self._put_x(x)
        self.cond.copy_(cond)

    def _put_x(self, x):
        self.x.copy_(x)
        if self.scale is not None:
            self.x2[self.x.shape[0]:].copy_(x)

    def _step_guided(self):
        d, s = self.d, self.scale
        eps = d.model(self.x2, self.cond2, self.t2).float().contiguous()
        if self.eta is None:
            K.ddpm_step_cfg(self.x2, eps, self.z, self.t, *d._coefs(), s, out=self.x2)
        elif self.multistep:
            K.dpmpp_step_cfg(self.x2, eps, self.x0_last, self.t, self.t_prev, self.t_last, d.alphas_cumprod, s,
                             out=self.x2, x0_out=self.x0_last)
        else:
            K.ddim_step_cfg(self.x2, eps, self.z, self.t, self.t_prev, d.alphas_cumprod, self.eta, s, out=self.x2)

    def _step(self):
        if self.scale is not None:
            return self._step_guided()
        eps = self.d.model(self.x, self.cond, self.t).float().contiguous()
        if self.eta is None:
            K.ddpm_step(self.x, eps, self.z, self.t, *self.d._coefs(), out=self.x)
        elif self.multistep:
            K.dpmpp_step(self.x, eps, self.x0_last, self.t, self.t_prev, self.t_last, self.d.alphas_cumprod, out=self.x,
                         x0_out=self.x0_last)
        else:
            K.ddim_step(self.x, eps, self.z, self.t, self.t_prev, self.d.alphas_cumprod, self.eta, out=self.x)

    def run(self, tt, tt_prev=None, tt_last=None):
        """one step at time index tt for every sample; a DDIM step also needs its target tt_prev (-1 <= tt_prev < tt),
        a DPM-Solver++(2M) step also the previous step's time index tt_last (-1: none, else tt < tt_last < T)"""
        if (tt_prev is None) != (self.t_prev is None):
            raise ValueError("run(tt) is the DDPM step, run(tt, tt_prev) the DDIM step (ddim_eta given)")
        if (tt_last is None) != (self.t_last is None):
            raise ValueError("run(tt, tt_prev, tt_last) is the DPM-Solver++(2M) step (solver='dpmpp2m')")
        if not 0 <= tt < self.d.T or (tt_prev is not None and not -1 <= tt_prev < tt):
            raise ValueError(f"step indices out of range: t = {tt}, t_prev = {tt_prev}, T = {self.d.T}")
        if tt_last is not None and not (tt_last == -1 or tt < tt_last < self.d.T):
            raise ValueError(f"step indices out of range: t = {tt}, t_last = {tt_last}, T = {self.d.T}")
        (self.t if self.scale is None else self.t2).fill_(tt)
        if tt_prev is not None:
            self.t_prev.fill_(tt_prev)
        if tt_last is not None:
            self.t_last.fill_(tt_last)
        self.graph.replay()
