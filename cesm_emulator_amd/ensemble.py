"""Ensemble verification: how good is a sampled ensemble against the held-out truth?

The model emulates a large ensemble; Diffusion.sample_ensemble draws M members per condition.  This module judges
them with the standard measures, all from ONE kernel pass over the [B, M, V, H, W] ensemble (kernels.ens_stats,
csrc/ensemble.hip; the per-pixel contract is in include/cesm_hip.h):

  mse / rmse   of the ensemble mean against obs,            var / spread = sqrt(var)   mean ensemble variance,
  ssr          spread / skill = sqrt((M + 1) / M * var / mse)   (1 for a reliable ensemble; Fortin et al. 2014),
  crps         fair CRPS (Ferro 2014),                      rank_hist [V, M + 1]   rank of obs among the members,

every one an area-weighted mean over the grid: row weights model.latitude_weights(lat) of the FULL grid's latitudes,
crop row offsets row0 as for the weighted loss (uniform weights of 1 without lat).  The sums live in a float64
[V, 4 + M + 1] accumulator on the device; EnsembleVerifier keeps one across batches without a host synchronisation.
"""
from __future__ import annotations

import torch

from . import kernels as K
from .model import check_row0, latitude_weights

SCALARS = ("mse", "rmse", "var", "spread", "ssr", "crps", "rank_hist")


def norm_scale(norm):
    """summarize()'s scale from normalisation statistics (data.load_fields' norm; None passes through)"""
    return None if norm is None else norm["target_std"]


def summarize(acc, members, has_obs=True, scale=None):
    """The per-variable scalars of an accumulator acc [V, 4 + M + 1] (float64; columns: sum w, sum w (mean - obs)^2,
    sum w var, sum w crps, sum w [rank = r] for r = 0 .. M), as float64 tensors on acc's device: mse, rmse, var, spread,
    ssr, crps are [V]; rank_hist [V, M + 1] holds weighted fractions that sum to 1.  has_obs=False: only var and spread
    are formed, the others are None.  scale [V] (the variables' target_std): results in physical units -- rmse, spread
    and crps times scale[v], mse and var times scale[v]^2; ssr and rank_hist have no unit and stay."""
    M = int(members)
    if acc.ndim != 2 or acc.shape[1] != 4 + M + 1:
        raise ValueError(f"acc must be [V, {4 + M + 1}] for {M} members, got {tuple(acc.shape)}")
    acc = acc.double()
    sw = acc[:, 0]
    var = acc[:, 2] / sw
    out = dict.fromkeys(SCALARS)
    out["var"], out["spread"] = var, var.sqrt()
    if has_obs:
        mse = acc[:, 1] / sw
        hist = acc[:, 4:]
        out.update(mse=mse, rmse=mse.sqrt(), crps=acc[:, 3] / sw, ssr=((M + 1) / M * var / mse).sqrt(),
                   rank_hist=hist / hist.sum(dim=1, keepdim=True))
    if scale is not None:
        sc = torch.as_tensor(scale, dtype=torch.float64, device=acc.device).reshape(-1)
        if sc.numel() != acc.shape[0]:
            raise ValueError(f"scale must have one entry per variable ({acc.shape[0]}), got {sc.numel()}")
        for k, f in (("rmse", sc), ("spread", sc), ("crps", sc), ("mse", sc * sc), ("var", sc * sc)):
            if out[k] is not None:
                out[k] = out[k] * f
    return out


def row_weights(lat, H, device):
    """fp32 row weights [Hg] on `device`: latitude_weights(lat) for full-grid latitudes, ones(H) without"""
    if lat is None:
        return torch.ones(H, dtype=torch.float32, device=device)
    w = latitude_weights(lat)
    if w.numel() < H:
        raise ValueError(f"lat has {w.numel()} rows, the ensemble {H}")
    return w.to(device)


def ensemble_stats(ens, obs=None, lat=None, row0=None, maps=True):
    """Maps and area-weighted scalars of one ensemble, one kernel call.  ens [B, M, V, H, W] fp32 on the GPU (a
    [B * M, V, H, W] sampler batch viewed), obs [B, V, H, W] or None, lat: latitudes in degrees of the full grid's rows
    (None: uniform weights of 1, the tensor is the whole grid), row0: grid row of each condition's row 0 (a list or CPU
    tensor is range-checked, a device tensor is not read back; None: 0).

    Returns a dict: the scalars of summarize(), "acc" (the raw accumulator) and "maps": None with maps=False, else
    {"mean", "var"} (fp32) and, with obs, {"crps" (fp32), "rank" (int32)} (None without), each [B, V, H, W]."""
    if not torch.is_tensor(ens) or ens.ndim != 5:
        raise RuntimeError("shape mismatch: ens must be [B, M, V, H, W]")
    B, M, V, H, W = ens.shape
    w = row_weights(lat, H, ens.device)
    row0 = check_row0(row0, B, H, w.numel(), ens.device, has_lat=lat is not None)
    maps = bool(maps)
    has_obs = obs is not None
    r = K.ens_stats(ens, obs, w, row0, mean=maps, var=maps, crps=maps and has_obs, rank=maps and has_obs, acc=True)
    out = summarize(r["acc"], M, has_obs)
    out["acc"] = r["acc"]
    out["maps"] = {k: r[k] for k in ("mean", "var", "crps", "rank")} if maps else None
    return out


class EnsembleVerifier:
    """Running verification over many batches: update(ens, obs, row0) adds a batch into one float64 device buffer (one
    kernel call, no host synchronisation), result() gives summarize() over everything seen, reset() clears it."""

    def __init__(self, members, n_vars, lat=None, device="cuda"):
        self.members, self.n_vars = int(members), int(n_vars)
        if not K.ENS_MIN_M <= self.members <= K.ENS_MAX_M:
            raise ValueError(f"members must be in {K.ENS_MIN_M} .. {K.ENS_MAX_M}, got {members}")
        if self.n_vars < 1:
            raise ValueError(f"n_vars must be >= 1, got {n_vars}")
        self.lat = None if lat is None else torch.as_tensor(lat, dtype=torch.float64, device="cpu").reshape(-1)
        self.device = torch.device(device)
        self.acc = torch.zeros(self.n_vars, 4 + self.members + 1, dtype=torch.float64, device=self.device)
        self._w = {}  # H -> row weights

    def _weights(self, H):
        key = H if self.lat is None else -1
        if key not in self._w:
            self._w[key] = row_weights(self.lat, H, self.device)
        w = self._w[key]
        if w.numel() < H:
            raise ValueError(f"lat has {w.numel()} rows, the ensemble {H}")
        return w

    def update(self, ens, obs, row0=None):
        if not torch.is_tensor(ens) or ens.ndim != 5 or ens.shape[1] != self.members or ens.shape[2] != self.n_vars:
            raise RuntimeError(f"shape mismatch: ens must be [B, {self.members}, {self.n_vars}, H, W]")
        if obs is None:
            raise ValueError("verification needs obs")
        B, H = ens.shape[0], ens.shape[3]
        w = self._weights(H)
        row0 = check_row0(row0, B, H, w.numel(), ens.device, has_lat=self.lat is not None)
        K.ens_stats(ens, obs, w, row0, mean=False, var=False, crps=False, rank=False, acc=self.acc, accumulate=True)

    def result(self, norm=None):
        """summarize() over everything seen; norm (data.load_fields' statistics): in physical units"""
        return summarize(self.acc, self.members, scale=norm_scale(norm))

    def reset(self):
        self.acc.zero_()
