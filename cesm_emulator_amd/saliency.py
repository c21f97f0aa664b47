"""Input gradients of the diffusion loss: which emissions (cond) and which noisy state (x_t) the prediction
depends on.  The reference computes |d loss / d cond| during validation (train.py saliency_wrt_cond, plotted by
quad_with_saliency); here the backward runs through the HIP network's dX chain and ends in the stem's data gradient
(csrc/stem_dgrad.h; csrc/multivar.h for several target variables), with every weight gradient left out.

Both helpers leave the model as found: no p.grad is created or changed, no requires_grad flag is touched; they work on
trainable and on frozen (checkpoint.load_checkpoint) models, in either compute_dtype.  A plain loss.backward() with
cond.requires_grad_(True) gives the same cond.grad, and accumulates parameter gradients as every backward does.
"""
from __future__ import annotations

import torch

from .model import _CondMask, _MSE
from .video_net import input_grads_only


def input_grads(diffusion, x0, cond, t=None, noise=None, keep=None):
    """(loss, d loss / d x_t, d loss / d cond) of the eps-prediction MSE at x_t = q_sample(x0, t, noise).
    x0 [B,V,H,W]; cond [B,Cc,H,W] (F = 1) or a window [B,Cc,F,H,W] (Cc = the model's cond_channels, V by default); t
    defaults to T // 2 for every sample.  The
    gradients have x_t's (= x0's) and cond's shapes and are fp32; loss is detached.  keep (bool [B], the condition
    dropout of Diffusion.loss): the samples with keep False see the null condition, and their d cond is exactly zero;
    nothing is drawn here, whatever the diffusion's p_uncond."""
    B = x0.size(0)
    if t is None:
        t = torch.full((B,), diffusion.T // 2, device=x0.device, dtype=torch.long)
    with torch.enable_grad():
        x_t, noise = diffusion.q_sample(x0.detach(), t, noise)
        x_req = x_t.detach().requires_grad_(True)
        cond_req = cond.detach().clone().requires_grad_(True)
        cond_in = cond_req
        if keep is not None:
            keep = torch.as_tensor(keep, dtype=torch.bool, device=x0.device).contiguous()
            if tuple(keep.shape) != (B,):
                raise ValueError(f"keep needs one entry per sample ({B}), got {tuple(keep.shape)}")
            cond_in = _CondMask.apply(cond_req.float().contiguous(), keep)
        eps = diffusion.model(x_req, cond_in, t)
        loss = _MSE.apply(eps, noise.float().contiguous())
        with input_grads_only():
            dxt, dcond = torch.autograd.grad(loss, (x_req, cond_req))
    return loss.detach(), dxt, dcond


def counterfactual_delta(diffusion, cond, scale_mask=None, scale=1.1, steps=None, ddim_eta=0.0, paired=False,
                         n_samples=1, solver="ddim", spacing=None, guidance_scale=None):
    """Sampled response to scaled emissions (the reference's train.py counterfactual_delta): sample(cond2) -
    sample(cond) with cond2 = cond * scale, or cond * (1 + (scale - 1) * scale_mask) where a mask is given.  steps,
    ddim_eta, solver, spacing and guidance_scale go to Diffusion.sample (steps=None: the full ancestral loop; with
    guidance the paired halves are rows of the batch and the guidance halves stay inside the steps).

    Default: two sampling runs, base first, each drawing its own x_T and step noise (the reference's semantics), so
    the difference also carries the sampling noise.  paired=True: ONE run of batch 2B over [cond, cond2] in which both
    halves get the same x_T and the same step noise (drawn for B samples, copied to the other half); the difference
    then isolates the change in cond.

    n_samples = n > 1 (the reference's _mean_of_samples): the mean over n members of the perturbed ensemble minus that
    of the base ensemble, both drawn with Diffusion.sample_ensemble (base first).  With paired=True the two ensembles
    are one run over [cond, cond2] in which member m of both gets the same x_T and the same step noise.  n_samples = 1
    is the code path above, unchanged."""
    n_samples = int(n_samples)
    if n_samples < 1:
        raise ValueError(f"n_samples must be >= 1, got {n_samples}")
    cond2 = cond * scale if scale_mask is None else cond * (1.0 + (scale - 1.0) * scale_mask)
    # V target variables: the network's (cond carries cond_channels maps, which need not be V)
    B, V, H, W = cond.shape[0], diffusion._n_vars(cond), cond.shape[-2], cond.shape[-1]
    kw = dict(solver=solver, spacing=spacing, guidance_scale=guidance_scale)
    if n_samples > 1:
        if paired:
            x = diffusion._sample_ensemble(torch.cat([cond, cond2], dim=0), n_samples, cond.device, steps, ddim_eta,
                                           None, None, None, None, True, **kw)
            return x[B:].mean(dim=1) - x[:B].mean(dim=1)
        base = diffusion.sample_ensemble(cond, n_samples, steps=steps, ddim_eta=ddim_eta, **kw).mean(dim=1)
        pert = diffusion.sample_ensemble(cond2, n_samples, steps=steps, ddim_eta=ddim_eta, **kw).mean(dim=1)
        return pert - base
    if paired:
        x = diffusion._sample(torch.cat([cond, cond2], dim=0), (2 * B, V, H, W), cond.device, None, None, None, steps,
                              ddim_eta, True, **kw)
        return x[B:] - x[:B]
    base = diffusion.sample(cond, (B, V, H, W), cond.device, steps=steps, ddim_eta=ddim_eta, **kw)
    pert = diffusion.sample(cond2, (B, V, H, W), cond.device, steps=steps, ddim_eta=ddim_eta, **kw)
    return pert - base


def saliency_wrt_cond(diffusion, x0, cond, t=None, noise=None, normalize=True, keep=None):
    """|d loss / d cond| in cond's shape (the reference's train.py saliency_wrt_cond); with normalize, every sample's
    map(s) divided by its spatial maximum + 1e-8.  keep: as input_grads (a dropped sample's map is all zero)."""
    g = input_grads(diffusion, x0, cond, t, noise, keep=keep)[2].abs()
    if normalize:
        g = g / (g.amax(dim=(-2, -1), keepdim=True) + 1e-8)
    return g
