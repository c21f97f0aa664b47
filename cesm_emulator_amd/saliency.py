"""Input gradients of the diffusion loss: which emissions (cond) and which noisy state (x_t) the prediction
depends on.  The reference computes |d loss / d cond| during validation (train.py saliency_wrt_cond, plotted by
quad_with_saliency); here the backward runs through the HIP network's dX chain and ends in the stem's data gradient
(csrc/stem_dgrad.h), with every weight gradient left out.

Both helpers leave the model as found: no p.grad is created or changed, no requires_grad flag is touched; they work on
trainable and on frozen (checkpoint.load_checkpoint) models, in either compute_dtype.  A plain loss.backward() with
cond.requires_grad_(True) gives the same cond.grad, and accumulates parameter gradients as every backward does.
"""
from __future__ import annotations

import torch

from .model import _MSE
from .video_net import input_grads_only


def input_grads(diffusion, x0, cond, t=None, noise=None):
    """(loss, d loss / d x_t, d loss / d cond) of the eps-prediction MSE at x_t = q_sample(x0, t, noise).
    x0 [B,1,H,W]; cond [B,1,H,W] (F = 1) or a window [B,1,F,H,W]; t defaults to T // 2 for every sample.  The
    gradients have x_t's (= x0's) and cond's shapes and are fp32; loss is detached."""
    B = x0.size(0)
    if t is None:
        t = torch.full((B,), diffusion.T // 2, device=x0.device, dtype=torch.long)
    with torch.enable_grad():
        x_t, noise = diffusion.q_sample(x0.detach(), t, noise)
        x_req = x_t.detach().requires_grad_(True)
        cond_req = cond.detach().clone().requires_grad_(True)
        eps = diffusion.model(x_req, cond_req, t)
        loss = _MSE.apply(eps, noise.float().contiguous())
        with input_grads_only():
            dxt, dcond = torch.autograd.grad(loss, (x_req, cond_req))
    return loss.detach(), dxt, dcond


def saliency_wrt_cond(diffusion, x0, cond, t=None, noise=None, normalize=True):
    """|d loss / d cond| in cond's shape (the reference's train.py saliency_wrt_cond); with normalize, every sample's
    map(s) divided by its spatial maximum + 1e-8."""
    g = input_grads(diffusion, x0, cond, t, noise)[2].abs()
    if normalize:
        g = g / (g.amax(dim=(-2, -1), keepdim=True) + 1e-8)
    return g
