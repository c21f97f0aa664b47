"""cesm_emulator_amd — MI355X-native (gfx950) drop-in for the video_net training hot path of
kallenordling/cesm_emulator: `model.UNet` / `model.Diffusion` surface, HIP kernels for every
network op and for the AdamW step, RCCL data parallelism, device-side training-window gather.
"""
from .model import UNet, Diffusion  # noqa: F401
from .optim import FusedAdamW  # noqa: F401
from .ema import EMA, ema_decay  # noqa: F401
from .saliency import counterfactual_delta, input_grads, saliency_wrt_cond  # noqa: F401
from .ensemble import EnsembleVerifier, ensemble_stats  # noqa: F401

__all__ = ["UNet", "Diffusion", "FusedAdamW", "EMA", "ema_decay", "input_grads", "saliency_wrt_cond", "counterfactual_delta",
           "EnsembleVerifier", "ensemble_stats"]
