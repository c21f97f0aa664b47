"""Discretisation error of the few-step samplers with the real network: relative L2 distance of
Diffusion.sample(steps=N, solver=, spacing=) from the same seed's 1000-step DDIM run on the uniform grid, for the four
solver x spacing combinations and N in --steps-list.  The network is the config's UNet at its random initial weights
(seed 1), fp32 compute, B = 2 on a 64x96 grid, with one fixed cond and x_T: every run is deterministic (ddim_eta = 0),
so the only difference between two runs is the step rule and the time grid.  tests/test_dpmpp_host.py has the same
table for an analytic Gaussian score in float64; this one answers whether the network's eps behaves like it, and
whether "logsnr" is the right default grid for dpmpp2m.  Prints a markdown table and one JSON line.
usage: python tools/sampler_convergence.py [--config more_blocks] [--batch 2] [--height 64] [--width 96]
                                           [--ref-steps 1000] [--steps-list 5 10 20 40] [--dtype fp32]"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cesm_emulator_amd.model import Diffusion  # noqa: E402
from cesm_emulator_amd.train import build_model_from_config  # noqa: E402

COMBOS = [("ddim", "uniform"), ("ddim", "logsnr"), ("dpmpp2m", "uniform"), ("dpmpp2m", "logsnr")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="more_blocks")
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--height", type=int, default=64)
    ap.add_argument("--width", type=int, default=96)
    ap.add_argument("--ref-steps", type=int, default=1000)
    ap.add_argument("--steps-list", type=int, nargs="+", default=[5, 10, 20, 40])
    ap.add_argument("--dtype", default="fp32", choices=["bf16", "fp32"])
    a = ap.parse_args()
    dev = torch.device("cuda")
    cfg = json.load(open(os.path.join(ROOT, "config", a.config)))
    torch.manual_seed(1)
    net = build_model_from_config(cfg["unet"]).to(dev)
    net.compute_dtype = torch.bfloat16 if a.dtype == "bf16" else torch.float32
    d = Diffusion(net).to(dev)
    shape = (a.batch, 1, a.height, a.width)
    g = torch.Generator().manual_seed(2)
    cond = torch.randn(shape, generator=g).to(dev)
    x_T = torch.randn(shape, generator=g).to(dev)

    def run(steps, solver, spacing):
        y = d.sample(cond, shape, dev, use_graph=True, x_T=x_T, steps=steps, solver=solver, spacing=spacing)
        assert torch.isfinite(y).all(), (steps, solver, spacing)
        return y.double()

    ref = run(a.ref_steps, "ddim", "uniform")
    rn = torch.linalg.vector_norm(ref)
    err = {}
    print(f"relative L2 error against {a.ref_steps} DDIM steps (uniform grid), {a.config} at random initial weights, "
          f"{a.dtype}, {a.batch}x1x{a.height}x{a.width}")
    print("| N | " + " | ".join(f"{s}, {p}" for s, p in COMBOS) + " |")
    print("|---|" + "---|" * len(COMBOS))
    for n in a.steps_list:
        for s, p in COMBOS:
            err[f"{n}/{s}/{p}"] = (torch.linalg.vector_norm(run(n, s, p) - ref) / rn).item()
        print(f"| {n} | " + " | ".join(f"{err[f'{n}/{s}/{p}']:.4f}" for s, p in COMBOS) + " |", flush=True)
    print(json.dumps({"metric": "relative L2 error of few-step sampling vs the reference run", "config": a.config,
                      "dtype": a.dtype, "shape": list(shape), "ref_steps": a.ref_steps,
                      "ref_rms": (rn / ref.numel() ** 0.5).item(), "err": err}), flush=True)


if __name__ == "__main__":
    main()
