"""DDPM sampling throughput (inference.py:225-230 -> Diffusion.sample): one p_sample
step = F=1 forward of the full 192x288 grid + the fused update.  Times K steps of the eager loop
(model.py:186-194 semantics, one Python-driven launch sequence per step) and of the HIP-graph replay
(GraphSampleStep), and prints one JSON line.
--sample-steps N (with --eta) also times whole few-step calls Diffusion.sample(..., steps=N, ddim_eta=eta) end to end
-- graph capture and its warm-up forwards included, as every call pays them -- after one untimed call, and adds
ms_per_field / fields_per_s of such a call plus the call's fixed part (GraphSampleStep construction) to the line;
N = 0 times the full ancestral loop (steps=None) the same way.
usage: python tools/sample_bench.py [--config more_blocks] [--batch 8] [--steps 50] [--dtype bf16]
                                    [--sample-steps N [--eta 0.0] [--calls 3]]"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cesm_emulator_amd.model import Diffusion, GraphSampleStep  # noqa: E402
from cesm_emulator_amd.train import build_model_from_config  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="more_blocks")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp32"])
    ap.add_argument("--height", type=int, default=192)
    ap.add_argument("--width", type=int, default=288)
    ap.add_argument("--sample-steps", type=int, default=None,
                    help="time whole sample(steps=N) calls; 0 = the full ancestral loop (steps=None)")
    ap.add_argument("--eta", type=float, default=0.0, help="ddim_eta of the --sample-steps calls")
    ap.add_argument("--calls", type=int, default=3, help="timed sample() calls of --sample-steps")
    a = ap.parse_args()
    dev = torch.device("cuda")
    cfg = json.load(open(os.path.join(ROOT, "config", a.config)))
    torch.manual_seed(1)
    net = build_model_from_config(cfg["unet"]).to(dev)
    net.compute_dtype = torch.bfloat16 if a.dtype == "bf16" else torch.float32
    d = Diffusion(net).to(dev)
    B, H, W = a.batch, a.height, a.width
    cond = torch.randn(B, 1, H, W, device=dev)
    x = torch.randn(B, 1, H, W, device=dev)
    out = {"metric": "DDPM sampling steps/s (p_sample, F=1)", "config": a.config, "batch": B, "grid": [H, W],
           "dtype": a.dtype}
    with torch.inference_mode():
        # eager loop (reference control flow: host-side t tensor, randn_like, p_sample)
        for _ in range(3):
            x = d.p_sample(x, cond, torch.full((B,), 500, device=dev, dtype=torch.long))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(a.steps):
            x = d.p_sample(x, cond, torch.full((B,), 999 - i, device=dev, dtype=torch.long))
        torch.cuda.synchronize()
        te = (time.perf_counter() - t0) / a.steps
        step = GraphSampleStep(d, cond, x)
        for _ in range(3):
            step.z.normal_()
            step.run(500)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(a.steps):
            step.z.normal_()
            step.run(999 - i)
        torch.cuda.synchronize()
        tg = (time.perf_counter() - t0) / a.steps
        assert torch.isfinite(step.x).all()
    out.update({"eager_ms_per_step": round(te * 1e3, 3), "graph_ms_per_step": round(tg * 1e3, 3),
                "graph_speedup": round(te / tg, 2), "graph_steps_per_s": round(1.0 / tg, 2),
                "fields_per_s_1000_steps": round(B / (1000 * tg), 4)})
    if a.sample_steps is not None:
        n = a.sample_steps if a.sample_steps > 0 else None
        eta = a.eta if n is not None else None

        def timed(fn, reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(reps):
                y = fn()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / reps, y

        def one_call():
            return d.sample(cond, (B, 1, H, W), dev, use_graph=True, steps=n, ddim_eta=a.eta)

        one_call()  # untimed: weight packs, allocator pools
        tc, y = timed(one_call, a.calls)
        assert torch.isfinite(y).all()
        # the part of a call that does not scale with the step count: warm-up forwards + capture
        with torch.inference_mode():
            tf, _ = timed(lambda: GraphSampleStep(d, cond, x.clone(), ddim_eta=eta), a.calls)
        out.update({"sample_steps": n if n is not None else d.T, "eta": eta, "sample_calls": a.calls,
                    "ms_per_call": round(tc * 1e3, 2), "ms_per_field": round(tc * 1e3 / B, 3),
                    "fields_per_s": round(B / tc, 3), "fixed_ms_per_call": round(tf * 1e3, 2),
                    "fixed_fraction": round(tf / tc, 4)})
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
