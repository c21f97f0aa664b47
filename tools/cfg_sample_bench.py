"""Cost of classifier-free guidance on the HIP-graph sampling path: whole N-step runs of a captured GraphSampleStep,
unguided (network batch B) against guidance_scale=s (network batch 2 B, the guided update kernel), alternating in one
process so that both see the same load of the box.  Per solver the two steps are captured once and warmed up; every
timed run reloads the same x_T (outside the timed window) and replays the solver's N steps between two device events,
ending in a synchronise.  Prints one JSON line per solver: ms per run and per step (mean, min, max), fields/s, and the
guided / unguided ratio -- 2 would be the cost of two separate unguided runs.
Random weights: the numbers are times, not sample quality (eps(x, 0) of an untrained network means nothing).
usage: python tools/cfg_sample_bench.py [--config more_blocks] [--batch 16] [--scale 2.0] [--rounds 5] [--dtype bf16]
                                        [--runs ddim:50,dpmpp2m:10]"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cesm_emulator_amd.model import Diffusion, GraphSampleStep  # noqa: E402
from cesm_emulator_amd.train import build_model_from_config  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="more_blocks")
    ap.add_argument("--batch", type=int, default=16, help="fields per run (the guided network batch is twice that)")
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp32"])
    ap.add_argument("--height", type=int, default=192)
    ap.add_argument("--width", type=int, default=288)
    ap.add_argument("--scale", type=float, default=2.0)
    ap.add_argument("--rounds", type=int, default=5, help="timed runs of each variant, alternating")
    ap.add_argument("--runs", default="ddim:50,dpmpp2m:10", help="solver:steps,...")
    a = ap.parse_args()
    dev = torch.device("cuda")
    cfg = json.load(open(os.path.join(ROOT, "config", a.config)))
    torch.manual_seed(1)
    net = build_model_from_config(cfg["unet"]).to(dev)
    net.compute_dtype = torch.bfloat16 if a.dtype == "bf16" else torch.float32
    d = Diffusion(net).to(dev)
    B, H, W = a.batch, a.height, a.width
    cond = torch.randn(B, 1, H, W, device=dev)
    x_T = torch.randn(B, 1, H, W, device=dev)
    for item in a.runs.split(","):
        solver, n = item.split(":")
        n = int(n)
        tau = d.sample_schedule(n, "logsnr" if solver == "dpmpp2m" else "uniform")
        pairs = list(zip(reversed(tau), reversed([-1] + tau[:-1])))
        if solver == "dpmpp2m":
            lasts = [-1] + [tt for tt, _ in pairs[:-1]]
            args = [(tt, tp, tl) for (tt, tp), tl in zip(pairs, lasts)]
        else:
            args = pairs
        with torch.inference_mode():
            steps = {"unguided": GraphSampleStep(d, cond, x_T.clone(), ddim_eta=0.0, solver=solver),
                     "guided": GraphSampleStep(d, cond, x_T.clone(), ddim_eta=0.0, solver=solver,
                                               guidance_scale=a.scale)}

            def run(step):
                step.load(cond, x_T)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record()
                for ar in args:
                    step.run(*ar)
                e1.record()
                e1.synchronize()
                return e0.elapsed_time(e1)

            for step in steps.values():  # warm-up of each captured graph
                run(step)
            ms = {k: [] for k in steps}
            for _ in range(a.rounds):
                for k, step in steps.items():
                    ms[k].append(run(step))
            assert all(torch.isfinite(s.x).all() for s in steps.values())
        out = {"metric": "guided vs unguided graph sampling", "config": a.config, "fields": B, "grid": [H, W],
               "dtype": a.dtype, "solver": solver, "sample_steps": n, "guidance_scale": a.scale, "rounds": a.rounds}
        for k, v in ms.items():
            mean = sum(v) / len(v)
            out[k] = {"network_batch": B if k == "unguided" else 2 * B, "ms_per_run": round(mean, 2),
                      "ms_per_run_min_max": [round(min(v), 2), round(max(v), 2)], "ms_per_step": round(mean / n, 4),
                      "fields_per_s": round(B / (mean * 1e-3), 3)}
        out["guided_over_unguided"] = round(sum(ms["guided"]) / sum(ms["unguided"]), 4)
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
