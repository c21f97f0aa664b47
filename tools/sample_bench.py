"""DDPM sampling throughput (inference.py:225-230 -> Diffusion.sample): one p_sample
step = F=1 forward of the full 192x288 grid + the fused update.  Times K steps of the eager loop
(model.py:186-194 semantics, one Python-driven launch sequence per step) and of the HIP-graph replay
(GraphSampleStep), and prints one JSON line.
--sample-steps N (with --eta) also times whole few-step calls Diffusion.sample(..., steps=N, ddim_eta=eta) end to end
-- graph capture and its warm-up forwards included, as every call pays them -- after one untimed call, and adds
ms_per_field / fields_per_s of such a call plus the call's fixed part (GraphSampleStep construction) to the line;
N = 0 times the full ancestral loop (steps=None) the same way.  --solver / --spacing go to those calls (dpmpp2m:
DPM-Solver++(2M), on the log-SNR grid unless --spacing says otherwise).  --versus SOLVER times the same calls with a
second solver in the same process, the two alternating call by call, and also the bare graph replay of one step of
each (blocks of --steps replays, alternating), so that the two are compared under the same load of the box: the line
then carries min / max of every timing for both, the second solver's under "versus".
usage: python tools/sample_bench.py [--config more_blocks] [--batch 8] [--steps 50] [--dtype bf16]
                                    [--sample-steps N [--eta 0.0] [--calls 3] [--solver ddim] [--spacing S]
                                     [--versus SOLVER]]"""
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
    ap.add_argument("--solver", default="ddim", choices=["ddim", "dpmpp2m"], help="solver of the --sample-steps calls")
    ap.add_argument("--spacing", default=None, choices=["uniform", "logsnr"],
                    help="time grid of the --sample-steps calls (default: the solver's)")
    ap.add_argument("--versus", default=None, choices=["ddim", "dpmpp2m"],
                    help="a second solver, timed alternately with --solver (needs --sample-steps > 0)")
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
        if n is None and (a.solver != "ddim" or a.versus):
            ap.error("--solver dpmpp2m and --versus need --sample-steps > 0")
        solvers = [a.solver] + ([a.versus] if a.versus else [])

        def timed(fn, reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(reps):
                y = fn()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / reps, y

        def eta_of(solver):
            return None if n is None else (a.eta if solver == "ddim" else 0.0)

        def one_call(solver):
            return d.sample(cond, (B, 1, H, W), dev, use_graph=True, steps=n, ddim_eta=eta_of(solver) or 0.0,
                            solver=solver, spacing=a.spacing)

        def new_step(solver):
            return GraphSampleStep(d, cond, x.clone(), ddim_eta=eta_of(solver), solver=solver)

        tc, tf = {s: [] for s in solvers}, {s: [] for s in solvers}
        for s in solvers:
            one_call(s)  # untimed: weight packs, allocator pools
        for _ in range(a.calls):  # the solvers alternate call by call
            for s in solvers:
                t, y = timed(lambda: one_call(s), 1)
                assert torch.isfinite(y).all()
                tc[s].append(t)
                # the part of a call that does not scale with the step count: warm-up forwards + capture
                with torch.inference_mode():
                    tf[s].append(timed(lambda: new_step(s), 1)[0])

        def report(s):
            c, f = sum(tc[s]) / a.calls, sum(tf[s]) / a.calls
            r = {"solver": s if n is not None else "ddpm",
                 "spacing": None if n is None else a.spacing or ("logsnr" if s == "dpmpp2m" else "uniform"),
                 "sample_steps": n if n is not None else d.T, "eta": eta_of(s), "sample_calls": a.calls,
                 "ms_per_call": round(c * 1e3, 2), "ms_per_call_min_max": [round(min(tc[s]) * 1e3, 2),
                                                                           round(max(tc[s]) * 1e3, 2)],
                 "ms_per_field": round(c * 1e3 / B, 3), "fields_per_s": round(B / c, 3),
                 "fixed_ms_per_call": round(f * 1e3, 2), "fixed_fraction": round(f / c, 4)}
            if s in ts:
                r.update({"replay_ms_per_step": round(sum(ts[s]) / len(ts[s]) * 1e3, 4),
                          "replay_ms_per_step_min_max": [round(min(ts[s]) * 1e3, 4), round(max(ts[s]) * 1e3, 4)]})
            return r

        ts = {}
        if a.versus:  # one captured step of each solver, blocks of a.steps replays, alternating
            with torch.inference_mode():
                steps = {s: new_step(s) for s in solvers}
                args = {"ddim": (500, 480), "dpmpp2m": (500, 480, 520)}
                ts = {s: [] for s in solvers}
                for s in solvers:
                    timed(lambda: steps[s].run(*args[s]), 3)
                for _ in range(a.calls):
                    for s in solvers:
                        ts[s].append(timed(lambda: steps[s].run(*args[s]), a.steps)[0])
        out.update(report(a.solver))
        if a.versus:
            out["versus"] = report(a.versus)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
