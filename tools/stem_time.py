"""HIP-event timing of the stem for V target variables at the bench shape (B = 8, F = 12, 192 x 288, bf16, x_t one
frame, cond 12): stem_fwd and stem_wgrad at V = 1 (the single-variable kernels), 2 and 4 in one process, the V values
alternated over several rounds.  The yardstick is V x t(1) (the single-variable kernel run once per plane pair); the
fused kernels are asked to stay within 1.1 x that.  --step adds one whole bf16 training step of config/more_blocks
(ch_mults 1, 2, 4, 8) at V = 1 and V = 2.
--mc times the multi-forcing stem (cond_channels) instead: (V, Cc) = (1, 2), (1, 3), (1, 4), forward and weight gradient
+ reduce, each against the V' = ceil((V + Cc) / 2) kernel of the equal-count stem (which moves at least as many
planes), alternated in this process; asked to stay within 1.1 x.  With --step: one whole bf16 more_blocks training step
at (V, Cc) = (1, 1) and (1, 3), alternated.
usage: [CESM_HIP_LIB=...] python tools/stem_time.py [--mc] [--step] [--rounds N]"""
import argparse
import sys

import torch

sys.path.insert(0, ".")
from cesm_emulator_amd import kernels as K  # noqa: E402

B, F, H, W, CO, KS = 8, 12, 192, 288, 64, 7


def timed(fn, reps=20):
    fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps * 1e3


def stem_case(V, dev):
    g = torch.Generator().manual_seed(V)
    xt = torch.randn(B, V, 1, H, W, generator=g).to(dev)
    cond = torch.randn(B, V, F, H, W, generator=g).to(dev)
    w = (torch.randn(CO, 2 * V, 1, KS, KS, generator=g) * 0.05).to(dev)
    b = torch.randn(CO, generator=g).to(dev)
    dy = torch.randn(B * F, H, W, CO, device=dev).to(torch.bfloat16)
    dw = torch.zeros_like(w)
    return dict(fwd=lambda: K.stem_fwd(xt, cond, w, b, F, torch.bfloat16),
                wgrad=lambda: K.stem_wgrad(xt, cond, dy, dw, F, accumulate=False))


def mc_case(V, Cc, dev):
    g = torch.Generator().manual_seed(10 * V + Cc)
    xt = torch.randn(B, V, 1, H, W, generator=g).to(dev)
    cond = torch.randn(B, Cc, F, H, W, generator=g).to(dev)
    w = (torch.randn(CO, V + Cc, 1, KS, KS, generator=g) * 0.05).to(dev)
    b = torch.randn(CO, generator=g).to(dev)
    dy = torch.randn(B * F, H, W, CO, device=dev).to(torch.bfloat16)
    dw = torch.zeros_like(w)
    return dict(fwd=lambda: K.stem_fwd_mc(xt, cond, w, b, F, torch.bfloat16),
                wgrad=lambda: K.stem_wgrad_mc(xt, cond, dy, dw, F, accumulate=False))


def step_time(V, dev, steps=5, Cc=None):
    from cesm_emulator_amd.model import Diffusion, UNet
    from cesm_emulator_amd.train import make_optimizer, train_step
    torch.manual_seed(0)
    d = Diffusion(UNet(out_channels=V, ch_mults=(1, 2, 4, 8), cond_channels=Cc).to(dev)).to(dev)
    opt = make_optimizer(d, {})
    x0 = torch.randn(B, V, H, W, device=dev)
    cond = torch.randn(B, V if Cc is None else Cc, F, H, W, device=dev)
    for _ in range(2):
        train_step(d, opt, x0, cond)
    return timed(lambda: train_step(d, opt, x0, cond), reps=steps) / 1e3


def main_mc(a, dev):
    pairs = [(1, 2), (1, 3), (1, 4)]
    yard = {p: (sum(p) + 1) // 2 for p in pairs}
    cases = {p: mc_case(*p, dev) for p in pairs}
    cases.update({V: stem_case(V, dev) for V in sorted(set(yard.values()))})
    best = {}
    for r in range(a.rounds):
        for key, c in cases.items():
            for name, fn in c.items():
                t = timed(fn)
                best[(name, key)] = min(t, best.get((name, key), float("inf")))
                print(f"round {r} stem_{name} {key}: {t:.1f} us", flush=True)
    for name in ("fwd", "wgrad"):
        for p in pairs:
            t, ty = best[(name, p)], best[(name, yard[p])]
            print(f"stem_{name}: t(V={p[0]}, Cc={p[1]}) = {t:.1f} us, t_mv(V'={yard[p]}) = {ty:.1f} us, ratio "
                  f"{t / ty:.3f} ({'within' if t <= 1.1 * ty else 'OVER'} 1.1)", flush=True)
    if a.step:
        for Cc in (None, 3, None, 3):
            print(f"train step V=1 Cc={1 if Cc is None else Cc}: {step_time(1, dev, Cc=Cc):.2f} ms", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mc", action="store_true", help="time the multi-forcing stem against the equal-count kernels")
    ap.add_argument("--step", action="store_true", help="also time a whole training step at V = 1 and V = 2")
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    dev = torch.device("cuda")
    if a.mc:
        return main_mc(a, dev)
    cases = {V: stem_case(V, dev) for V in (1, 2, 4)}
    best = {}
    for r in range(a.rounds):
        for V, c in cases.items():
            for name, fn in c.items():
                t = timed(fn)
                best[(name, V)] = min(t, best.get((name, V), float("inf")))
                print(f"round {r} stem_{name} V={V}: {t:.1f} us", flush=True)
    for name in ("fwd", "wgrad"):
        t1 = best[(name, 1)]
        for V in (2, 4):
            t = best[(name, V)]
            print(f"stem_{name}: t({V}) = {t:.1f} us, {V} x t(1) = {V * t1:.1f} us, ratio {t / (V * t1):.3f} "
                  f"({'within' if t <= 1.1 * V * t1 else 'OVER'} 1.1)", flush=True)
    if a.step:
        for V in (1, 2, 1, 2):
            print(f"train step V={V}: {step_time(V, dev):.2f} ms", flush=True)


if __name__ == "__main__":
    main()
