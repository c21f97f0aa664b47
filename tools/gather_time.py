"""HIP-event timing of the window gathers at two shapes: B = 8, K = 12 on the full 192 x 288 grid, and B = 64, K = 3 on
64 x 64 crops.  At each, the existing cesm_window_gather (one variable,
consecutive windows) is t_old(1), and cesm_window_gather_mv is timed at V = 1, 2, 4 (Vc = V, the same consecutive
windows as explicit frame indices) -- one process, warm, library entry points called directly into preallocated
outputs, 20 launches per sample queued behind a kernel that holds the stream (see timed()), the variants alternated
over 5 rounds, median per variant.

The yardstick of the new kernel at V variables is the old kernel run once per variable, V x t_old(1), measured here in
the same process; the gate printed at the end is t_new(V) <= 1.1 x V x t_old(1).  The floor beside each time is reading
and writing every gathered element once at the 6.3 TB/s the MI355X achieves from HBM; these launches are expected to
be latency-bound, so the absolute time is recorded, not gated.  The V = 1 outputs of the two kernels are compared.
usage: [CESM_HIP_LIB=...] python tools/gather_time.py [--rounds N] [--reps N]"""
import argparse
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, ".")
from cesm_emulator_amd import kernels as K  # noqa: E402
from cesm_emulator_amd._lib import call  # noqa: E402

HBM = 6.3e12
HOLD_US = 1000.0  # longer than the host takes to enqueue one sample's launches
T, M, H, W = 16, 4, 192, 288
SHAPES = [("B=8 K=12 192x288", 8, 12, 192, 288), ("B=64 K=3 64x64", 64, 3, 64, 64)]
VS = (1, 2, 4)


def timed(fn, reps):
    """device time per launch of reps launches that are already queued when the first one starts: a kernel that idles
    on one CU for HOLD_US goes in first, so the event window holds the kernels back to back and not the host's enqueue
    rate (a ctypes call takes about as long as one of the small launches runs)"""
    fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    call("cesm_hold_cus", 1, HOLD_US, K.S())
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps * 1e3


def items_for(rng, B, Kw, h, w):
    """consecutive windows in both forms: item rows (t0, m, anchor, rev = 0, i, j) and (times, meta)"""
    t0 = rng.integers(0, T - Kw + 1, B)
    m = rng.integers(0, M, B)
    i = rng.integers(0, H - h + 1, B)
    j = rng.integers(0, W - w + 1, B)
    anchor = t0 + Kw // 2
    items = np.stack([t0, m, anchor, np.zeros_like(t0), i, j], axis=1).astype(np.int64)
    times = (t0[:, None] + np.arange(Kw)[None]).astype(np.int64)
    meta = np.stack([m, anchor, i, j], axis=1).astype(np.int64)
    return items, times, meta


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    dev = torch.device("cuda")
    g = torch.Generator(device=dev).manual_seed(0)
    fields = {V: (torch.randn(T, M, V, H, W, device=dev, generator=g), torch.randn(T, M, V, H, W, device=dev, generator=g))
              for V in VS}
    c1, t1 = (f[:, :, 0].contiguous() for f in fields[1])  # the same data as (T, M, H, W) for the old kernel
    rng = np.random.default_rng(0)
    ok = True
    for name, B, Kw, h, w in SHAPES:
        items, times, meta = (torch.from_numpy(x).to(dev) for x in items_for(rng, B, Kw, h, w))
        out = {V: (torch.empty(B, V, Kw, h, w, device=dev), torch.empty(B, V, h, w, device=dev)) for V in VS}
        old_out = (torch.empty(B, 1, Kw, h, w, device=dev), torch.empty(B, 1, h, w, device=dev))

        def old():
            call("cesm_window_gather", K.P(c1), K.P(t1), K.P(items), K.P(old_out[0]), K.P(old_out[1]), B, Kw, M, H, W,
                 h, w, 1, K.S())

        def new(V):
            cf, tf = fields[V]
            cs = list(range(V)) + [0] * (4 - V)
            return lambda: K._mv_call("cesm_window_gather_mv", name, K.P(cf), K.P(tf), K.P(times), K.P(meta),
                                      K.P(out[V][0]), K.P(out[V][1]), B, Kw, V, V, *cs, T, M, H, W, h, w, K.S())

        cases = {"old(1)": old, **{f"new({V})": new(V) for V in VS}}
        for fn in cases.values():
            fn()
        torch.cuda.synchronize()
        same = torch.equal(old_out[0], out[1][0]) and torch.equal(old_out[1], out[1][1])
        print(f"{name}: V = 1 outputs of the two kernels equal: {same}", flush=True)
        ok &= same
        t = {k: [] for k in cases}
        for rnd in range(a.rounds):
            for k, fn in cases.items():
                us = timed(fn, a.reps)
                t[k].append(us)
                print(f"round {rnd} {name} {k}: {us:.2f} us", flush=True)
        med = {k: statistics.median(v) for k, v in t.items()}
        print(f"{name}: old(1) median {med['old(1)']:.2f} us (spread {min(t['old(1)']):.2f} .. {max(t['old(1)']):.2f})",
              flush=True)
        for V in VS:
            nbytes = 2 * B * (V * Kw + V) * h * w * 4
            floor = nbytes / HBM * 1e6
            tn, lim = med[f"new({V})"], 1.1 * V * med["old(1)"]
            passed = tn <= lim
            ok &= passed
            print(f"{name}: new({V}) median {tn:.2f} us (spread {min(t[f'new({V})']):.2f} .. {max(t[f'new({V})']):.2f}); "
                  f"yardstick V x old(1) = {V * med['old(1)']:.2f} us, gate 1.1 x = {lim:.2f} us: "
                  f"{'PASS' if passed else 'FAIL'}; {nbytes / 1e6:.1f} MB read + written, floor {floor:.2f} us "
                  f"({tn / floor:.1f} x floor, {nbytes / tn / 1e6:.2f} TB/s)", flush=True)
    print("GATE", "PASS" if ok else "FAIL", flush=True)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
