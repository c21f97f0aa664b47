"""HIP-event timing of the ensemble statistics at the sizes a validation run uses, [16, 40, 1, 192, 288] and
[16, 100, 1, 192, 288] fp32 (141 and 354 MB): kernels.ens_stats with every output (four maps and the accumulator)
against the torch composition of the same quantities on the same tensors -- mean, var(unbiased), CRPS from a sort
(sum_k (2k - M + 1) x_(k)), rank by comparison, the weighted sums and the rank histogram -- in one process, warm, the
two alternated over several rounds, median per variant.  The floor printed beside them is reading ens once at the
6.3 TB/s the MI355X achieves from HBM.  The two are also compared (relative L2 of crps, equality of rank).
usage: [CESM_HIP_LIB=...] python tools/ens_time.py [--rounds N] [--reps N]"""
import argparse
import statistics
import sys

import torch

sys.path.insert(0, ".")
from cesm_emulator_amd import kernels as K  # noqa: E402

B, V, H, W = 16, 1, 192, 288
HBM = 6.3e12


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps * 1e3


def torch_stats(ens, obs, w, row0):
    """the same outputs composed from torch ops (fp32 maps, float64 accumulator)"""
    Bn, M, Vn, Hn, Wn = ens.shape
    mean = ens.mean(dim=1)
    var = ens.var(dim=1, unbiased=True)
    y = obs.unsqueeze(1)
    A = (ens - y).abs().sum(dim=1)
    xs = ens.sort(dim=1).values
    k = torch.arange(M, device=ens.device, dtype=torch.float32).view(1, M, 1, 1, 1)
    P = ((2 * k - (M - 1)) * xs).sum(dim=1)
    crps = A / M - P / (M * (M - 1))
    rank = (ens < y).sum(dim=1, dtype=torch.int32)
    rows = (row0.view(Bn, 1) + torch.arange(Hn, device=ens.device).view(1, Hn)).clamp_(0, w.numel() - 1)
    wr = w[rows].view(Bn, 1, Hn, 1).double()
    acc = torch.empty(Vn, 4 + M + 1, dtype=torch.float64, device=ens.device)
    acc[:, 0] = wr.expand(Bn, Vn, Hn, Wn).sum(dim=(0, 2, 3))
    acc[:, 1] = (wr * (mean - obs) ** 2).sum(dim=(0, 2, 3))
    acc[:, 2] = (wr * var).sum(dim=(0, 2, 3))
    acc[:, 3] = (wr * crps).sum(dim=(0, 2, 3))
    onehot_w = wr.expand(Bn, Vn, Hn, Wn).permute(1, 0, 2, 3).reshape(Vn, -1)
    idx = rank.permute(1, 0, 2, 3).reshape(Vn, -1).long()
    acc[:, 4:] = torch.zeros(Vn, M + 1, dtype=torch.float64, device=ens.device).scatter_add_(1, idx, onehot_w)
    return mean, var, crps, rank, acc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()
    dev = torch.device("cuda")
    g = torch.Generator(device=dev).manual_seed(0)
    w = (2 * torch.rand(H, device=dev, generator=g)).contiguous()
    row0 = torch.zeros(B, dtype=torch.int64, device=dev)
    for M in (40, 100):
        ens = torch.randn(B, M, V, H, W, device=dev, generator=g)
        obs = torch.randn(B, V, H, W, device=dev, generator=g)
        cases = {"hip": lambda: K.ens_stats(ens, obs, w, row0), "torch": lambda: torch_stats(ens, obs, w, row0)}
        r = K.ens_stats(ens, obs, w, row0)
        t = torch_stats(ens, obs, w, row0)
        rel = float((r["crps"].double() - t[2].double()).norm() / t[2].double().norm())
        same_rank = bool(torch.equal(r["rank"], t[3]))
        acc_rel = float(((r["acc"] - t[4]).abs() / t[4].abs().clamp_min(1e-300)).max())
        print(f"M={M}: hip vs torch crps rel L2 {rel:.2e}, rank equal {same_rank}, acc worst rel {acc_rel:.2e}",
              flush=True)
        times = {k: [] for k in cases}
        for rnd in range(a.rounds):
            for name, fn in cases.items():
                us = timed(fn, a.reps)
                times[name].append(us)
                print(f"round {rnd} M={M} {name}: {us:.1f} us", flush=True)
        floor = ens.numel() * 4 / HBM * 1e6
        med = {k: statistics.median(v) for k, v in times.items()}
        print(f"M={M}: ens {ens.numel() * 4 / 1e6:.0f} MB, read-once floor {floor:.1f} us; hip median {med['hip']:.1f} us "
              f"({med['hip'] / floor:.2f} x floor, {ens.numel() * 4 / med['hip'] / 1e6:.2f} TB/s of ens), torch median "
              f"{med['torch']:.1f} us ({med['torch'] / med['hip']:.1f} x the kernel)", flush=True)
        del ens, obs, r, t


if __name__ == "__main__":
    main()
