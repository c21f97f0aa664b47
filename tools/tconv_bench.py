"""Per-call time of the temporal-conv block (csrc/tconv.h) beside the attention block it replaces and the LayerNorm
floor, in one process:  python tools/tconv_bench.py [--shape B F H W C] [--reps N] [--rounds R]
Whole training step of a config with use_temp_attn False against True:  python tools/tconv_bench.py --step [--shape ..]

Timed through the executors of video_net.py (tconv_fwd / tconv_bwd, tattn_fwd / tattn_bwd: every launch of a block's
forward and of its backward with all parameter gradients), bf16, HIP events around `reps` back-to-back calls; the
variants alternate over `rounds` rounds and the median round is reported.  cesm_ln_fwd on the same tensor moves the
temporal-conv forward's bytes (one read, one write) and is its floor.  Bytes and FLOPs are counted from the shape.
"""
import argparse
import json
import statistics
import sys

import torch

sys.path.insert(0, ".")
from cesm_emulator_amd import kernels as K  # noqa: E402
from cesm_emulator_amd import video_net as VN  # noqa: E402


def timed(fn, reps):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps * 1e3  # us


def step_bench(a):
    """bf16 training steps (bench.py's loop: FusedAdamW + clip, resident batch) of config/<a.config> with
    use_temp_attn False and True, alternating rounds in one process; median round per variant"""
    import time
    from cesm_emulator_amd.model import Diffusion
    from cesm_emulator_amd.optim import FusedAdamW
    from cesm_emulator_amd.train import build_model_from_config, train_step, rank_generator
    B, F, H, W, _ = a.shape
    dev = torch.device("cuda")
    with open(f"config/{a.config}") as fh:
        cfg = json.load(fh)["unet"]
    g = torch.Generator(device=dev).manual_seed(1000)
    x0 = torch.randn(B, 1, H, W, device=dev, generator=g)
    cond = torch.randn(B, 1, F, H, W, device=dev, generator=g)
    runs = {}
    for flag in (False, True):
        torch.manual_seed(1)
        unet = build_model_from_config(dict(cfg, use_temp_attn=flag)).to(dev)
        unet.compute_dtype = torch.bfloat16
        diff = Diffusion(unet).to(dev)
        diff.generator = rank_generator(dev, 2, 0)
        opt = FusedAdamW(diff.parameters(), lr=2e-4, betas=(0.9, 0.999), weight_decay=1e-4, max_grad_norm=1.0)
        runs[flag] = (diff, opt)
        for _ in range(3):
            loss = train_step(diff, opt, x0, cond, 1.0, None)
        torch.cuda.synchronize()
        assert torch.isfinite(loss).item()
    ms = {False: [], True: []}
    for _ in range(a.rounds):
        for flag, (diff, opt) in runs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.reps):
                train_step(diff, opt, x0, cond, 1.0, None)
            torch.cuda.synchronize()
            ms[flag].append((time.perf_counter() - t0) / a.reps * 1e3)
    med = {k: statistics.median(v) for k, v in ms.items()}
    print(json.dumps({"config": a.config, "shape": {"B": B, "F": F, "H": H, "W": W}, "steps_per_round": a.reps,
                      "rounds": a.rounds,
                      "use_temp_attn_false": {"ms_per_step": round(med[False], 2), "samples_per_s": round(B / med[False] * 1e3, 3),
                                              "min_max_ms": [round(min(ms[False]), 2), round(max(ms[False]), 2)]},
                      "use_temp_attn_true": {"ms_per_step": round(med[True], 2), "samples_per_s": round(B / med[True] * 1e3, 3),
                                             "min_max_ms": [round(min(ms[True]), 2), round(max(ms[True]), 2)]}}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", action="store_true", help="time whole training steps of --config, both variants")
    ap.add_argument("--config", default="more_blocks")
    ap.add_argument("--shape", type=int, nargs=5, default=[8, 12, 192, 288, 64], metavar=("B", "F", "H", "W", "C"))
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--no-attn", action="store_true", help="skip the attention block (kernels only)")
    a = ap.parse_args()
    B, F, H, W, C = a.shape
    if not torch.cuda.is_available():
        raise SystemExit("tconv_bench needs the GPU (no CPU timing)")
    if a.step:
        return step_bench(a)
    dev = torch.device("cuda")
    torch.manual_seed(0)
    x = torch.randn(B * F, H, W, C, device=dev).to(torch.bfloat16)
    dy = torch.randn_like(x)
    nets = {}
    for name, flag in (("tconv", False), ("attn", True)):
        torch.manual_seed(1)
        net = VN.UNetModel3D(1, C, dim_mults=(1, 2, 4), use_temp_attn=flag).to(dev)
        net.compute_dtype = torch.bfloat16
        if not flag:
            with torch.no_grad():
                conv = net.input_temp_op.fn.fn.temporal_conv
                conv.weight.copy_(torch.randn_like(conv.weight) * 0.05)
                conv.bias.copy_(torch.randn_like(conv.bias) * 0.1)
        nets[name] = net

    def ctx(net):
        rc = VN.RunCtx(net, B, F, torch.bfloat16, True)
        rpb = net.time_rel_pos_bias
        rc.bias = K.relpos_fwd(rpb.relative_attention_bias.weight, F, rpb.num_buckets, rpb.max_distance)
        rc.rot = K.rope_table(net.mid_temporal_attn.fn.fn.fn.rotary_emb.freqs, F)
        rc.dtable = VN.gbuf(rpb.relative_attention_bias.weight)
        return rc

    st = {}
    variants = {}
    rc_c = ctx(nets["tconv"])
    blk_c = nets["tconv"].input_temp_op

    def c_fwd():
        st["c"] = VN.tconv_fwd(rc_c, blk_c, x)[1]

    def c_bwd():
        VN.tconv_bwd(rc_c, blk_c, st["c"], dy)

    gamma = VN._flat(blk_c.fn.norm.gamma)
    variants["ln_fwd"] = lambda: K.ln_fwd(x, gamma, save=True)
    variants["tconv_fwd"] = c_fwd
    variants["tconv_bwd"] = c_bwd
    if not a.no_attn:
        rc_a = ctx(nets["attn"])
        blk_a = nets["attn"].input_temp_op

        def a_fwd():
            st["a"] = VN.tattn_fwd(rc_a, blk_a, x)[1]

        def a_bwd():
            VN.tattn_bwd(rc_a, blk_a, st["a"], dy)
            rc_a.join()

        variants["tattn_fwd"] = a_fwd
        variants["tattn_bwd"] = a_bwd
    for fn in variants.values():  # warm-up: code objects, allocator, weight packs
        fn()
        fn()
    times = {k: [] for k in variants}
    for _ in range(a.rounds):
        for k, fn in variants.items():
            times[k].append(timed(fn, a.reps))
    med = {k: statistics.median(v) for k, v in times.items()}
    V = B * F * H * W
    res = {"shape": {"B": B, "F": F, "H": H, "W": W, "C": C}, "reps": a.reps, "rounds": a.rounds,
           "median_us": {k: round(v, 1) for k, v in med.items()},
           "min_max_us": {k: [round(min(v), 1), round(max(v), 1)] for k, v in times.items()},
           "fwd_bytes": 2 * V * C * 2, "fwd_flop": 2 * 3 * C * C * V,
           "fwd_GBps": round(2 * V * C * 2 / med["tconv_fwd"] / 1e3, 1),
           "fwd_over_ln_floor": round(med["tconv_fwd"] / med["ln_fwd"], 3),
           # the backward reads x and dy twice (dx pass, dW pass) and writes dx
           "bwd_bytes": 5 * V * C * 2, "bwd_GBps": round(5 * V * C * 2 / med["tconv_bwd"] / 1e3, 1)}
    if not a.no_attn:
        res["tconv_fwd_bwd_us"] = round(med["tconv_fwd"] + med["tconv_bwd"], 1)
        res["tattn_fwd_bwd_us"] = round(med["tattn_fwd"] + med["tattn_bwd"], 1)
        res["tconv_faster_than_attention"] = res["tconv_fwd_bwd_us"] < res["tattn_fwd_bwd_us"]
    print(json.dumps(res))
    if not a.no_attn and not res["tconv_faster_than_attention"]:
        raise SystemExit("the temporal-conv block is not faster than the attention block it replaces")


if __name__ == "__main__":
    main()
