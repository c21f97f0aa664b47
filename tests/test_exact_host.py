"""CPU half of the exact integer-data tests (tests/exact_data.py): the input regime and the kernel coverage of the
sweeps that tests/test_gpu_exact.py runs, frozen without a GPU.  A planner change that silently stops a kernel from being
exercised, or an input change that leaves the exact regime, fails here."""
import pytest
import torch
import torch.nn.functional as F

import exact_data as X
from exact_data import BF


# ------------------------------------------------------------------ generator rule
def test_ints_distribution():
    g = torch.Generator().manual_seed(1)
    for amax, e2 in ((2, 2.0), (1, 2.0 / 3.0), (1, 1024.0 / (2 * 4608)), (3, 4.0), (3, 1.0)):
        v = X.ints((200000,), amax, e2, g)
        assert v.dtype == torch.float64 and torch.equal(v, v.round()) and float(v.abs().max()) <= amax
        assert abs(float((v * v).mean()) - e2) < 0.03 * max(e2, 0.1), (amax, e2, float((v * v).mean()))


# K = 64 .. 4608: 1x1 at 64 / 256 / 768, 4x4 at 128, 3x3 at 64 / 512 channels
@pytest.mark.parametrize("k,cin", [(1, 64), (1, 256), (1, 768), (4, 128), (3, 64), (3, 512)])
def test_operand_rule_keeps_the_regime(k, cin):
    """x in {-2..2}, ternary weights thinned to min(2/3, 1024 / (2K)), bias and residual in {-3..3}: check_regime
    passes on the reference alone (bf16-stored y and y + res at or below 256, sum |x||w| far below 2^22), with most
    outputs non-zero"""
    Kc = k * k * cin
    g = X.gen_for("rule", k, cin)
    x = X.ints((2, cin, 24, 40), X.X_AMAX, X.X_E2, g)
    w = X.ints((64, cin, k, k), 1, X.weight_e2(Kc), g)
    b = X.ints((64,), 3, 4.0, g)
    y = F.conv2d(x, w, b, padding=k // 2)
    res = X.ints(tuple(y.shape), 3, 4.0, g)
    sabs = F.conv2d(x.abs(), w.abs(), b.abs(), padding=k // 2)
    X.check_regime([y], [y, y + res], [sabs])
    assert Kc * X.X_E2 * X.weight_e2(Kc) <= 1024 + 1e-9
    assert float((y != 0).double().mean()) > 0.95
    assert float(sabs.max()) < 2048


def test_check_regime_and_assert_exact_have_teeth():
    ok = torch.tensor([1.0, -256.0])
    X.check_regime([ok], [ok], [ok.abs(), 100])
    for bad in (dict(ref=[torch.tensor([0.5])], stored_bf16=[]), dict(ref=[ok], stored_bf16=[torch.tensor([257.0])]),
                dict(ref=[ok], stored_bf16=[], abs_ref=[torch.tensor([float(1 << 22)])]),
                dict(ref=[ok], stored_bf16=[], abs_ref=[1 << 22]), dict(ref=[torch.tensor([float(1 << 24)])], stored_bf16=[])):
        with pytest.raises(AssertionError):
            X.check_regime(**bad)
    a = torch.zeros(2, 40, 80, 4)
    b = a.clone()
    X.assert_exact(a, b, "same")
    b[1, 3, 35, 2] = 1
    b[1, 5, 71, 0] = float("nan")
    with pytest.raises(AssertionError) as e:
        X.assert_exact(b, a, "y")
    msg = str(e.value)
    assert "2 of" in msg and "[(1, 1), (3, 5), (35, 71), (0, 2)]" in msg and "'axis2%36': [35]" in msg
    assert "'axis2%32': [3, 7]" in msg and "(1, 3, 35, 2), 1.0, 0.0" in msg
    nanx = X.poison(torch.zeros(3))
    with pytest.raises(AssertionError):
        X.assert_exact(nanx, nanx, "poison never passes")


@pytest.mark.parametrize("case", [("3x3", BF, 3, 9, 33, 64, 0, 64, True), ("3x3", BF, 3, 9, 36, 64, 128, 64, True),
                                  ("down", BF, 2, 4, 66, 64, 0, 64, True), ("up", BF, 2, 2, 33, 128, 0, 128, True),
                                  ("1x1", BF, 1, 1, 257, 64, 0, 768, False), ("3x3", X.F32, 2, 5, 7, 64, 64, 128, True)])
def test_conv_case_reference(case):
    """a ConvCase builds (its constructor asserts the regime) and its gradients are those of a plain per-element
    restatement at a few sampled positions"""
    c = X.ConvCase(*case)
    kind, _, Nb, H, W, c1, c2, cout, _ = case
    k, s, p, tr = X.KINDS[kind]
    Ho, Wo = X.out_hw(kind, H, W)
    assert c.y.shape == (Nb, Ho, Wo, cout) and c.dx.shape == c.x.shape and c.dw.shape == c.w.shape
    g = X.gen_for("probe", *case[2:8])
    for _ in range(6):  # dW[a][b][ky][kx] = sum over pixels of the two tensors it couples
        ky, kx = (int(torch.randint(0, k, (1,), generator=g)) for _ in range(2))
        co, ci = int(torch.randint(0, cout, (1,), generator=g)), int(torch.randint(0, c1 + c2, (1,), generator=g))
        tot = 0.0
        for oy in range(Ho):
            for ox in range(Wo):
                if tr:  # y[iy*s - p + ky] += x[iy] w[ci][co][ky]
                    iy, r1 = divmod(oy + p - ky, s)
                    ix, r2 = divmod(ox + p - kx, s)
                    if r1 or r2:
                        continue
                else:
                    iy, ix = oy * s - p + ky, ox * s - p + kx
                if 0 <= iy < H and 0 <= ix < W:
                    tot += float((c.x[:, iy, ix, ci] * c.dy[:, oy, ox, co]).sum())
        got = c.dw[ci, co, 0, ky, kx] if tr else c.dw[co, ci, 0, ky, kx]
        assert float(got) == tot


# ------------------------------------------------------------------ dispatch coverage
def _collect(sweep):
    fwd, wg, ns3 = set(), set(), []
    for (kind, dt, Nb, H, W, c1, c2, co, bias) in sweep:
        f, w, ns = X.conv_kernel_names(kind, dt, Nb, H, W, c1, c2, co, bias)
        fwd |= f
        wg |= w
        if kind == "3x3" and dt == BF:
            ns3 += ns
    return fwd, wg, ns3


def test_sweeps_reach_every_conv_kernel():
    """the union of the kernels the GPU sweeps reach is the complete name table of cesm_conv_fwd_variant and
    cesm_conv_wgrad_variant -- all 17 forward names, the three halo / stride-2 weight-gradient kernels, the six
    square-tile and six wide instantiations and the fp32 generic one -- and the 3x3 sweeps split the pixels"""
    from cesm_emulator_amd import kernels as K
    from cesm_emulator_amd.build import build
    build()
    fwd, wg, ns3 = set(), set(), []
    per = {}
    for name, sweep in X.SWEEPS.items():
        per[name] = _collect(sweep)
        fwd |= per[name][0]
        wg |= per[name][1]
        ns3 += per[name][2]
    assert "invalid" not in fwd
    assert {n: len(s) for n, s in X.SWEEPS.items()} == {"3x3_full": 2 * 11 * 12, "3x3_reduced": 3 * 3 * 4 + 1,
                                                        "s2": 2 * 2 * 5 * 8, "s2_generic": 4, "1x1": 8 * 9 * 2, "fp32": 16}
    assert all(len(set(s)) == len(s) for s in X.SWEEPS.values())
    assert len(X.FWD_NAMES) == 17 and fwd == X.FWD_NAMES, fwd ^ X.FWD_NAMES
    assert len(X.WGRAD_NAMES) == 16 and wg == X.WGRAD_NAMES, wg ^ X.WGRAD_NAMES
    assert max(ns3) > 1 and sum(n > 1 for n in ns3) >= 100
    # what each sweep is there for (DESIGN.md "Exact-data tests" lists the same)
    assert {"conv3x3ws_kernel<32>", "conv3x3ws_kernel<36>", "conv3x3p_kernel<32,7,true>", "conv3x3_bf16_kernel<36>",
            "conv3x3_bf16_kernel<32>"} == per["3x3_full"][0]
    assert per["3x3_full"][1] == per["3x3_reduced"][1] == {"wgrad3x3c64_kernel", "wgrad3x3w36c64_kernel"}
    assert per["3x3_reduced"][0] == {"conv3x3_bf16_kernel<36>"}  # the 32-wide halo: narrow widths of the full sweep
    assert per["s2"][0] == {f"convs2_bf16_kernel<{tw},{d}>" for tw in (32, 36) for d in ("down", "up")}
    # (below Wl = 64 the wide kernel: with the bias gradient riding for the down conv, without for the transposed one)
    assert per["s2"][1] == {"wgrads2_bf16_kernel"} | {f"wgrad_wide_kernel<{c},{b}>" for c in (64, 128)
                                                      for b in ("false", "true")}
    assert per["s2_generic"][0] == {"conv_fwd_bf16_kernel<64>", "conv_fwd_bf16_kernel<128>",
                                    "conv_fwd_bf16_kernel<64,true>", "conv_fwd_bf16_kernel<128,true>"}
    assert per["1x1"][0] == {"gemm1x1_kernel<128>", "gemm1x1_kernel<64>"}
    assert per["1x1"][1] == X.WGRAD_NAMES - {"wgrad3x3c64_kernel", "wgrad3x3w36c64_kernel", "wgrads2_bf16_kernel",
                                             "conv_wgrad_kernel<float>"}
    assert per["fp32"][0] == {"conv_fwd_kernel<float,128>", "conv_fwd_kernel<float,64>"}
    assert per["fp32"][1] == {"conv_wgrad_kernel<float>"}
    # the one name no sweep can hold: the generic kernel in bf16 serves only M >= 2^31 output pixels
    big = (BF, 1 << 15, 1 << 8, 1 << 8, 64, 0, 1 << 8, 1 << 8, 64, 64, 1, 1, 1, 0, 1)
    assert K.conv_wgrad_variant(*big) == X.WGRAD_NAME_BIG_M
    assert K.conv_wgrad_variant(BF, (1 << 15) - 1, *big[2:]) == "wgrad_wide_kernel<64,false>"


def test_named_tiny_shapes():
    """the smallest shapes that reach the level-0 kernels and the stride-2 pair, as (H, W) of the layer's input"""
    from cesm_emulator_amd import kernels as K

    def fv(kind, H, W, c1=64, c2=0, co=64):
        return K.conv_fwd_variant(*X.conv_launches(kind, BF, 1, H, W, c1, c2, co)[0][1])

    assert fv("3x3", 7, 33) == "conv3x3ws_kernel<36>"
    assert fv("3x3", 8, 29) == "conv3x3ws_kernel<32>"
    assert fv("3x3", 1, 32) == "conv3x3p_kernel<32,7,true>"
    assert fv("3x3", 13, 4) == "conv3x3_bf16_kernel<32>"
    assert fv("down", 4, 66) == "convs2_bf16_kernel<36,down>"
    assert fv("up", 2, 33) == "convs2_bf16_kernel<36,up>"
    assert fv("down", 9, 11) == "conv_fwd_bf16_kernel<64>"


def test_reduced_sweeps_lose_coverage():
    """the coverage assertions are tight: the 64 -> 64 sweep without its 32-multiple widths loses conv3x3p, without the
    widths 36 / 72 the 36-wide weight-gradient kernel; the stride-2 sweep below Wl = 64 loses wgrads2; the 1x1 sweep
    without its bias-free half loses the six <..., false> / unsuffixed weight-gradient kernels"""
    no32 = [c for c in X.SWEEP_3X3_FULL if c[4] % 32]
    assert "conv3x3p_kernel<32,7,true>" not in _collect(no32)[0]
    no36 = [c for c in X.SWEEP_3X3_FULL + X.SWEEP_3X3_REDUCED if c[4] % 36]
    assert "wgrad3x3w36c64_kernel" not in _collect(no36)[1]
    narrow = [c for c in X.SWEEP_S2 if (c[4] if c[0] == "up" else c[4] // 2) < 64]
    assert "wgrads2_bf16_kernel" not in _collect(narrow)[1]
    with_bias = [c for c in X.SWEEP_1X1 if c[8]]
    assert len(_collect(with_bias)[1]) == 6
    one_px_tile = [c for c in X.SWEEP_3X3_FULL if c[2] * c[3] * c[4] < 512]
    assert max(_collect(one_px_tile)[2]) == 1


# ------------------------------------------------------------------ the data is the same in every process
SENS_CASE = ("3x3", BF, 3, 9, 33, 64, 0, 64, True)   # the sensitivity case of tests/test_gpu_exact.py


def test_case_data_is_pinned():
    """the seed of a case comes from its parameters alone (a CRC of their repr: no per-process hash salt), so the CPU
    run here and the GPU run see the same integers, and a mismatch reported on one machine is regenerated on any other;
    one case's seed and checksums are pinned"""
    assert X.seed_for("3x3", "torch.bfloat16", 3, 9, 33, 64, 0, 64, True) == 926223425
    c = X.ConvCase(*SENS_CASE)
    assert (float(c.x.sum()), float((c.x * c.x).sum()), int((c.w != 0).sum())) == (-117.0, 114109.0, 24663)
    assert (float(c.y.sum()), float(c.y.abs().max())) == (-3391.0, 127.0)
    again = X.ConvCase(*SENS_CASE)
    assert torch.equal(c.x, again.x) and torch.equal(c.w, again.w) and torch.equal(c.dy, again.dy)


def test_sensitivity_figures():
    """what the GPU sensitivity case must see, from the reference alone: one +1 on channel 5 of image 1 at either image
    corner changes 176 / 164 of the 57,024 outputs, a relative L2 of 2.1e-3 / 2.0e-3 -- under the 1e-2 gate of the
    tolerance-based tests (DESIGN.md quotes these)"""
    c = X.ConvCase(*SENS_CASE)
    for (iy, ix), count, rel in (((0, 0), 176, 2.104e-3), ((8, 32), 164, 2.031e-3)):
        d = torch.zeros_like(c.y)
        for oy in range(max(0, iy - 1), min(9, iy + 2)):
            for ox in range(max(0, ix - 1), min(33, ix + 2)):
                d[1, oy, ox] = c.w[:, 5, 0, iy - oy + 1, ix - ox + 1]
        assert int((d != 0).sum()) == count and d.numel() == 57024
        assert abs((d.norm() / c.y.norm()).item() - rel) < 1e-6


def test_sweep_extremes():
    """every case of every sweep builds (its constructor asserts the regime), and the largest bf16-stored magnitudes
    over all of them are the ones DESIGN.md quotes: |y|, |y + res| <= 170 and |dx|, |dx + dres| <= 186, against 256"""
    my = mdx = 0.0
    for sweep in X.SWEEPS.values():
        for case in sweep:
            c = X.ConvCase(*case)
            my = max(my, float(c.y.abs().max()), float((c.y + c.res).abs().max()))
            mdx = max(mdx, float(c.dx.abs().max()), float((c.dx + c.dres).abs().max()))
    assert (my, mdx) == (170.0, 186.0)


@pytest.mark.parametrize("amax,M", X.HEADROOM_CASES)
def test_headroom_cases_sit_in_the_band(amax, M):
    """the headroom cases lie where they claim (asserted inside headroom_case): 2^22 <= max sum |a||b| < 2^24, with
    |dW| itself far below 2^24"""
    x, dy, dw, sabs = X.headroom_case(amax, M)
    assert float(dw.abs().max()) < (1 << 22) and float(x.abs().max()) == amax == float(dy.abs().max())
