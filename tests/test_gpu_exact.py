"""Exact integer-data tests of every conv, GEMM and reduction kernel (tests/exact_data.py holds the regime).

The kernels are linear: on small integer operands every product and every partial sum is exact in fp32 and every
bf16-stored result is representable, so each comparison below is bitwise equality with a float64 reference -- no
tolerance.  The preconditions are asserted on the reference alone (check_regime).  Every output and workspace the
wrappers allocate is NaN-filled before the launch (the `poisoned` fixture replaces kernels.empty), caller-owned slabs
are poisoned by hand, and destinations that accumulate hold small integers first.

The convs run through the product's own path (VN.conv_forward / VN.conv_backward on a module whose weight and bias hold
the integers): forward, data gradient, weight gradient and bias gradient of each shape in one go.  Which kernel each
sweep reaches is asserted on the CPU by tests/test_exact_host.py.
"""
import os
import sys

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import exact_data as X  # noqa: E402
from exact_data import BF, F32  # noqa: E402
from cesm_emulator_amd import kernels as K  # noqa: E402
from cesm_emulator_amd import video_net as VN  # noqa: E402
from cesm_emulator_amd._lib import call  # noqa: E402

pytestmark = pytest.mark.gpu
DTYPES = [F32, BF]


@pytest.fixture(autouse=True)
def poisoned(monkeypatch):
    """every tensor a kernels.* wrapper allocates (outputs, slabs, partials) starts as NaN"""
    def empty(shape, dtype, device):
        t = torch.empty(shape, dtype=dtype, device=device)
        return X.poison(t) if t.is_floating_point() else t
    monkeypatch.setattr(K, "empty", empty)


def nan(shape, dev, dtype=F32):
    return X.poison(torch.empty(shape, dtype=dtype, device=dev))


class _PackHost:
    def _packed(self, w, cdt, cout, cin, kh, kw, swap, flip):
        return K.conv_pack(w.detach().contiguous(), cdt, cout, cin, kh, kw, swap, flip)


# ------------------------------------------------------------------ a / c / d / e: convs through the product path
def run_conv_case(dev, case, res_modes=(False, True)):
    kind, dt, Nb, H, W, c1, c2, cout, bias = case
    c = X.ConvCase(*case)  # reference + regime
    k, s, p, tr = X.KINDS[kind]
    md = (nn.ConvTranspose3d if tr else nn.Conv3d)(c1 + c2, cout, (1, k, k), (1, s, s), (0, p, p), bias=bias).to(dev)
    with torch.no_grad():
        md.weight.copy_(c.w)
        if bias:
            md.bias.copy_(c.bias)
    rc = VN.RunCtx(_PackHost(), 1, Nb, dt, True)
    spec = VN.ConvSpec(md)
    x = c.x.to(dev, dt)
    x1 = x[..., :c1].contiguous()
    x2 = x[..., c1:].contiguous() if c2 else None
    dy = c.dy.to(dev, dt)
    for with_res in res_modes:
        tag = f"{kind} {dt} Nb={Nb} {H}x{W} {c1}+{c2}->{cout} bias={bias} res={with_res}"
        y, st = VN.conv_forward(rc, spec, x1, x2, c.res.to(dev, dt) if with_res else None)
        md.weight.grad = c.dw0.to(dev, F32)
        if bias:
            md.bias.grad = c.db0.to(dev, F32)
        dres = c.dres.to(dev, dt) if with_res else None
        d1 = dres[..., :c1].contiguous() if with_res else None
        d2 = dres[..., c1:].contiguous() if with_res and c2 else None
        dx = VN.conv_backward(rc, spec, st, dy, True, d1, d2)
        torch.cuda.synchronize()
        X.assert_exact(y, c.y + c.res if with_res else c.y, tag + ": y")
        want = c.dx + c.dres if with_res else c.dx
        if c2:
            X.assert_exact(dx[0], want[..., :c1], tag + ": dx (first source)")
            X.assert_exact(dx[1], want[..., c1:], tag + ": dx (second source)")
        else:
            X.assert_exact(dx, want, tag + ": dx")
        X.assert_exact(md.weight.grad, c.dw0 + c.dw, tag + ": dW (+= onto integers)", spatial=(3, 4))
        if bias:
            X.assert_exact(md.bias.grad, c.db0 + c.db, tag + ": db (+= onto integers)")


@pytest.mark.parametrize("cout", [64, 128])
@pytest.mark.parametrize("W", X.FULL_W)
def test_conv3x3_full_sweep(dev, W, cout):
    """a: 64 -> 64 reaches conv3x3ws<32>, <36>, conv3x3p and both halo widths; 64 -> 128 the halo kernels in their 256-
    and 448-pixel tiles; every height of the sweep at this width, with and without the fused residuals"""
    cases = [c for c in X.SWEEP_3X3_FULL if c[4] == W and c[7] == cout]
    assert len(cases) == len(X.FULL_H)
    for case in cases:
        run_conv_case(dev, case)


@pytest.mark.parametrize("chan", [(64, 128, 64), (128, 0, 64), (256, 0, 512), (512, 0, 512)], ids=str)
def test_conv3x3_reduced_sweep(dev, chan):
    """a: concat input (the data gradient is split), Cin != Cout, the deep levels"""
    cases = [c for c in X.SWEEP_3X3_REDUCED if c[5:8] == chan]
    assert len(cases) == (1 if chan[0] == 512 else 12)
    for case in cases:
        run_conv_case(dev, case)


@pytest.mark.parametrize("C", [64, 128])
@pytest.mark.parametrize("kind", ["down", "up"])
def test_stride2_sweep(dev, kind, C):
    """c: 4x4 stride-2 down and its transpose up on the low-resolution grid sweep; dW from wgrads2 where Wl >= 64, the
    wide kernel elsewhere"""
    cases = [c for c in X.SWEEP_S2 if c[0] == kind and c[5] == C]
    assert len(cases) == 40
    for case in cases:
        run_conv_case(dev, case)


@pytest.mark.parametrize("case", X.SWEEP_S2_GENERIC, ids=str)
def test_stride2_generic_bf16(dev, case):
    """c: odd sizes and concat / split: conv_fwd_bf16_kernel<64>, <128> and their parity forms <64,true>, <128,true>"""
    run_conv_case(dev, case)


@pytest.mark.parametrize("chan", X.CH_1X1, ids=str)
def test_conv1x1_sweep(dev, chan):
    """d: gemm1x1 (one- and two-stage, split destination in the concat's data gradient) and the wide / square-tile
    weight gradients, with the bias gradient riding and (bias-free module) without"""
    cases = [c for c in X.SWEEP_1X1 if c[5:8] == chan]
    assert len(cases) == 2 * len(X.M_1X1)
    for case in cases:
        run_conv_case(dev, case)


@pytest.mark.parametrize("case", X.SWEEP_FP32, ids=str)
def test_fp32_generic(dev, case):
    """e: the fp32 generic forward / weight-gradient kernels: 3x3, 4x4 stride 2, transposed 4x4, concat with split"""
    run_conv_case(dev, case)


def _rows(M, cin, cout, key):
    g = X.gen_for("rows", M, cin, cout, key)
    x = X.ints((M, cin), X.X_AMAX, X.X_E2, g)
    dy = X.ints((M, cout), X.X_AMAX, X.X_E2, g)
    dw0, db0 = X.prefill((cout, cin), g), X.prefill((cout,), g)
    dw, db = torch.einsum("mo,mi->oi", dy, x), dy.sum(0)
    X.check_regime([dw, db, dw + dw0, db + db0], [], [M * X.X_AMAX * X.X_AMAX])
    return x, dy, dw0, db0, dw, db


def test_conv1x1_wgrad_split_destination(dev):
    """d: the weight gradient of a conv whose output went to two tensors (Co1 != Cout: dy1 | dy2)"""
    for M in (65, 1000):
        cin, cout, co1 = 128, 128, 64
        x, dy, dw0, _, dw, _ = _rows(M, cin, cout, "split")
        xd = x.to(dev, BF).view(1, 1, M, cin)
        dy1 = dy[:, :co1].contiguous().to(dev, BF).view(1, 1, M, co1)
        dy2 = dy[:, co1:].contiguous().to(dev, BF).view(1, 1, M, cout - co1)
        out = dw0.to(dev, F32).view(cout, cin, 1, 1, 1).contiguous()
        assert K.conv_wgrad(xd, None, dy1, dy2, out, (1, M, cout, 1, 1, 1, 0, 1), 0, 0, accumulate=True) is False
        torch.cuda.synchronize()
        X.assert_exact(out.view(cout, cin), dw0 + dw, f"split-destination dW M={M}")


@pytest.mark.parametrize("nsplit", [1, 3, 7])
@pytest.mark.parametrize("M", [300, 1000])
def test_conv_wgrad_explicit_nsplit(dev, M, nsplit):
    """d: cesm_conv_wgrad accepts any nsplit >= 1: caller-sized, poisoned slabs; at M = 300 the 32-pixel-aligned splits
    of nsplit = 7 leave trailing splits without a pixel, which must still leave an exact dW and db"""
    for cin, cout in ((64, 128), (256, 256), (256, 64)):
        x, dy, dw0, db0, dw, db = _rows(M, cin, cout, nsplit)
        xd, dyd = x.to(dev, BF), dy.to(dev, BF)
        for with_db in (False, True):
            slab = nan((nsplit, cout, cin), dev)
            bslab = nan((nsplit, cout), dev) if with_db else None
            out, bout = dw0.to(dev, F32), db0.to(dev, F32)
            call("cesm_conv_wgrad", K.BF16, K.P(xd), 0, K.P(dyd), 0, K.P(out), K.P(slab), K.P(bout if with_db else None),
                 K.P(bslab), nsplit, 1, 1, M, cin, 0, 1, M, cout, cout, 1, 1, 1, 0, 1, 0, 0, 1, K.S())
            torch.cuda.synchronize()
            tag = f"cesm_conv_wgrad {cin}->{cout} M={M} nsplit={nsplit} db={with_db}"
            X.assert_exact(out, dw0 + dw, tag + ": dW")
            X.assert_exact(bout, db0 + db if with_db else db0, tag + ": db")


# ------------------------------------------------------------------ b: GroupNorm partials of the conv epilogue
GN_CHANS = sorted({c[5:8] for c in X.SWEEP_3X3_FULL + X.SWEEP_3X3_REDUCED})   # every channel set of (a)


def _gn_shapes(chan):
    """the (H, W) of every case of the 3x3 sweeps (a) with these channels"""
    return [(c[3], c[4]) for c in X.SWEEP_3X3_FULL + X.SWEEP_3X3_REDUCED if c[5:8] == chan]


@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("chan", GN_CHANS, ids=str)
def test_conv_gn_partials(dev, chan, B):
    """b: cesm_conv_fwd_gn on the shapes of (a): y exact, and the partials summed over the slot axis in float64 equal the
    exact sum of y and of y^2 per (sample, channel quad) -- the slot layout is internal, its total is not: a pixel
    counted twice or dropped on a partial tile fails.  Operands thinned to K E[x^2] E[w^2] <= 256 so that the sum of
    y^2 per (sample, quad) stays below 2^24 (asserted on the reference)."""
    c1, c2, cout = chan
    cin, Fr = c1 + c2, 3
    Nb = B * Fr
    ran = 0
    for (H, W) in _gn_shapes(chan):
        geom = (H, W, cout, 3, 3, 1, 1, 1)
        g = X.gen_for("gn", chan, B, H, W)
        x = X.ints((Nb, H, W, cin), X.X_AMAX, X.X_E2, g)
        w = X.ints((cout, cin, 1, 3, 3), 1, X.weight_e2(9 * cin, 256.0), g)
        bias = X.ints((cout,), 3, 4.0, g)
        xd = x.to(dev, BF)
        x1 = xd[..., :c1].contiguous()
        x2 = xd[..., c1:].contiguous() if c2 else None
        nslot = K.conv_gn_nslot(x1, x2, geom, B)
        if nslot <= 0:
            continue
        ran += 1
        y = X.to_cl(F.conv2d(X.to_cf(x), w[:, :, 0], bias, 1, 1))
        yq = y.view(B, Fr * H * W, cout // 4, 4)
        tot = torch.stack([yq.sum((1, 3)), (yq * yq).sum((1, 3))], -1)      # [B, cout/4, 2]
        X.check_regime([y, tot], [y], [9 * cin * X.X_AMAX + 3])   # tot < 2^24: the partial sums are exact in fp32
        wp = K.conv_pack(w.to(dev, F32), BF, cout, cin, 3, 3, 0, 0)
        yd, part = K.conv_fwd_gn(x1, x2, wp, bias.to(dev, F32), geom, B, nslot)
        torch.cuda.synchronize()
        tag = f"conv_fwd_gn {chan} B={B} {H}x{W} nslot={nslot}"
        assert part.shape == (B, nslot, cout // 4, 2)
        X.assert_exact(yd, y, tag + ": y")
        X.assert_exact(part.double().sum(1), tot, tag + ": (sum y, sum y^2) per (sample, quad)")
    # every 3x3 bf16 shape of (a) has an epilogue with partials: none is skipped
    assert ran == len(_gn_shapes(chan)) == {(64, 0, 64): 132, (64, 0, 128): 132, (512, 0, 512): 1}.get(chan, 12)


# ------------------------------------------------------------------ f: qkv_bwd
@pytest.mark.parametrize("C", [64, 128, 256, 512])
def test_qkv_bwd(dev, C):
    """f: dx = dy . W over K = 768 (dy ternary, W thinned ternary) and dw (+)= dy^T . x, onto a pre-filled dw and with
    dw = None"""
    for M in (64, 65, 1000, 3077):
        g = X.gen_for("qkv", M, C)
        dy = X.ints((M, 768), 1, X.TERNARY_E2, g)
        w = X.ints((768, C), 1, X.weight_e2(768, other_e2=X.TERNARY_E2), g)
        x = X.ints((M, C), X.X_AMAX, X.X_E2, g)
        dw0 = X.prefill((768, C), g)
        dx, dw = dy @ w, dy.t() @ x
        X.check_regime([dx, dw, dw + dw0], [dx], [768, M * X.X_AMAX])
        dyd, xd = dy.to(dev, BF), x.to(dev, BF)
        wt = w.t().contiguous().to(dev, BF)            # [C][768]: wt[c][n] = W[n][c]
        out = dw0.to(dev, F32)
        got = K.qkv_bwd(dyd, xd, wt, out, accumulate=True)
        got_nodw = K.qkv_bwd(dyd, xd, wt, None)
        over = nan((768, C), dev)
        K.qkv_bwd(dyd, xd, wt, over, accumulate=False)
        torch.cuda.synchronize()
        X.assert_exact(got, dx, f"qkv_bwd M={M} C={C}: dx")
        X.assert_exact(got_nodw, dx, f"qkv_bwd M={M} C={C}: dx (dw = None)")
        X.assert_exact(out, dw0 + dw, f"qkv_bwd M={M} C={C}: dw (+= onto integers)")
        X.assert_exact(over, dw, f"qkv_bwd M={M} C={C}: dw (overwrite)")


# ------------------------------------------------------------------ g: stem and head
STEM_HW = [(1, 1), (15, 17), (16, 32), (17, 33)]
STEM_FRAMES = [(1, 1, 1), (3, 3, 3), (3, 1, 3), (3, 3, 1), (3, 1, 1)]   # (F, Fx, Fc): per frame or broadcast


@pytest.mark.parametrize("dt", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("V", [1, 2, 3])
def test_stem(dev, V, dt):
    """g: stem_fwd, stem_wgrad (accumulating) and stem_dgrad (each output nullable); an input broadcast over the frames
    receives the gradient summed over them"""
    Bn, Co = 2, 64
    for (H, W) in STEM_HW:
        for (Fr, Fx, Fc) in STEM_FRAMES:
            for KS in (3, 7):
                g = X.gen_for("stem", V, H, W, Fr, Fx, Fc, KS)
                xt = X.ints((Bn, V, Fx, H, W), X.X_AMAX, X.X_E2, g)
                cond = X.ints((Bn, V, Fc, H, W), X.X_AMAX, X.X_E2, g)
                w = X.ints((Co, 2 * V, 1, KS, KS), 1, X.weight_e2(2 * V * KS * KS), g)
                bias = X.ints((Co,), 3, 4.0, g)
                dy = X.ints((Bn, Co, Fr, H, W), X.X_AMAX, X.X_E2, g)
                dw0 = X.prefill(tuple(w.shape), g)
                xr, cr, wr = xt.clone().requires_grad_(True), cond.clone().requires_grad_(True), w.clone().requires_grad_(True)
                xin = torch.cat([xr.expand(-1, -1, Fr, -1, -1), cr.expand(-1, -1, Fr, -1, -1)], dim=1)
                y = F.conv3d(xin, wr, bias, padding=(0, KS // 2, KS // 2))
                gx, gc, gw = torch.autograd.grad(y, (xr, cr, wr), dy)
                y = y.detach()
                nterm = Co * KS * KS * Fr
                X.check_regime([y, gx, gc, gw, gw + dw0], [y] if dt == BF else [],
                               [2 * V * KS * KS * X.X_AMAX + 3, nterm * X.X_AMAX, Bn * Fr * H * W * X.X_AMAX ** 2])
                cl = lambda t: t.permute(0, 2, 3, 4, 1).reshape(Bn * Fr, H, W, Co).contiguous()  # noqa: E731
                xtd, cd, wd = xt.to(dev, F32), cond.to(dev, F32), w.to(dev, F32)
                dyd = cl(dy).to(dev, dt)
                tag = f"stem V={V} {dt} {H}x{W} F={Fr} Fx={Fx} Fc={Fc} KS={KS}"
                yd = K.stem_fwd(xtd, cd, wd, bias.to(dev, F32), Fr, dt)
                dwd = dw0.to(dev, F32)
                K.stem_wgrad(xtd, cd, dyd, dwd, Fr, accumulate=True)
                both = K.stem_dgrad(dyd, wd, Bn, Fr, Fx, Fc)
                only_x = K.stem_dgrad(dyd, wd, Bn, Fr, Fx, Fc, want_cond=False)
                only_c = K.stem_dgrad(dyd, wd, Bn, Fr, Fx, Fc, want_xt=False)
                torch.cuda.synchronize()
                X.assert_exact(yd, cl(y), tag + ": y")
                X.assert_exact(dwd, dw0 + gw, tag + ": dW (+= onto integers)", spatial=(3, 4))
                assert only_x[1] is None and only_c[0] is None
                for name, got, want in (("dxt", both[0], gx), ("dcond", both[1], gc), ("dxt alone", only_x[0], gx),
                                        ("dcond alone", only_c[1], gc)):
                    X.assert_exact(got.reshape(want.shape), want, f"{tag}: {name}", spatial=(3, 4))


@pytest.mark.parametrize("dt", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("V", [1, 2, 3])
def test_head(dev, V, dt):
    """g: head_fwd, and head_bwd's dx (zero off the middle frame), dw and db (accumulating and overwriting)"""
    Bn, Fr = 2, 3
    for HW in (1, 7, 255, 1000):
        for C in (64, 128):
            g = X.gen_for("head", V, HW, C)
            x = X.ints((Bn, Fr, HW, C), X.X_AMAX, X.X_E2, g)
            w = X.ints((V, C), 1, X.TERNARY_E2, g)
            b = X.ints((V,), 3, 4.0, g)
            dout = X.ints((Bn, V, HW), X.X_AMAX, X.X_E2, g)
            dw0, db0 = X.prefill((V, C), g), X.prefill((V,), g)
            xm = x[:, Fr // 2]                                       # [B, HW, C]
            out = torch.einsum("bpc,vc->bvp", xm, w) + b[None, :, None]
            dx = torch.zeros_like(x)
            dx[:, Fr // 2] = torch.einsum("bvp,vc->bpc", dout, w)
            dw, db = torch.einsum("bvp,bpc->vc", dout, xm), dout.sum((0, 2))
            X.check_regime([out, dx, dw, db, dw + dw0, db + db0], [dx] if dt == BF else [],
                           [C * X.X_AMAX + 3, Bn * HW * X.X_AMAX ** 2])
            xd = x.reshape(Bn * Fr, 1, HW, C).to(dev, dt)
            wd, doutd = w.to(dev, F32), dout.reshape(Bn, V, 1, HW).to(dev, F32)
            tag = f"head V={V} {dt} HW={HW} C={C}"
            outd = K.head_fwd(xd, wd, b.to(dev, F32), Bn, Fr)
            dwd, dbd = dw0.to(dev, F32), db0.to(dev, F32)
            dxd = K.head_bwd(doutd, xd, wd, dwd, dbd, Bn, Fr, need_dx=True, accumulate=True)
            dwo, dbo = nan((V, C), dev), nan((V,), dev)
            assert K.head_bwd(doutd, xd, wd, dwo, dbo, Bn, Fr, need_dx=False, accumulate=False) is None
            torch.cuda.synchronize()
            X.assert_exact(outd.reshape(Bn, V, HW), out, tag + ": out")
            X.assert_exact(dxd.reshape(Bn, Fr, HW, C), dx, tag + ": dx")
            X.assert_exact(dwd, dw0 + dw, tag + ": dw (+=)")
            X.assert_exact(dbd, db0 + db, tag + ": db (+=)")
            X.assert_exact(dwo, dw, tag + ": dw (overwrite)")
            X.assert_exact(dbo, db, tag + ": db (overwrite)")


# ------------------------------------------------------------------ h: column sums and the small element-wise ops
@pytest.mark.parametrize("dt", DTYPES, ids=["fp32", "bf16"])
def test_colsum_add_cast(dev, dt):
    """h: K.colsum (the wrapper's split count), cesm_colsum with nsplit in {1, 7} (rows not divisible by the split), and
    K.add / K.cast on the same integers"""
    for rows in (1, 511, 1500, 5000):
        for C in (4, 68, 1024):
            g = X.gen_for("colsum", rows, C)
            x = X.ints((rows, C), X.X_AMAX, X.X_E2, g)
            d0 = X.prefill((C,), g)
            s = x.sum(0)
            X.check_regime([s, s + d0], [], [rows * X.X_AMAX])
            xd = x.to(dev, dt)
            dst = d0.to(dev, F32)
            K.colsum(xd, dst, accumulate=True)
            tag = f"colsum {dt} rows={rows} C={C}"
            outs = []
            for nsplit in (1, 7):
                o, part = nan((C,), dev), nan((nsplit, C), dev)
                call("cesm_colsum", K._DT[dt], K.P(xd), K.P(o), K.P(part), nsplit, rows, C, 0, K.S())
                outs.append((nsplit, o))
            torch.cuda.synchronize()
            X.assert_exact(dst, s + d0, tag + " (+= onto integers)")
            for nsplit, o in outs:
                X.assert_exact(o, s, f"{tag} nsplit={nsplit} (overwrite)")
    for n in (8, 8 * 1001, 8 * 70000):
        g = X.gen_for("add", n)
        a, b = X.ints((n,), 100, 3000.0, g), X.ints((n,), 100, 3000.0, g)
        X.check_regime([a + b], [a, b, a + b])
        X.assert_exact(K.add(a.to(dev, dt), b.to(dev, dt)), a + b, f"add {dt} n={n}")
    if dt == BF:
        return
    for n in (1, 255, 256 * 8192 + 3):
        a = X.ints((n,), 256, 20000.0, X.gen_for("cast", n))
        a32 = a.to(dev, F32)
        abf = K.cast(a32, BF)
        assert abf.dtype == BF
        X.assert_exact(abf, a, f"cast fp32 -> bf16 n={n}")
        X.assert_exact(K.cast(abf, F32), a, f"cast bf16 -> fp32 n={n}")
        X.assert_exact(K.cast(a32, F32), a, f"cast fp32 -> fp32 n={n}")


# ------------------------------------------------------------------ i: sensitivity
@pytest.mark.parametrize("corner", [(0, 0), (8, 32)], ids=["first", "last"])
def test_single_unit_change_is_seen_exactly(dev, corner):
    """i: one input element at an image corner changed by 1 after the reference is computed: the kernel's output differs
    from the unchanged reference on exactly the set the operation predicts (the taps' footprint x the output channels
    with a non-zero weight there) and nowhere else.  The printed relative L2 of that difference is what the 1e-2 gate of
    the tolerance-based tests lets through."""
    case = ("3x3", BF, 3, 9, 33, 64, 0, 64, True)
    c = X.ConvCase(*case)
    Nb, H, W, C = c.x.shape
    n, ci = 1, 5
    iy, ix = corner
    x = c.x.clone()
    x[n, iy, ix, ci] += 1
    delta = torch.zeros_like(c.y)
    for oy in range(max(0, iy - 1), min(H, iy + 2)):
        for ox in range(max(0, ix - 1), min(W, ix + 2)):
            delta[n, oy, ox] = c.w[:, ci, 0, iy - oy + 1, ix - ox + 1]       # y[oy] += w[ky = iy - oy + 1] x[iy]
    assert 0 < int((delta != 0).sum()) <= 4 * 64
    X.check_regime([c.y + delta], [c.y + delta])
    wp = K.conv_pack(c.w.to(dev, F32), BF, 64, 64, 3, 3, 0, 0)
    y = K.conv_fwd(x.to(dev, BF), None, wp, c.bias.to(dev, F32), (H, W, 64, 3, 3, 1, 1, 1))
    torch.cuda.synchronize()
    yc = y.double().cpu()
    assert torch.equal((yc != c.y), (delta != 0)), "the changed outputs are not the predicted set"
    X.assert_exact(y, c.y + delta, "y of the changed input")
    rel = (torch.linalg.vector_norm(yc - c.y) / torch.linalg.vector_norm(c.y)).item()
    msg = (f"one +1 at {corner}: {int((delta != 0).sum())} of {delta.numel()} outputs change, relative L2 {rel:.2e} "
           f"(the tolerance-based gate is 1e-2)")
    print(msg)   # pytest shows it with -s or -rP; DESIGN.md "Exact-data tests" records the figures
    assert rel < 1e-2, msg  # invisible to the old metric, visible here


# ------------------------------------------------------------------ the headroom band of check_regime
@pytest.mark.parametrize("amax,M", X.HEADROOM_CASES)
def test_wgrad_wide_exact_in_headroom_band(dev, amax, M):
    """Outside check_regime on purpose: wgrad_wide_kernel<128,false> (mfma_f32_16x16x32_bf16, fp32 accumulate) on
    integers up to +-256 with 2^22 <= max sum |a||b| < 2^24, the band the regime's two bits of headroom leave out.
    Every partial sum is below 2^24, so the result is exact if the MFMA adder keeps all 24 bits in any grouping.  It
    does on an MI355X (DESIGN.md "Exact-data tests").  A failure here alone, with the sweeps passing, says that the
    adder drops low bits when it aligns addends -- the reason check_regime stops at 2^22 -- not that a term is lost."""
    cin, cout = X.HEADROOM_CH
    x, dy, dw, _ = X.headroom_case(amax, M)
    assert K.conv_wgrad_variant(BF, 1, 1, M, cin, 0, 1, M, cout, cout, 1, 1, 1, 0, 1) == "wgrad_wide_kernel<128,false>"
    xd, dyd = x.to(dev, BF), dy.to(dev, BF)
    for nsplit in (1, 3):
        out, slab = nan((cout, cin), dev), nan((nsplit, cout, cin), dev)
        call("cesm_conv_wgrad", K.BF16, K.P(xd), 0, K.P(dyd), 0, K.P(out), K.P(slab), 0, 0, nsplit, 1, 1, M, cin, 0, 1, M,
             cout, cout, 1, 1, 1, 0, 1, 0, 0, 0, K.S())
        torch.cuda.synchronize()
        X.assert_exact(out, dw, f"headroom band amax={amax} M={M} nsplit={nsplit}: dW")
