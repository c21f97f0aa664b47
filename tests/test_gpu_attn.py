"""The attention kernels against float64, judged per slice and per element (tests/attn_ref.py) at every regime of
their launch plans (which case sits in which regime: tests/test_attn_host.py): the MFMA temporal core
(cesm_tflash_fwd / _bwd), the VALU temporal core (cesm_tattn_fwd / _bwd, fp32 and the bf16 instantiation no wrapper
reaches), the SLA core (cesm_sla_fwd / _bwd) and the fused temporal block (cesm_tblock_fwd / _bwd, _fwd_fold /
_bwd_dw), the last judged on the attention branch alone (y - x, dx - dy).

Every output and workspace a kernels.* wrapper allocates starts NaN-filled (the `poisoned` fixture of
test_gpu_norm.py), the buffers of the direct calls are poisoned by hand, and destinations that accumulate (dtable,
dgamma, dwqkv) hold finite non-zero values first.  The float64 reference and its bf16 emulation / float32 evaluation
run on the device.  Each test prints its worst err / tol with the err and the e16 / e32 that went with it
(profiles/attn_parity.txt).
"""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn_ref as A  # noqa: E402
from attn_ref import BF, F32, LN2, SCALE  # noqa: E402
from test_gpu_norm import garbage, nan, poisoned  # noqa: E402,F401  (poisoned: autouse here too)
from cesm_emulator_amd import kernels as K  # noqa: E402
from cesm_emulator_amd._lib import call, lib  # noqa: E402
from cesm_emulator_amd.kernels import P, S  # noqa: E402

pytestmark = pytest.mark.gpu

CESM_DT = {F32: 0, BF: 1}


def tables(inp, F, dev, md=32):
    """the kernels' expanded bias and RoPE table; the bias is an exact gather"""
    bias = K.relpos_fwd(inp["table"], F, 32, md)
    assert torch.equal(bias, A.bias_from_table(inp["table"], F, 32, md))
    return bias, K.rope_table(A.rope_freqs(dev), F)


def core_got(out, lse, dqkv, B, F, HW, log2=False, pixel_major=False):
    """kernel results in the slice layout, lse in nats"""
    got = dict(o=A.rows_core(out, B, F, HW)[0])
    if lse is not None:
        got["lse"] = lse.permute(0, 2, 1, 3) * (LN2 if log2 else 1.0)
    if dqkv is not None:
        got["dq"], got["dk"], got["dv"] = A.rows_core(dqkv, B, F, HW, pixel_major)
    return got


# ------------------------------------------------------------------------------------------ MFMA temporal core
@pytest.mark.parametrize("case", list(A.MFMA_CASES), ids=A.case_id)
def test_mfma_core(dev, case):
    """K.tattn_fwd / K.tattn_bwd in bf16: out, lse, dq / dk / dv and dtable (accumulated over garbage), frame-major and
    (nt >= 2) pixel-major qkv, each against float64; save=False and dtable=None give bit-identical results"""
    B, F, HW, md = case
    inp = A.tcore_inputs(case, BF, dev)
    r, e = A.tcore_ref(inp, max_distance=md), A.tcore_ref(inp, "e16", max_distance=md)
    bias, rot = tables(inp, F, dev, md)
    assert K._tflash(inp["qkv"], F)
    g = A.pixel_group(F)
    v = []
    for pm in ((False, True) if F > 16 else (False,)):
        tag = "pixel-major" if pm else "frame-major"
        qkv = inp["qkv"].view(B, F, HW, 768).transpose(1, 2).reshape(-1, 768).contiguous() if pm else inp["qkv"]
        out, lse = K.tattn_fwd(qkv, bias, rot, B, F, HW, SCALE, pixel_major=pm)
        prior = garbage((32, 8), dev, 5)
        dtable = prior.clone()
        dqkv = K.tattn_bwd(qkv, out, inp["dout"], lse, bias, rot, dtable, B, F, HW, SCALE, 32, md, pixel_major=pm)
        v += A.judge_core(tag, core_got(out, lse, dqkv, B, F, HW, True, pm), r, e, BF, g)
        v += A.judge_dtable(tag, dtable, prior, r, e, BF, F, 32, md)
        out2, lse2 = K.tattn_fwd(qkv, bias, rot, B, F, HW, SCALE, save=False, pixel_major=pm)
        assert lse2 is None and torch.equal(out2, out)
        dqkv2 = K.tattn_bwd(qkv, out, inp["dout"], lse, bias, rot, None, B, F, HW, SCALE, 32, md, pixel_major=pm)
        assert torch.equal(dqkv2, dqkv)
    A.report(f"mfma core {A.case_id(case)}", v)


@pytest.mark.parametrize("case", [(3, 7, 5, 32), (1, 64, 5, 128)], ids=A.case_id)
def test_mfma_bwd_overwrites_dtable(dev, case):
    """cesm_tflash_bwd itself with accumulate = 0 over a NaN dtable (both backward forms)"""
    B, F, HW, md = case
    inp = A.tcore_inputs(case, BF, dev)
    r, e = A.tcore_ref(inp, max_distance=md), A.tcore_ref(inp, "e16", max_distance=md)
    bias, rot = tables(inp, F, dev, md)
    out, lse = K.tattn_fwd(inp["qkv"], bias, rot, B, F, HW, SCALE)
    nblk = lib().cesm_tflash_nblk(HW)
    dqkv, dtable = nan(inp["qkv"].shape, dev, BF), nan((32, 8), dev)
    dbuf, part, off = nan((B, 8, HW, F), dev), nan((B * 8 * nblk * (2 * F - 1),), dev), nan((8 * (2 * F - 1),), dev)
    call("cesm_tflash_bwd", P(inp["qkv"]), P(out), P(inp["dout"]), P(lse), P(bias), P(rot), P(dqkv), P(dtable), P(dbuf),
         P(part), P(off), B, F, HW, float(SCALE), 32, md, 0, 0, S())
    v = A.judge_core("direct", core_got(out, None, dqkv, B, F, HW), r, e, BF, A.pixel_group(F), names=("dq", "dk", "dv"))
    v += A.judge_dtable("direct", dtable, torch.zeros_like(dtable), r, e, BF, F, 32, md)
    A.report(f"mfma bwd accumulate=0 {A.case_id(case)}", v)


# ------------------------------------------------------------------------------------------ VALU temporal core
def valu_run(inp, bias, rot, dtable, dev):
    """fp32 through the wrappers; bf16 through the C entry points (K.tattn_fwd sends bf16 to the MFMA core)"""
    B, F, HW = inp["case"]
    qkv, dout = inp["qkv"], inp["dout"]
    if inp["dt"] == F32:
        out, lse = K.tattn_fwd(qkv, bias, rot, B, F, HW, SCALE)
        return out, lse, K.tattn_bwd(qkv, out, dout, lse, bias, rot, dtable, B, F, HW, SCALE)
    out, lse = nan((qkv.shape[0], 256), dev, BF), nan((B, 8, HW, F), dev)
    call("cesm_tattn_fwd", CESM_DT[BF], P(qkv), P(bias), P(rot), P(out), P(lse), B, F, HW, float(SCALE), S())
    nblk = lib().cesm_tattn_nblk(F, HW)
    dqkv, part, ws = nan(qkv.shape, dev, BF), nan((B * 8 * nblk, F, F), dev), nan((8, F, F), dev)
    call("cesm_tattn_bwd", CESM_DT[BF], P(qkv), P(out), P(dout), P(lse), P(bias), P(rot), P(dqkv), P(part), B, F, HW,
         float(SCALE), S())
    call("cesm_relpos_bwd", P(part), nblk, B, P(dtable), P(ws), F, 8, 32, 32, 1, S())
    return out, lse, dqkv


@pytest.mark.parametrize("dt", A.DTYPES, ids=A.dt_id)
@pytest.mark.parametrize("case", list(A.VALU_CASES), ids=A.case_id)
def test_valu_core(dev, case, dt):
    B, F, HW = case
    inp = A.tcore_inputs(case, dt, dev)
    r, e = A.tcore_ref(inp), A.tcore_ref(inp, "r32" if dt == F32 else "e16")
    bias, rot = tables(inp, F, dev)
    assert dt == BF or not K._tflash(inp["qkv"], F)
    prior = garbage((32, 8), dev, 6)
    dtable = prior.clone()
    out, lse, dqkv = valu_run(inp, bias, rot, dtable, dev)
    v = A.judge_core("valu", core_got(out, lse, dqkv, B, F, HW), r, e, dt, A.pixel_group(F))
    v += A.judge_dtable("valu", dtable, prior, r, e, dt, F)
    A.report(f"valu core {A.dt_id(dt)} {A.case_id(case)}", v)


# ------------------------------------------------------------------------------------------ SLA core
@pytest.mark.parametrize("dt", A.DTYPES, ids=A.dt_id)
@pytest.mark.parametrize("case", A.SLA_CASES, ids=A.case_id)
def test_sla_core(dev, case, dt):
    """K.sla_fwd / K.sla_bwd: out, ctx, the k-softmax statistic m + log l, dq / dk / dv"""
    Nf, HW = case
    inp = A.sla_inputs(case, dt, dev)
    mode = "r32" if dt == F32 else "e16"
    r, e = A.sla_eval(inp), A.sla_eval(inp, mode)
    out, ctx, ml = K.sla_fwd(inp["qkv"], Nf, HW, SCALE)
    dqkv = K.sla_bwd(inp["qkv"], inp["dout"], ctx, ml, Nf, HW, SCALE)
    got = dict(zip(("dq", "dk", "dv"), A.rows_sla(dqkv, Nf, HW)), out=A.rows_sla(out, Nf, HW)[0])
    v = []
    for nm in ("out", "dq", "dk", "dv"):
        if HW == 1 and nm in ("dq", "dk"):
            # one position: both vanish by cancellation (dq over d; dk = ks (dks - sum ks dks) with ks = 1, which the
            # kernels leave at an fp32 residue of the two sums, ~5e-8 of the terms): judged against the rms of the terms
            worst = float(got[nm].double().abs().max()) / float(r[nm + "_terms"])
            v.append(A.Verdict(f"sla {nm}", worst / A.BOUND_BWD[dt], worst, 0.0, "max |.| over the rms of the cancelling terms"))
            continue
        rr, sid, n = A.sla_slices(r[nm])
        v.append(A.judge(f"sla {nm}", A.sla_slices(got[nm])[0], rr, sid, n,
                         (A.BOUND_FWD if nm == "out" else A.BOUND_BWD)[dt], A.sla_slices(e[nm])[0], dt))
    # ctx and the statistic are fp32 results of fp32 sums in both modes: the fp32 rule, 1e-4 / 1e-5 with 8 * e32
    r32 = e if dt == F32 else A.sla_eval(inp, "r32", backward=False)
    v.append(A.judge("sla ctx", ctx.reshape(Nf * 8, 1024), r["ctx"].reshape(Nf * 8, 1024), None, Nf * 8, A.BOUND_STAT,
                     r32["ctx"].reshape(Nf * 8, 1024), F32))
    stat = ml[..., 0] + torch.log(ml[..., 1])
    v.append(A.judge_lse("sla stat", stat, r["stat"], None, 0, r32["stat"], F32))
    A.report(f"sla core {A.dt_id(dt)} {A.case_id(case)}", v)


# ------------------------------------------------------------------------------------------ fused temporal block
def block_weights(inp):
    C = inp["case"][3]
    w, wo = inp["wqkv"].contiguous(), inp["wout"].contiguous()
    return dict(wq=K.conv_pack(w, BF, 768, C, 1, 1, 0, 0), wo=K.conv_pack(wo, BF, C, 256, 1, 1, 0, 0),
                wq_t=K.conv_pack(w, BF, C, 768, 1, 1, 1, 1), wo_t=K.conv_pack(wo, BF, 256, C, 1, 1, 1, 1))


def judge_block_fwd(tag, inp, r, e, y, mr, lse, o):
    B, F, HW, C = inp["case"]
    g = A.pixel_group(F)
    assert A._rms(r["branch"]) >= 0.5 * A._rms(inp["x"])  # else the allowance below swallows the branch
    x = inp["x"].double()
    rr, sid, n = A.block_slices(r["branch"], B, F, HW, g)
    v = [A.judge(f"{tag} y - x", y.reshape(-1, C).double() - x, rr, sid, n, A.BOUND_FWD[BF], e["y"] - x, BF,
                 allow=2.0 ** -8 * r["y"].abs())]
    got = dict(lse=lse.permute(0, 2, 1, 3) * (LN2 if C <= 256 else 1.0))
    if o is not None:
        got["o"] = A.rows_core(o.reshape(-1, 256), B, F, HW)[0]
    v += A.judge_core(tag, got, r, e, BF, g, names=("o", "lse"))
    torch.testing.assert_close(mr[:, 0].double(), r["mean"], rtol=A.BOUND_STAT, atol=A.BOUND_STAT)
    torch.testing.assert_close(mr[:, 1].double(), r["rstd"], rtol=A.BOUND_STAT, atol=A.BOUND_STAT)
    return v


def judge_block_bwd(tag, inp, r, e, dx, o, dgamma, dtable, dwqkv, priors):
    """dgamma, dtable, dwqkv as accumulated over priors (dwqkv: a float64 product has the prior 0)"""
    B, F, HW, C = inp["case"]
    g = A.pixel_group(F)
    assert A._rms(r["dxb"]) >= 0.5 * A._rms(inp["dy"])
    dy = inp["dy"].double()
    rr, sid, n = A.block_slices(r["dxb"], B, F, HW, g)
    v = [A.judge(f"{tag} dx - dy", dx.reshape(-1, C).double() - dy, rr, sid, n, A.BOUND_BWD[BF], e["dx"] - dy, BF,
                 allow=2.0 ** -8 * r["dx"].abs())]
    v.append(A.judge_cols(f"{tag} dgamma", (dgamma.double() - priors["dgamma"].double())[None], r["dgamma"][None],
                          A.BOUND_BWD[BF], e["dgamma"][None], BF))
    v += A.judge_dtable(tag, dtable, priors["dtable"], r, e, BF, F)
    v.append(A.judge_cols(f"{tag} dWqkv", dwqkv.double() - priors["dwqkv"], r["dwqkv"], A.BOUND_BWD[BF], e["dwqkv"], BF))
    if o is not None:
        o = o.reshape(-1, 256)
        v += A.judge_core(f"{tag} bwd", dict(o=A.rows_core(o, B, F, HW)[0]), r, e, BF, g, names=("o",))
        v.append(A.judge_cols(f"{tag} dWout", dy.t() @ o.double(), r["dwout"], A.BOUND_BWD[BF], e["dwout"], BF))
    return v


@pytest.mark.parametrize("case", list(A.TBLOCK_CASES) + [A.TBLOCK_STRIDE_CASE], ids=A.case_id)
def test_fused_block(dev, case):
    """K.tblock_fwd / K.tblock_bwd on the branch alone: y - x, o (the forward's with save_o, the backward's emission),
    mr, lse, dx - dy, dq / dk / dv (the emitted dqkv), dgamma, dtable, dW_qkv = dqkv^T xn, dW_out = dy^T o; emit_o=False leaves dx and dqkv as they are"""
    B, F, HW, C = case
    inp = A.tblock_inputs(case, dev)
    r, e = A.tblock_eval(inp), A.tblock_eval(inp, "e16")
    bias, rot = tables(inp, F, dev)
    w = block_weights(inp)
    x4, dy4 = inp["x"].view(B * F, 1, HW, C), inp["dy"].view(B * F, 1, HW, C)
    save_o = C <= 256
    y, mr, lse, o_fwd = K.tblock_fwd(x4, inp["gamma"], w["wq"], w["wo"], bias, rot, B, F, SCALE, save_o=save_o)
    v = judge_block_fwd("tblock", inp, r, e, y, mr, lse, o_fwd)
    y2, _, _, o2 = K.tblock_fwd(x4, inp["gamma"], w["wq"], w["wo"], bias, rot, B, F, SCALE, save=False)
    assert o2 is None and torch.equal(y2, y)
    priors = dict(dgamma=garbage((C,), dev, 7), dtable=garbage((32, 8), dev, 8), dwqkv=0.0)
    dgamma, dtable = priors["dgamma"].clone(), priors["dtable"].clone()
    dx, dqkv, o, xn = K.tblock_bwd(x4, dy4, inp["gamma"], mr, lse, w["wq"], w["wq_t"], w["wo_t"], bias, rot, dgamma,
                                   dtable, B, F, SCALE)
    dwq = dqkv.reshape(-1, 768).double().t() @ xn.reshape(-1, C).double()
    v += judge_block_bwd("tblock", inp, r, e, dx, o, dgamma, dtable, dwq, priors)
    got = dict(zip(("dq", "dk", "dv"), A.rows_core(dqkv.reshape(-1, 768), B, F, HW)))
    v += A.judge_core("tblock", got, r, e, BF, A.pixel_group(F), names=("dq", "dk", "dv"))
    dx2, dqkv2, o2, _ = K.tblock_bwd(x4, dy4, inp["gamma"], mr, lse, w["wq"], w["wq_t"], w["wo_t"], bias, rot, None, None,
                                     B, F, SCALE, emit_o=False)
    assert o2 is None
    rr, sid, n = A.block_slices(r["dxb"], B, F, HW, A.pixel_group(F))
    dy = inp["dy"].double()
    v.append(A.judge("tblock dx - dy (emit_o=False)", dx2.reshape(-1, C).double() - dy, rr, sid, n, A.BOUND_BWD[BF],
                     e["dx"] - dy, BF, allow=2.0 ** -8 * r["dx"].abs()))
    v.append(A.judge_cols("tblock dWqkv (emit_o=False)", dqkv2.reshape(-1, 768).double().t() @ xn.reshape(-1, C).double(),
                          r["dwqkv"], A.BOUND_BWD[BF], e["dwqkv"], BF))
    A.report(f"fused block {A.case_id(case)}", v)


DW_CASES = [c for c in A.TBLOCK_CASES if c[3] == 64 and c[1] in A.TBLOCK_DW_F] + A.TBLOCK_DW_CASES


@pytest.mark.parametrize("case", DW_CASES, ids=A.case_id)
def test_fused_block_fold_dw(dev, case):
    """K.tblock_fwd_fold / K.tblock_bwd_dw (gamma folded into to_qkv, in-kernel dW_qkv / dgamma over garbage)"""
    B, F, HW, C = case
    assert K.tblock_bwd_dw_supported(B, F, HW, C) and not K.tblock_bwd_dw_supported(B, 13, HW, C)
    inp = A.tblock_inputs(case, dev)
    r, e = A.tblock_eval(inp, fold=True), A.tblock_eval(inp, "e16", fold=True)
    bias, rot = tables(inp, F, dev)
    w = block_weights(inp)
    x4, dy4 = inp["x"].view(B * F, 1, HW, C), inp["dy"].view(B * F, 1, HW, C)
    wqkv = inp["wqkv"].contiguous()
    y, mr, lse, o_fwd = K.tblock_fwd_fold(x4, inp["gamma"], wqkv, w["wo"], bias, rot, B, F, SCALE, save_o=True)
    v = judge_block_fwd("fold", inp, r, e, y, mr, lse, o_fwd)
    priors = dict(dgamma=garbage((C,), dev, 7), dtable=garbage((32, 8), dev, 8), dwqkv=garbage((768, C), dev, 9))
    dgamma, dtable, dwq = priors["dgamma"].clone(), priors["dtable"].clone(), priors["dwqkv"].clone()
    dx, ob = K.tblock_bwd_dw(x4, dy4, mr, lse, wqkv, inp["gamma"], w["wo_t"], bias, rot, dwq, dgamma, dtable, B, F,
                             SCALE, emit_o=True)
    v += judge_block_bwd("dw", inp, r, e, dx, ob, dgamma, dtable, dwq, priors)
    dx2 = K.tblock_bwd_dw(x4, dy4, mr, lse, wqkv, inp["gamma"], w["wo_t"], bias, rot, None, None, None, B, F, SCALE)
    assert torch.equal(dx2, dx)
    A.report(f"fused block fold/dw {A.case_id(case)}", v)
