"""CPU checks behind the attention-kernel parity tests (tests/test_gpu_attn.py): the launch-plan regime of every case,
asserted from the library's host-only queries and the documented formulas; the float64 references against autograd
and the CPU oracle; the teeth of the per-slice judge; and the conditions on the bf16 emulation that keep the rule
tol = max(bound, 4 * e16) from hiding a failure."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn_ref as A  # noqa: E402
from attn_ref import BF, F32  # noqa: E402
from cesm_emulator_amd._lib import lib  # noqa: E402
from oracle import ref_cpu as R  # noqa: E402


# ------------------------------------------------------------------------------------------ plan regimes
@pytest.mark.parametrize("case", list(A.MFMA_CASES), ids=A.case_id)
def test_mfma_case_regime(case):
    B, F, HW, md = case
    want = A.MFMA_CASES[case]
    assert lib().cesm_tflash_supported(F) == 1
    assert want["nt"] == -(-F // 16)
    name = lib().cesm_tflash_bwd_variant(F, HW).decode()
    if want["bwd"] == "fused":
        assert name == f"tflash_bwd_fused_kernel<{want['nt']}>"
    else:
        assert name == "tflash_bwd_q_kernel<1>" and want["nt"] == 1
    assert lib().cesm_tflash_bwd_nd(F, 32, md) == want["nd"]
    assert lib().cesm_tflash_nblk(HW) == 128  # pixel-pair streams per (sample, head pair)


def test_mfma_regimes_are_all_there():
    have = A.MFMA_CASES
    assert {c[1] for c in have} == A.MFMA_F and {c[2] for c in have} == A.MFMA_HW
    assert {w["nt"] for w in have.values()} == set(range(1, 9))
    assert {w["bwd"] for w in have.values()} == {"two", "fused"}
    assert {c[1] for c in have if c[1] in (7, 8)} == {7, 8}  # both sides of the two-kernel / fused switch
    for hw in A.MFMA_HW:  # every HW with a window below 8 frames, one of 8..16 and one of 64 or more
        fs = {c[1] for c in have if c[2] == hw}
        assert any(f < 8 for f in fs) and any(8 <= f <= 16 for f in fs) and any(f >= 64 for f in fs), hw
    assert {c[1] for c in have if c[2] == 257} >= {120, 128}
    assert {c[0] for c in have} == {1, 3}
    assert {c[1] for c in have if c[3] == 128} == {64, 81, 120, 128}
    # both ND forms of the fused backward for NT >= 4: saturated (ND = 2) and exact (ND = NT - 1), per NT where the
    # cases have both
    for nt in (4, 6, 8):
        assert {w["nd"] for w in have.values() if w["nt"] == nt} == {2, nt - 1}, nt
    assert all(w["nd"] == 2 for w in have.values() if w["nt"] in (5, 7))
    # HW against the fused backward's 128 pixel-pair streams: half a pair, an odd count, a stream without a pixel, all
    # streams with exactly one pair, one stream with a second (half) pair
    assert {1, 255, 256, 257} <= A.MFMA_HW


def test_tflash_bwd_nd_query():
    """the ND the launcher instantiates: -1 without a fused kernel, NT - 1 below NT = 4, and for NT >= 4 the
    saturated form exactly when every offset beyond two diagonals shares the last bucket"""
    q = lib().cesm_tflash_bwd_nd
    assert q(0, 32, 32) == -1 and q(129, 32, 32) == -1 and q(7, 32, 32) == -1
    for F in range(8, 129):
        nt = -(-F // 16)
        for md in (32, 128):
            nd = q(F, 32, md)
            if nt < 4:
                assert nd == nt - 1
                continue
            bm = A.bucket_map(F, 32, md)
            far = [bm[0, n] == bm[0, F - 1] and bm[n, 0] == bm[F - 1, 0] for n in range(33, F)]
            assert nd in (2, nt - 1)
            if nd == 2:  # the saturated form is only ever chosen where it is exact
                assert all(far), (F, md)
    assert q(120, 32, 32) == 2 and q(120, 32, 128) == 7 and q(64, 32, 128) == 3


@pytest.mark.parametrize("case", list(A.VALU_CASES), ids=A.case_id)
def test_valu_case_regime(case):
    B, F, HW = case
    want = A.VALU_CASES[case]
    G = 128 // F
    assert want["G"] == G
    npb = -(-HW // G)
    assert lib().cesm_tattn_nblk(F, HW) == want["nblk"] == min(npb, 256)
    assert want["vlds"] == (F > 32)
    assert want["ragged"] == (HW % G != 0)
    assert want["stride"] == (npb > 256)


def test_valu_regimes_are_all_there():
    have = A.VALU_CASES
    assert {w["G"] for w in have.values()} >= {128, 64, 10, 4, 3, 2, 1}
    assert {w["vlds"] for w in have.values()} == {False, True}
    assert any(w["stride"] and not w["vlds"] for w in have.values())
    assert any(w["stride"] and w["vlds"] and w["G"] == 2 for w in have.values())
    assert any(w["stride"] and w["G"] == 1 for w in have.values())
    assert any(c[2] < w["G"] for c, w in have.items())  # fewer pixels than one block's groups
    assert {c[1] for c in have} >= {32, 33, 128}


@pytest.mark.parametrize("hw", list(A.SLA_HW))
def test_sla_case_regime(hw):
    want = A.SLA_HW[hw]
    n = lib().cesm_sla_nchunk(hw)
    assert n == want["nchunk"] == -(-hw // 2048)
    assert want["last"] == hw - (n - 1) * 2048
    assert want["tile"] == (hw - 1) % 64 + 1


def test_tblock_case_regimes():
    for (B, F, HW, C), want in A.TBLOCK_CASES.items():
        if C <= 256:
            pw = {64: 4, 128: 2, 256: 1}[C]
            assert want["nv"] == -(-pw * F // 16)
        assert lib().cesm_tblock_bwd_nblk(B, F, HW, C) >= 1
        assert (lib().cesm_tblock_bwd_dw_nblk(B, F, HW, C) > 0) == (C == 64 and F in A.TBLOCK_DW_F)
    nv = {C: {w["nv"] for c, w in A.TBLOCK_CASES.items() if c[3] == C} for C in (64, 128, 256)}
    assert nv == {64: {1, 2, 3, 4}, 128: {1, 2}, 256: {1}}  # every nv each C supports (F <= 16)
    assert {c[1] for c in A.TBLOCK_CASES if c[3] == 64} == {1, 4, 5, 8, 9, 12, 13, 16}
    assert {c[2] for c in A.TBLOCK_CASES} == {1, 15, 16, 17, 35}
    assert lib().cesm_tblock_bwd_dw_nblk(2, 13, 15, 64) == 0  # 4 F > 48: tw_bwd<64, 4> takes over
    B, F, HW, C = A.TBLOCK_STRIDE_CASE
    groups = -(-(-(-HW // 4)) // 4)  # blocks of 4 waves, a wave a group of 4 pixels
    assert lib().cesm_tblock_bwd_nblk(B, F, HW, C) < groups
    (B1, F1, HW1, _), (B2, F2, HW2, _) = A.TBLOCK_DW_CASES
    assert 0 < lib().cesm_tblock_bwd_dw_nblk(B1, F1, HW1, 64) < B1 * -(-HW1 // 4)
    assert lib().cesm_tblock_bwd_dw_nblk(B2, F2, HW2, 64) == B2 * -(-HW2 // 4)


# ------------------------------------------------------------------------------------------ references
@pytest.mark.parametrize("md", [32, 128])
@pytest.mark.parametrize("F", [1, 2, 12, 40, 128])
def test_bucket_map_and_dtable_scatter_match_oracle(F, md):
    pos = torch.arange(F)
    assert torch.equal(A.bucket_map(F, 32, md), R.RelativePositionBias.bucket(pos[None, :] - pos[:, None], 32, md))
    rp = R.RelativePositionBias(8, 32, md).double()
    g = torch.randn(8, F, F, dtype=torch.float64, generator=torch.Generator().manual_seed(F))
    (rp(F) * g).sum().backward()
    want = rp.relative_attention_bias.weight.grad
    assert (A.dtable_from_dbias(g, 32, md) - want).abs().max() <= 1e-10
    assert torch.equal(A.bias_from_table(rp.relative_attention_bias.weight.detach(), F, 32, md), rp(F).detach())
    assert torch.equal(want.abs().sum(1) > 0, A.reached_buckets(F, 32, md))


@pytest.mark.parametrize("case,md", [((2, 1, 5), 32), ((2, 3, 9), 32), ((2, 12, 7), 128), ((1, 40, 3), 32),
                                     ((1, 120, 2), 128)], ids=str)
def test_core_closed_form_matches_autograd(case, md):
    inp = A.tcore_inputs(case, BF)
    r = A.tcore_ref(inp, max_distance=md)
    a = A.tcore_autograd(inp, max_distance=md)
    for n in ("o", "dq", "dk", "dv", "dtable"):
        assert (r[n] - a[n]).abs().max() <= 1e-10, n
    # the forward formula is the oracle's Attention core (video_net.py:401-453)
    B, F, HW = case
    att = R.Attention(64, 8, 32, R.RotaryEmbedding(32)).double()
    q, k, v = (t.permute(0, 1, 3, 2, 4) for t in A.rows_core(inp["qkv"].double(), B, F, HW))  # b, p, F, h, d
    qkv = torch.cat([t.reshape(B, HW, F, 256) for t in (q, k, v)], -1)
    att.to_qkv, att.to_out = torch.nn.Identity(), torch.nn.Identity()
    o = att(qkv, pos_bias=A.bias_from_table(inp["table"].double(), F, 32, md))  # b, p, F, 256
    assert (o.reshape(B, HW, F, 8, 32).permute(0, 1, 3, 2, 4) - r["o"]).abs().max() <= 1e-10
    # lse against an independent form: logsumexp of the scores built with the oracle's rotary embedding
    rot = R.RotaryEmbedding(32).double()
    q4, k4, _ = A.rows_core(inp["qkv"].double(), B, F, HW)
    sim = torch.einsum("bphid,bphjd->bphij", rot.rotate_queries_or_keys(q4 * A.SCALE), rot.rotate_queries_or_keys(k4))
    sim = sim + A.bias_from_table(inp["table"].double(), F, 32, md)
    assert (torch.logsumexp(sim, -1) - r["lse"]).abs().max() <= 1e-10
    # pixel-major rows are the same pixels in another order
    if F > 1:
        pm = A.tcore_ref(dict(inp, qkv=inp["qkv"].view(B, F, HW, 768).transpose(1, 2).reshape(-1, 768)),
                         max_distance=md, pixel_major=True)
        assert all(torch.equal(pm[n], r[n]) for n in ("o", "dq", "lse"))


def test_sla_closed_form_matches_autograd_and_oracle():
    for case in [(2, 1), (2, 7), (1, 130)]:
        inp = A.sla_inputs(case, BF)
        r, a = A.sla_eval(inp), A.sla_autograd(inp)
        for n in ("out", "ctx", "dk", "dv"):
            assert (r[n] - a[n]).abs().max() <= 1e-10, n
        assert (r["dq"] - a["dq"]).abs().max() <= 1e-10 * max(1.0, float(r["dq_terms"]))
        k_ = A.rows_sla(inp["qkv"].double(), *case)[1]  # [Nf, h, n, d]
        assert (torch.logsumexp(k_, -2) - r["stat"]).abs().max() <= 1e-10
        Nf, HW = case
        m = R.SpatialLinearAttention(768, 8, 32).double()  # to_qkv = identity, to_out = the first 256 channels
        with torch.no_grad():
            m.to_qkv.weight.copy_(torch.eye(768).view(768, 768, 1, 1))
            m.to_out.weight.zero_()
            m.to_out.weight[:256].copy_(torch.eye(256).view(256, 256, 1, 1))
            m.to_out.bias.zero_()
            o = m(inp["qkv"].double().view(1, Nf, HW, 1, 768).permute(0, 4, 1, 2, 3))[0, :256, :, :, 0]  # (h e), f, n
        o = o.reshape(8, 32, Nf, HW).permute(2, 0, 3, 1)
        assert (o - r["out"]).abs().max() <= 1e-10


@pytest.mark.parametrize("case", [(2, 1, 3, 64), (2, 5, 6, 64), (1, 12, 4, 128)], ids=A.case_id)
def test_block_reference_matches_oracle(case):
    B, F, HW, C = case
    inp = A.tblock_inputs(case)
    ref = R.Residual(R.PreNorm(C, R.EinopsToAndFrom(R.Attention(C, 8, 32, R.RotaryEmbedding(32))))).double()
    ref.fn.norm.gamma.data.copy_(inp["gamma"].double().view_as(ref.fn.norm.gamma))
    att = ref.fn.fn.fn
    att.to_qkv.weight.data.copy_(inp["wqkv"].double())
    att.to_out.weight.data.copy_(inp["wout"].double())
    rp = R.RelativePositionBias(8, 32, 32).double()
    rp.relative_attention_bias.weight.data.copy_(inp["table"].double())
    x = inp["x"].double().view(B, F, 1, HW, C).permute(0, 4, 1, 2, 3).requires_grad_(True)  # b c f h w
    y = ref(x, pos_bias=rp(F))
    dy = inp["dy"].double().view(B, F, 1, HW, C).permute(0, 4, 1, 2, 3)
    (y * dy).sum().backward()

    def rows(t):
        return t.permute(0, 2, 3, 4, 1).reshape(B * F * HW, C)
    for fold in (False, True):
        r = A.tblock_eval(inp, fold=fold)
        want = dict(y=rows(y.detach()), dx=rows(x.grad), dwqkv=att.to_qkv.weight.grad, dwout=att.to_out.weight.grad,
                    dgamma=ref.fn.norm.gamma.grad.reshape(-1), dtable=rp.relative_attention_bias.weight.grad)
        for n, w in want.items():
            assert (r[n] - w).abs().max() <= 1e-10 * max(1.0, float(w.abs().max())), (n, fold)
        assert (r["branch"] - (want["y"] - inp["x"].double())).abs().max() <= 1e-10
        assert (r["dxb"] - (want["dx"] - inp["dy"].double())).abs().max() <= 1e-10
    # the precondition of the branch allowance: neither the branch nor its input gradient is swallowed by the residual
    assert A._rms(r["branch"]) >= 0.5 * A._rms(inp["x"]) and A._rms(r["dxb"]) >= 0.5 * A._rms(inp["dy"])


# ------------------------------------------------------------------------------------------ judge has teeth
TEETH = (2, 120, 64)


@pytest.fixture(scope="module")
def teeth():
    inp = A.tcore_inputs(TEETH, BF)
    return inp, A.tcore_ref(inp), A.tcore_ref(inp, "e16")


def _whole_dqkv(got, r):
    return A.whole_l2(torch.cat([got[n] for n in ("dq", "dk", "dv")], -1), torch.cat([r[n] for n in ("dq", "dk", "dv")], -1))


def _refused(name, got, r, e, whole, gate, nm):
    v = A.judge_core("teeth", {nm: got}, r, e, BF, A.pixel_group(TEETH[1]), names=(nm,))[0]
    print(f"attn_teeth {name}: whole-tensor L2 {whole:.3g} (old gate {gate}), judge {v}")
    assert whole < gate, name
    assert not v.ok, name
    return v


def test_judge_passes_the_emulation(teeth):
    inp, r, e = teeth
    assert all(v.ok for v in A.judge_core("e16", e, r, e, BF, 1))
    r32 = A.tcore_ref(dict(inp, qkv=inp["qkv"].float(), dout=inp["dout"].float()), "r32")
    assert all(v.ok for v in A.judge_core("r32", r32, r, r32, F32, 1))


def test_judge_rejects_one_zeroed_pixel_head(teeth):
    _, r, e = teeth
    got = {n: r[n].clone() for n in ("dq", "dk", "dv")}
    got["dq"][1, 37, 5] = 0
    v = _refused("one (pixel, head) slice of dq zeroed", got["dq"], r, e, _whole_dqkv(got, r), 3e-2, "dq")
    assert "L2" in v.what


def test_judge_rejects_rows_of_the_neighbouring_pixel(teeth):
    _, r, e = teeth
    o = r["o"].clone()
    o[0, 20, 3, 77] = r["o"][0, 21, 3, 77]
    _refused("one frame row taken from the next pixel", o, r, e, A.whole_l2(o, r["o"]), 2e-2, "o")
    dq = r["dq"].clone()
    dq[0, 20, 3, 77] = r["dq"][0, 21, 3, 77]
    got = dict(dq=dq, dk=r["dk"], dv=r["dv"])
    _refused("one frame row of dq taken from the next pixel", dq, r, e, _whole_dqkv(got, r), 3e-2, "dq")


def test_judge_rejects_one_dropped_element(teeth):
    _, r, e = teeth
    o = r["o"].clone()
    sl = o[1, 5, 2]
    i = int(r["o"][1, 5, 2].abs().argmax())
    sl.view(-1)[i] = 0
    v = _refused("one element dropped", o, r, e, A.whole_l2(o, r["o"]), 2e-2, "o")
    assert "element" in v.what


def test_judge_rejects_a_masked_tile_tail(teeth):
    _, r, e = teeth
    o = r["o"].clone()
    o[1, 63, 7, 112:] = 0  # the last 8 rows of the last 16-frame tile (F = 120)
    _refused("last 8 rows of the last tile zeroed", o, r, e, A.whole_l2(o, r["o"]), 2e-2, "o")


def test_judge_rejects_one_missing_diagonal_in_dtable(teeth):
    _, r, e = teeth
    F = TEETH[1]
    bm = A.bucket_map(F)
    n = 100  # offset +100 lies in the saturated bucket of +(F - 1)
    assert bm[0, n] == bm[0, F - 1]
    dt = r["dtable"].clone()
    dt[bm[0, n], 4] -= torch.diagonal(r["dbias"][4], n).sum()
    whole = A.whole_l2(dt, r["dtable"])
    v = A.judge_cols("dtable", dt.t(), r["dtable"].t(), A.BOUND_BWD[BF], e["dtable"].t(), BF)
    print(f"attn_teeth one diagonal missing in a saturated bucket: whole-tensor L2 {whole:.3g} (old gate 0.03), judge {v}")
    assert whole < 3e-2 and not v.ok


def test_judge_rejects_an_lse_offset(teeth):
    _, r, e = teeth
    lse = r["lse"].clone()
    lse[1, 9, 0, 119] += 0.1
    v = A.judge_core("teeth", dict(lse=lse), r, e, BF, 1, names=("lse",))[0]
    print(f"attn_teeth lse of one row off by 0.1: judge {v}")
    assert not v.ok


def test_judge_rejects_nan_and_a_changed_zero(teeth):
    _, r, e = teeth
    o = r["o"].clone()
    o[0, 0, 0, 0, 0] = float("nan")
    assert not A.judge_core("nan", dict(o=o), r, e, BF, 1, names=("o",))[0].ok
    one = A.tcore_inputs((2, 1, 5), BF)
    r1 = A.tcore_ref(one)
    assert r1["dq"].abs().max() == 0 and r1["dk"].abs().max() == 0 and r1["dbias"].abs().max() == 0
    dq = r1["dq"].clone()
    assert A.judge_core("zero", dict(dq=dq), r1, r1, BF, 16, names=("dq",))[0].ok
    dq[1, 2, 3, 0, 4] = 1e-30  # where the reference is exactly zero, only exactly zero passes
    assert not A.judge_core("zero", dict(dq=dq), r1, r1, BF, 16, names=("dq",))[0].ok
    prior = torch.rand(32, 8) + 1
    with pytest.raises(AssertionError):
        A.judge_dtable("zero", prior + 1e-6, prior, r1, r1, BF, 1)
    assert A.judge_dtable("zero", prior.clone(), prior, r1, r1, BF, 1) == []


# ------------------------------------------------------------------------------------------ conditions on the emulation
def _cond(name, emu, r, sid, n, bound, allow=None):
    """no slice's L2 tolerance above 2 x its bound, no element tolerance above 0.3, no row without a slice"""
    assert int(sid.min()) >= 0 and int(sid.max()) < n and sid.numel() == r.shape[0], name
    assert int(torch.bincount(sid, minlength=n).min()) > 0, name
    t2, te, _, _ = A.slice_tols(emu, r, sid, n, bound, allow)
    assert float(t2.max()) <= A.COND_L2 * bound, (name, "L2 tolerance", float(t2.max()))
    assert float(te.max()) <= A.COND_EL, (name, "element tolerance", float(te.max()))
    return float(t2.max()), float(te.max())


def _cond_cols(name, r, emu):
    """per-entry results: no tolerance above 0.3 of the row's rms (rows the reference leaves exactly zero are judged as
    exactly zero, without a tolerance)"""
    r = r.reshape(-1, r.shape[-1])
    live = r.abs().amax(-1) > 0
    t = A.cols_tol(r[live], emu.reshape(r.shape)[live], A.BOUND_BWD[BF])
    assert float(t.max()) <= A.COND_COLS, (name, "entry tolerance", float(t.max()))


def _cond_lse(name, e, r, g):
    rr, sid, n = A.core_slices(r["lse"], g)
    t = float(A.lse_tol(A.core_slices(e["lse"], g)[0], rr, sid, n, BF)[0].max())
    assert t <= A.COND_LSE, (name, "lse tolerance", t)
    return t


CORE_BF16 = sorted(set(A.MFMA_CASES) | {c + (32,) for c in A.VALU_CASES})


@pytest.mark.parametrize("case", CORE_BF16, ids=A.case_id)
def test_conditions_temporal_core(case):
    B, F, HW, md = case
    inp = A.tcore_inputs(case, BF)
    r, e = A.tcore_ref(inp, max_distance=md), A.tcore_ref(inp, "e16", max_distance=md)
    g = A.pixel_group(F)
    worst = [0.0, 0.0]
    for nm in ("o", "dq", "dk", "dv"):
        if F == 1 and nm in ("dq", "dk"):
            assert r[nm].abs().max() == 0  # judged as exactly zero, no tolerance
            continue
        rr, sid, n = A.core_slices(r[nm], g)
        t = _cond(f"{case} {nm}", A.core_slices(e[nm], g)[0], rr, sid, n, (A.BOUND_FWD if nm == "o" else A.BOUND_BWD)[BF])
        worst = [max(a, b) for a, b in zip(worst, t)]
    lse_tol = _cond_lse(f"{case} lse", e, r, g)
    if F > 1:
        _cond_cols(f"{case} dtable", r["dtable"].t(), e["dtable"].t())
    print(f"attn_cond core {A.case_id(case)}: worst L2 tol {worst[0]:.3g} element tol {worst[1]:.3g} lse tol {lse_tol:.3g}")


@pytest.mark.parametrize("case", A.SLA_CASES, ids=A.case_id)
def test_conditions_sla_core(case):
    inp = A.sla_inputs(case, BF)
    r, e = A.sla_eval(inp), A.sla_eval(inp, "e16")
    for nm in ("out", "dq", "dk", "dv"):
        if case[1] == 1 and nm in ("dq", "dk"):
            continue  # one position: both vanish (test_gpu_attn judges them against the size of the terms)
        rr, sid, n = A.sla_slices(r[nm])
        _cond(f"{case} {nm}", A.sla_slices(e[nm])[0], rr, sid, n, (A.BOUND_FWD if nm == "out" else A.BOUND_BWD)[BF])


@pytest.mark.parametrize("case", list(A.TBLOCK_CASES) + [A.TBLOCK_STRIDE_CASE] + A.TBLOCK_DW_CASES, ids=A.case_id)
def test_conditions_fused_block(case):
    B, F, HW, C = case
    inp = A.tblock_inputs(case)
    r = A.tblock_eval(inp)
    assert A._rms(r["branch"]) >= 0.5 * A._rms(inp["x"]) and A._rms(r["dxb"]) >= 0.5 * A._rms(inp["dy"])
    g = A.pixel_group(F)
    for fold in ((False, True) if C == 64 and F in A.TBLOCK_DW_F else (False,)):
        e = A.tblock_eval(inp, "e16", fold=fold)
        # dq / dk / dv are observable (and judged) only where tblock_bwd emits dqkv, not in the fold / dw pair
        for nm in ("o",) if fold or case in A.TBLOCK_DW_CASES else ("o", "dq", "dk", "dv"):
            if F == 1 and nm in ("dq", "dk"):
                assert r[nm].abs().max() == 0
                continue
            rr, sid, n = A.core_slices(r[nm], g)
            _cond(f"{case} {nm}", A.core_slices(e[nm], g)[0], rr, sid, n, (A.BOUND_FWD if nm == "o" else A.BOUND_BWD)[BF])
        _cond_lse(f"{case} lse", e, r, g)
        if F > 1:
            _cond_cols(f"{case} dtable", r["dtable"].t(), e["dtable"].t())
        for nm in ("dwqkv", "dwout"):
            _cond_cols(f"{case} {nm}", r[nm], e[nm])
        _cond_cols(f"{case} dgamma", r["dgamma"][None], e["dgamma"][None])
        for nm, full, res, bound in (("branch", "y", "x", A.BOUND_FWD[BF]), ("dxb", "dx", "dy", A.BOUND_BWD[BF])):
            rr, sid, n = A.block_slices(r[nm], B, F, HW, g)
            _cond(f"{case} {nm}", e[full] - inp[res].double(), rr, sid, n, bound, allow=2.0 ** -8 * r[full].abs())
