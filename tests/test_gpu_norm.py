"""The dense GroupNorm kernels (cesm_gn_stats, cesm_gn_apply, cesm_gn_bwd) and LayerNorm kernels (cesm_ln_fwd,
cesm_ln_bwd) against float64, judged per (sample, group) / per 64-voxel block and per element (tests/norm_ref.py), at
every regime of the launch plan (which case sits in which regime: tests/test_norm_host.py), in fp32 and bf16.

Every output and workspace a kernels.* wrapper allocates starts NaN-filled (the `poisoned` fixture), the buffers of
the direct calls are poisoned by hand, and destinations that accumulate hold finite non-zero values first: with the
empty-chunk, V = 1 and B = 4 cases, every partial a finalize kernel reads was written by the launch under test.

Each test prints its worst err / tol with the err and the e32 that went with it (profiles/norm_parity.txt).
"""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import norm_ref as N  # noqa: E402
from norm_ref import BF, F32  # noqa: E402
from cesm_emulator_amd import kernels as K  # noqa: E402
from cesm_emulator_amd._lib import KernelError, call  # noqa: E402
from cesm_emulator_amd.kernels import P, S  # noqa: E402

pytestmark = pytest.mark.gpu

GN_ALL = list(N.GN_CASES)
GN_BWD = [c for c in GN_ALL if c not in N.GN_FWD_ONLY]
SMALL = 1 << 20  # elements up to which a case also runs every null-pointer combination


def poison(t):
    return t.fill_(float("nan"))


@pytest.fixture(autouse=True)
def poisoned(monkeypatch):
    """every tensor a kernels.* wrapper allocates (outputs, workspaces, partials) starts as NaN"""
    def empty(shape, dtype, device):
        t = torch.empty(shape, dtype=dtype, device=device)
        return poison(t) if t.is_floating_point() else t
    monkeypatch.setattr(K, "empty", empty)


def nan(shape, dev, dtype=F32):
    return poison(torch.empty(shape, dtype=dtype, device=dev))


def garbage(shape, dev, seed):
    """finite, non-zero prior contents of a destination"""
    g = torch.Generator(device=dev).manual_seed(seed)
    return torch.rand(shape, device=dev, generator=g) * 4 + 1


# ------------------------------------------------------------------------------------------ GroupNorm
def gn_forward(inp, with_ss, with_res):
    B, rows, C, G = inp["case"]
    st = K.gn_stats(inp["y"], B, G)
    out = K.gn_apply(inp["y"], st, inp["gamma"], inp["beta"], inp["ss"] if with_ss else None,
                     inp["res"] if with_res else None, B, G)
    return st, out


def gn_bwd_raw(inp, st, with_ss, dss, dgamma, dbeta, dbias, accumulate):
    """cesm_gn_bwd itself (the wrapper always accumulates and always passes dgamma / dbeta): poisoned dy and workspace"""
    B, rows, C, G = inp["case"]
    y = inp["y"]
    dy = nan(y.shape, y.device, y.dtype)
    ws = nan((max(B * 1024, 1024) * C * 3 + B * C * 3 + B * C * 5,), y.device)
    call("cesm_gn_bwd", K.dtcode(y), P(inp["dout"]), P(y), P(st), P(inp["gamma"]), P(inp["beta"]),
         P(inp["ss"] if with_ss else None), P(dy), P(dss), P(dgamma), P(dbeta), P(dbias), P(ws), B, rows, C, G,
         int(accumulate), S())
    return dy


def judge_gn_fwd(tag, inp, st, out, r, r32):
    G, dt = inp["case"][3], inp["dt"]
    kk, sid, n = N.gn_slices(out, G)
    return [N.judge_stats(f"{tag} stats", st[..., 0], st[..., 1], r, r32=r32),
            N.judge_act(f"{tag} out", kk, N.gn_slices(r["out"], G)[0], sid, n, N.tol_gn_fwd(dt),
                        None if r32 is None else N.gn_slices(r32["out"], G)[0])]


def judge_gn_bwd(tag, inp, dy, dss, dgamma, dbeta, dbias, r, r32):
    B, rows, C, G = inp["case"]
    tol = N.tol_gn_bwd(inp["dt"])
    kk, sid, n = N.gn_slices(dy, G)
    v = [N.judge_act(f"{tag} dy", kk, N.gn_slices(r["dy"], G)[0], sid, n, tol,
                     None if r32 is None else N.gn_slices(r32["dy"], G)[0])]
    got = dict(dgamma=dgamma, dbeta=dbeta, dbias=dbias)
    if dss is not None:
        got.update(dscale=dss[:, :C], dshift=dss[:, C:])
    for name, k in got.items():
        if k is not None:
            v.append(N.judge_chan(f"{tag} {name}", k, r[name], tol, None if r32 is None else r32[name]))
    return v


def fp32_eval(inp, **kw):
    """PyTorch's float32 evaluation, for e32: fp32 mode only (the bf16 bounds stand as they are)"""
    return N.gn_torch(inp, torch.float32, **kw) if inp["dt"] == F32 else None


@pytest.mark.parametrize("dt", N.DTYPES, ids=N.dt_id)
@pytest.mark.parametrize("case", GN_ALL, ids=N.case_id)
def test_gn_forward(dev, case, dt):
    """gn_stats -> gn_apply with and without scale/shift, with and without the residual"""
    inp = N.gn_inputs(case, dt, dev)
    v = []
    for with_ss in (True, False):
        for with_res in (True, False):
            st, out = gn_forward(inp, with_ss, with_res)
            kw = dict(with_ss=with_ss, with_res=with_res, backward=False)
            v += judge_gn_fwd(f"ss={int(with_ss)} res={int(with_res)}", inp, st, out, N.gn_ref(inp, **kw),
                              fp32_eval(inp, **kw))
    N.report(f"gn_forward[{N.case_id(case)}-{N.dt_id(dt)}]", v)


def run_gn_backward(tag, inp, every_null):
    B, rows, C, G = inp["case"]
    dev = inp["y"].device
    st = K.gn_stats(inp["y"], B, G)
    r, r32 = N.gn_ref(inp), fp32_eval(inp)
    v = judge_gn_fwd("fwd", inp, st, K.gn_apply(inp["y"], st, inp["gamma"], inp["beta"], inp["ss"], inp["res"], B, G),
                     r, r32)
    # overwrite: prior contents of every destination are finite garbage, and must not show
    dss, dg, db, dbi = (garbage(s, dev, i) for i, s in enumerate(((B, 2 * C), (C,), (C,), (C,))))
    dy = gn_bwd_raw(inp, st, True, dss, dg, db, dbi, 0)
    v += judge_gn_bwd("overwrite", inp, dy, dss, dg, db, dbi, r, r32)
    # accumulate into zeros == overwrite; accumulate into prior contents == prior + overwrite (one fp32 add each)
    z = [torch.zeros(C, device=dev) for _ in range(3)]
    dss1 = nan((B, 2 * C), dev)
    dy1 = gn_bwd_raw(inp, st, True, dss1, *z, 1)
    assert torch.equal(dy1, dy) and torch.equal(dss1, dss)
    assert all(torch.equal(a, b) for a, b in zip(z, (dg, db, dbi)))
    prior = [garbage((C,), dev, 10 + i) for i in range(3)]
    acc = [p.clone() for p in prior]
    gn_bwd_raw(inp, st, True, None, *acc, 1)
    assert all(torch.equal(a, p + o) for a, p, o in zip(acc, prior, (dg, db, dbi)))
    # nothing but dy, no scale/shift: its own reference
    dy0 = gn_bwd_raw(inp, st, False, None, None, None, None, 0)
    v += judge_gn_bwd("all null", inp, dy0, None, None, None, None, N.gn_ref(inp, with_ss=False),
                      fp32_eval(inp, with_ss=False))
    if every_null:  # each destination null in turn: the others are what they were
        full = (dss, dg, db, dbi)
        for i in range(4):
            outs = [None if j == i else nan(full[j].shape, dev) for j in range(4)]
            assert torch.equal(gn_bwd_raw(inp, st, True, *outs, 0), dy)
            assert all(o is None or torch.equal(o, f) for o, f in zip(outs, full)), i
    torch.cuda.synchronize()
    N.report(tag, v)


@pytest.mark.parametrize("dt", N.DTYPES, ids=N.dt_id)
@pytest.mark.parametrize("case", GN_BWD, ids=N.case_id)
def test_gn_backward(dev, case, dt):
    """cesm_gn_bwd on the stored y with gn_stats' statistics: overwrite and accumulate, destinations present or null"""
    inp = N.gn_inputs(case, dt, dev)
    run_gn_backward(f"gn_backward[{N.case_id(case)}-{N.dt_id(dt)}]", inp, inp["y"].numel() <= SMALL)


@pytest.mark.parametrize("dt", N.DTYPES, ids=N.dt_id)
@pytest.mark.parametrize("m", N.OFFSETS)
@pytest.mark.parametrize("case", N.GN_OFFSET_CASES, ids=N.case_id)
def test_gn_offset(dev, case, m, dt):
    """group means at +- m * std (sign alternating across groups), non-zero beta and shift: the one-pass variance
    E[y^2] - mean^2 and the backward's S3 - mean * S1 cancel here.

    With fp32 per-thread sums alone the fp32 statistics missed this at m = 32 (err / tol 6.45, 2.58, 7.11 for the three
    cases: rstd off by up to 4.7e-5); gn_stats_kernel's fp32 instantiation now takes double sums for a group that
    far off zero (csrc/gn.hip, GN_OFFSET_STD)."""
    inp = N.gn_inputs(case, dt, dev, m=m)
    run_gn_backward(f"gn_offset[{N.case_id(case)}-m{m}-{N.dt_id(dt)}]", inp, False)


@pytest.mark.parametrize("dt", N.DTYPES, ids=N.dt_id)
def test_gn_silu_range(dev, dt):
    """pre-activations out to about +- 90 in three channels: exp overflows to inf inside the bf16 path's sigmoid;
    outputs and gradients stay finite and inside the bounds"""
    inp = N.gn_inputs(N.GN_SILU_CASE, dt, dev, silu_range=True)
    B, rows, C, G = inp["case"]
    r = N.gn_ref(inp, with_ss=False, with_res=False, backward=False)
    yg = inp["y"].double().view(B, rows, G, C // G)
    xhat = ((yg - r["mean"].view(B, 1, G, 1)) * r["rstd"].view(B, 1, G, 1)).view(B, rows, C)
    a = xhat * inp["gamma"].double() + inp["beta"].double()  # the pre-activation before scale / shift
    assert a.max() > 85 and a.min() < -85, (a.min().item(), a.max().item())
    run_gn_backward(f"gn_silu_range[{N.dt_id(dt)}]", inp, False)


@pytest.mark.parametrize("dt", N.DTYPES, ids=N.dt_id)
def test_gn_width_guards(dev, dt):
    """cesm_gn_bwd refuses the widths its reduction cannot add (C / 8 not a power of two: the xor shuffles would sum the
    wrong lanes, in bounds and silently), and both directions refuse groups narrower than a thread's 8 channels"""
    for case in N.GN_BWD_REFUSED:
        B, rows, C, G = case
        inp = N.gn_inputs(case, dt, dev)
        st = torch.zeros(B, G, 2, device=dev)
        dg, db = torch.zeros(C, device=dev), torch.zeros(C, device=dev)
        with pytest.raises(KernelError):
            K.gn_bwd(inp["dout"], inp["y"], st, inp["gamma"], inp["beta"], inp["ss"], dg, db, B, G, True)
        assert not dg.any() and not db.any()
    inp = N.gn_inputs((2, 300, 32, 8), dt, dev)
    with pytest.raises(KernelError):
        K.gn_apply(inp["y"], torch.zeros(2, 8, 2, device=dev), inp["gamma"], inp["beta"], None, None, 2, 8)
    with pytest.raises(KernelError):
        K.gn_stats(inp["y"], 2, 8)
    # the forward of the refused C = 192 is right (test_gn_forward's (1, 300, 192, 8)), at G = 24 too
    inp = N.gn_inputs((1, 300, 192, 24), dt, dev)
    st, out = gn_forward(inp, True, True)
    kw = dict(backward=False)
    N.report(f"gn_width_guards[192/24 forward-{N.dt_id(dt)}]",
             judge_gn_fwd("fwd", inp, st, out, N.gn_ref(inp, **kw), fp32_eval(inp, **kw)))


@pytest.mark.parametrize("m", N.OFFSETS)
def test_gn_epilogue_stats_offset(dev, m):
    """The conv epilogue's statistics partials (cesm_conv_fwd_gn -> cesm_gn_stats_part, bf16, 64 -> 64 at 20 x 96) with
    a conv bias that puts the group means at about +- m * std: (mean, rstd) against float64 statistics of the stored
    bf16 y (not against gn_stats)."""
    B, Fr, H, W, C, G = 2, 3, 20, 96, 64, 8
    Nb = B * Fr
    g = torch.Generator(device=dev).manual_seed(64 + H + W)
    x = (torch.randn(Nb, H, W, C, device=dev, generator=g) + 0.3).to(BF)
    w = torch.randn(C, C, 1, 3, 3, device=dev, generator=g) * C ** -0.5 / 3
    bias0 = torch.randn(C, device=dev, generator=g) * 0.5
    wp = K.conv_pack(w, BF, C, C, 3, 3, 0, 0)
    geom = (H, W, C, 3, 3, 1, 1, 1)
    nslot = K.conv_gn_nslot(x, None, geom, B)
    assert nslot > 0
    y0 = K.conv_fwd(x, None, wp, bias0, geom).double().view(-1, G, C // G)
    std = (y0 - y0.mean((0, 2), keepdim=True)).square().mean((0, 2)).sqrt()  # per group, the bias spread included
    sign = 1.0 - 2.0 * (torch.arange(G, device=dev) % 2)
    bias = bias0 + (sign * m * std).float().repeat_interleave(C // G)
    y, part = K.conv_fwd_gn(x, None, wp, bias, geom, B, nslot)
    rows_b = y.numel() // (C * B)
    st = K.gn_stats_part(part, rows_b, G)
    inp = dict(case=(B, rows_b, C, G), y=y.view(B, rows_b, C), gamma=torch.ones(C, device=dev),
               beta=torch.zeros(C, device=dev), dt=BF)
    kw = dict(with_ss=False, with_res=False, backward=False)
    r, r32 = N.gn_ref(inp, **kw), N.gn_torch(inp, torch.float32, **kw)
    ratio = r["mean"].abs() * r["rstd"]
    assert (ratio > 0.75 * m).all() and (ratio < 1.3 * m).all(), ratio
    N.report(f"gn_epilogue_stats_offset[m{m}]", [N.judge_stats("stats_part", st[..., 0], st[..., 1], r, r32=r32)])


# ------------------------------------------------------------------------------------------ LayerNorm
def ln_bwd_raw(inp, mr, with_dres, dgamma, accumulate):
    V, C, perm = inp["case"]
    x = inp["x"]
    dx = nan(x.shape, x.device, x.dtype)
    nblk = 1024
    part = nan((nblk, C), x.device)
    pf, phw = perm if perm else (0, 0)
    call("cesm_ln_bwd", K.dtcode(x), P(inp["dy"]), P(x), P(mr), P(inp["gamma"]), P(inp["dres"] if with_dres else None),
         P(dx), P(dgamma), P(part), nblk, V, C, int(accumulate), pf, phw, S())
    return dx


def run_ln(tag, inp):
    V, C, perm = inp["case"]
    dt, dev = inp["dt"], inp["x"].device
    r = N.ln_ref(inp)
    r32 = N.ln_torch(inp, torch.float32) if dt == F32 else None
    out, mr = K.ln_fwd(inp["x"], inp["gamma"], perm=perm)
    assert torch.equal(K.ln_fwd(inp["x"], inp["gamma"], save=False, perm=perm)[0], out)  # mr null: the same rows
    so, n = N.ln_slice_ids(V, perm, True, dev)
    sx, _ = N.ln_slice_ids(V, perm, False, dev)
    pick = (lambda name: None) if r32 is None else (lambda name: r32[name])
    v = [N.judge_act("out", out, r["out"], so, n, N.tol_ln_fwd(dt), pick("out")),
         N.judge_stats("mr", mr[:, 0], mr[:, 1], r, r32=r32)]
    if perm:  # voxel (b, f, p) is output row (b, p, f): a spot check that does not go through perm_rows
        f_, hw = perm
        b, f, p = 1, f_ - 2, hw - 1
        x1 = inp["x"][(b * f_ + f) * hw + p].double()
        want = (x1 - x1.mean()) / torch.sqrt(x1.var(unbiased=False) + N.EPS) * inp["gamma"].double()
        assert torch.allclose(out[(b * hw + p) * f_ + f].double(), want, rtol=4 * N.tol_ln_fwd(dt), atol=1e-4)
    tol = N.tol_ln_bwd(dt)
    dg = garbage((C,), dev, 5)
    dx = ln_bwd_raw(inp, mr, True, dg, 0)  # overwrite over garbage
    v += [N.judge_act("dx", dx, r["dx"], sx, n, tol, pick("dx")), N.judge_chan("dgamma", dg, r["dgamma"], tol,
                                                                               pick("dgamma"))]
    prior = garbage((C,), dev, 6)
    acc = prior.clone()
    assert torch.equal(K.ln_bwd(inp["dy"], inp["x"], mr, inp["gamma"], acc, dres=inp["dres"], perm=perm), dx)
    assert torch.equal(acc, prior + dg)
    dx0 = ln_bwd_raw(inp, mr, False, None, 0)  # no dres, no dgamma
    v.append(N.judge_act("dx (no dres)", dx0, N.ln_ref(inp, with_dres=False)["dx"], sx, n, tol,
                         None if r32 is None else N.ln_torch(inp, torch.float32, with_dres=False)["dx"]))
    torch.cuda.synchronize()
    N.report(tag, v)


@pytest.mark.parametrize("dt", N.DTYPES, ids=N.dt_id)
@pytest.mark.parametrize("case", N.LN_CASES, ids=N.case_id)
def test_ln(dev, case, dt):
    run_ln(f"ln[{N.case_id(case)}-{N.dt_id(dt)}]", N.ln_inputs(case, dt, dev))


@pytest.mark.parametrize("dt", N.DTYPES, ids=N.dt_id)
@pytest.mark.parametrize("m", N.OFFSETS)
@pytest.mark.parametrize("case", N.LN_OFFSET_CASES, ids=N.case_id)
def test_ln_offset(dev, case, m, dt):
    """every voxel's mean at +- m * std"""
    run_ln(f"ln_offset[{N.case_id(case)}-m{m}-{N.dt_id(dt)}]", N.ln_inputs(case, dt, dev, m=m))
