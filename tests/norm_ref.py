"""Float64 references, case tables and the judging rule for the GroupNorm and LayerNorm kernel tests
(tests/test_norm_host.py on the CPU, tests/test_gpu_norm.py on the GPU).  Nothing here calls a kernel of the project.

GroupNorm:  out = silu(GN_G(y) * (1 + scale) + shift) + res  over y [B, rows_b, C] (a sample's voxels are a
contiguous [rows_b, C] block), statistics per (sample, group), gradients dy, dss = (d scale | d shift), dgamma, dbeta
and dbias = sum of dy over samples and rows (the producing conv's bias gradient).
LayerNorm:  out = (x - mean) * rstd * gamma per voxel over C, biased variance, gamma only; dx = LN backward + dres;
with perm = (F, HW) the output row (and the dy row) of voxel (b, f, p) is (b, p, f).

Every reference takes its inputs already rounded to the storage dtype and evaluates in float64, on whatever device
the inputs live on.

Tolerances (tol_*) are the bounds tests/test_gpu_kernels.py applies to whole tensors (test_block_groupnorm,
test_layernorm), here applied to every slice and every element; none is derived from a kernel's measured error.
"""
import math

import torch
import torch.nn.functional as F

EPS = 1e-5
F32, BF = torch.float32, torch.bfloat16
DTYPES = [F32, BF]
TOL = {F32: 1e-5, BF: 1e-2}
E32_MARGIN = 8.0  # fp32 mode: tol = max(bound, 8 * e32); margin for another summation order + the one-pass variance
LN_BLOCK = 64     # LayerNorm results are judged per block of 64 consecutive voxels


def tol_gn_fwd(dt):
    return TOL[dt] * (3 if dt == BF else 1)


def tol_gn_bwd(dt):
    return TOL[dt] * (5 if dt == BF else 10)


def tol_ln_fwd(dt):
    return TOL[dt]


def tol_ln_bwd(dt):
    return TOL[dt] * 2


TOL_STATS = 1e-5  # (mean, rstd) are fp32 in both modes: the bound test_gn_epilogue_stats_bf16 uses


# ---------------------------------------------------------------------------------------------- case tables
# (B, rows_b, C, G) -> the launch-plan regime the case is there for, asserted from the library's plan queries by
# tests/test_norm_host.py:  chunks = reduction chunks per sample, rpc = rows per chunk, last = state of the LAST chunk
# ("full", "ragged": fewer rows than rpc, "empty": no row at all), capped = the chunk count no longer grows with
# rows_b, short = fewer rows than a block has row lanes.
# Not covered: the streaming kernels' cap of 4096 chunks needs 67M elements per sample; it changes the trip count of
# the same row loop and nothing else.
GN_CASES = {
    (2, 5, 64, 8): dict(chunks=1, rpc=5, last="full", capped=False, short=True),
    (1, 1, 512, 8): dict(chunks=1, rpc=1, last="full", capped=False, short=True),
    (3, 1000, 128, 8): dict(chunks=7, rpc=143, last="ragged", capped=False, short=False),
    (1, 76801, 64, 8): dict(chunks=300, rpc=257, last="empty", capped=False, short=False),
    (3, 16384 * 400 // 256, 256, 8): dict(chunks=1024 // 3, rpc=76, last="empty", capped=True, short=False),
    (4, 9000, 512, 8): dict(chunks=256, rpc=36, last="empty", capped=True, short=False),
    (2, 300, 1024, 16): dict(chunks=18, rpc=17, last="ragged", capped=False, short=False),  # C / 8 = 128 > 64
    (2, 300, 1024, 32): dict(chunks=18, rpc=17, last="ragged", capped=False, short=False),
    (2, 300, 64, 1): dict(chunks=1, rpc=300, last="full", capped=False, short=False),
    (2, 300, 64, 2): dict(chunks=1, rpc=300, last="full", capped=False, short=False),
    (2, 300, 32, 4): dict(chunks=1, rpc=300, last="full", capped=False, short=False),
    (2, 300, 64, 8): dict(chunks=1, rpc=300, last="full", capped=False, short=False),  # the third offset case
    (2, 288, 128, 8): dict(chunks=2, rpc=144, last="full", capped=False, short=False),  # test_block_groupnorm's
    (2, 288, 512, 8): dict(chunks=9, rpc=32, last="full", capped=False, short=False),
    (1, 300, 192, 8): dict(chunks=3, rpc=100, last="full", capped=False, short=False),  # forward only: C / 8 = 24
}
GN_FWD_ONLY = {(1, 300, 192, 8)}
GN_BWD_REFUSED = [(1, 300, 192, 24), (2, 300, 32, 8)]  # C / 8 not a power of two; 4 channels per group
GN_OFFSET_CASES = [(3, 1000, 128, 8), (2, 288, 512, 8), (2, 300, 64, 8)]
OFFSETS = [4, 32]  # group mean = +- m * std; m = 256 is out of scope (GroupNorm)
GN_SILU_CASE = (2, 288, 128, 8)

# (V, C, perm)
LN_CASES = [(V, C, None) for V in (1, 31, 1000, 4097) for C in (64, 128, 256, 512)]
LN_CASES += [(2 * f * hw, C, (f, hw)) for (f, hw) in ((5, 7), (17, 40), (120, 3)) for C in (64, 256)]
LN_CASES += [(1000, 8, None)]  # one lane per voxel
LN_OFFSET_CASES = [(1000, 64, None), (1000, 512, None)]


def case_id(c):
    return "-".join("x".join(map(str, v)) if isinstance(v, tuple) else str(v) for v in c)


def dt_id(dt):
    return "fp32" if dt == F32 else "bf16"


# ---------------------------------------------------------------------------------------------- inputs
def _gen(device, seed):
    return torch.Generator(device=device).manual_seed(seed)


def _r(t, dt):
    """round to the storage dtype"""
    return t.to(dt)


def gn_inputs(case, dt, device="cpu", m=0, silu_range=False, seed=0):
    """Inputs of one GroupNorm case in the storage dtype (y, res, dout) and fp32 (gamma, beta, ss).  m: every
    (sample, group) gets the offset +- m * std, sign alternating across groups; silu_range: three channels' gamma is
    +- 36, so that their pre-activation reaches about +- 90 at |xhat| = 2.5."""
    B, rows, C, G = case
    g = _gen(device, 1000 + seed)
    kw = dict(device=device, generator=g)
    std = torch.rand(B, 1, G, 1, **kw) + 0.5
    y = torch.randn(B, rows, G, C // G, **kw) * std
    if m:
        sign = 1.0 - 2.0 * (torch.arange(G, device=device) % 2).view(1, 1, G, 1)
        y = y + sign * m * std
    d = dict(case=case, dt=dt, m=m)
    d["y"] = _r(y.view(B, rows, C), dt).contiguous()
    d["res"] = _r(torch.randn(B, rows, C, **kw), dt)
    d["dout"] = _r(torch.randn(B, rows, C, **kw), dt)
    d["gamma"] = torch.rand(C, **kw) + 0.5
    d["beta"] = torch.rand(C, **kw) - 0.5
    if silu_range:
        for i, c in enumerate((3, C // 2 + 5, C - 2)):
            d["gamma"][c] = 36.0 * (-1) ** i
    d["ss"] = torch.randn(B, 2 * C, **kw) * 0.3
    return d


def ln_inputs(case, dt, device="cpu", m=0, seed=0):
    V, C, perm = case
    g = _gen(device, 2000 + seed)
    kw = dict(device=device, generator=g)
    std = torch.rand(V, 1, **kw) * 2 + 0.5
    x = torch.randn(V, C, **kw) * std + 0.5
    if m:
        x = x + (1.0 - 2.0 * (torch.arange(V, device=device) % 2).view(V, 1)) * m * std
    d = dict(case=case, dt=dt, m=m)
    d["x"] = _r(x, dt).contiguous()
    d["gamma"] = torch.rand(C, **kw) + 0.5
    d["dy"] = _r(torch.randn(V, C, **kw), dt)  # in the output's row order
    d["dres"] = _r(torch.randn(V, C, **kw), dt)
    return d


def perm_rows(V, perm, device="cpu"):
    """output row of every voxel: voxel (b, f, p) of [B][F][HW] -> row (b * HW + p) * F + f; identity without perm"""
    v = torch.arange(V, device=device)
    if not perm:
        return v
    f_, hw = perm
    b, r = v // (f_ * hw), v % (f_ * hw)
    return (b * hw + r % hw) * f_ + r // hw


# ---------------------------------------------------------------------------------------------- references
def gn_ref(inp, with_ss=True, with_res=True, backward=True):
    """float64 closed form; returns a dict of out, mean, rstd [B, G] and, with backward, dy, dscale, dshift [B, C],
    dgamma, dbeta, dbias [C]"""
    B, rows, C, G = inp["case"]
    cg = C // G
    y = inp["y"].double()
    gam, bet = inp["gamma"].double(), inp["beta"].double()
    yg = y.view(B, rows, G, cg)
    mean = yg.mean((1, 3))
    var = (yg - mean.view(B, 1, G, 1)).square().mean((1, 3))
    rstd = 1.0 / torch.sqrt(var + EPS)
    xhat = ((yg - mean.view(B, 1, G, 1)) * rstd.view(B, 1, G, 1)).view(B, rows, C)
    if with_ss:
        ss = inp["ss"].double()
        sc, sh = (1.0 + ss[:, :C]).view(B, 1, C), ss[:, C:].view(B, 1, C)
    else:
        sc = torch.ones(B, 1, C, dtype=torch.float64, device=y.device)
        sh = torch.zeros_like(sc)
    a = (xhat * gam + bet) * sc + sh
    sig = torch.sigmoid(a)
    out = a * sig
    if with_res:
        out = out + inp["res"].double()
    r = dict(out=out, mean=mean, rstd=rstd)
    if not backward:
        return r
    da = inp["dout"].double() * (sig * (1.0 + a * (1.0 - sig)))
    del sig, a, out
    s1 = da.sum(1)
    s2 = (da * xhat).sum(1)
    r["dscale"] = gam * s2 + bet * s1
    r["dshift"] = s1
    r["dgamma"] = (sc.view(B, C) * s2).sum(0)
    r["dbeta"] = (sc.view(B, C) * s1).sum(0)
    dxh = (da * (sc * gam)).view(B, rows, G, cg)
    del da
    xg = xhat.view(B, rows, G, cg)
    m1 = dxh.mean((1, 3)).view(B, 1, G, 1)
    m2 = (dxh * xg).mean((1, 3)).view(B, 1, G, 1)
    dy = (rstd.view(B, 1, G, 1) * (dxh - m1 - xg * m2)).view(B, rows, C)
    r["dy"] = dy
    r["dbias"] = dy.sum((0, 1))
    return r


def gn_torch(inp, dtype, with_ss=True, with_res=True, backward=True):
    """the same formula with PyTorch ops (native_group_norm, F.silu, autograd) in `dtype`: float32 gives e32, the
    error PyTorch's own fp32 evaluation leaves against float64; float64 cross-checks gn_ref"""
    B, rows, C, G = inp["case"]
    y = inp["y"].to(dtype).requires_grad_(backward)
    gam = inp["gamma"].to(dtype).requires_grad_(backward)
    bet = inp["beta"].to(dtype).requires_grad_(backward)
    ss = inp["ss"].to(dtype).requires_grad_(backward) if with_ss else None
    h, mean, rstd = torch.native_group_norm(y.permute(0, 2, 1).contiguous(), gam, bet, B, C, rows, G, EPS)
    h = h.permute(0, 2, 1)
    if with_ss:
        h = h * (ss[:, None, :C] + 1) + ss[:, None, C:]
    out = F.silu(h)
    if with_res:
        out = out + inp["res"].to(dtype)
    r = dict(out=out.detach(), mean=mean.detach().view(B, G), rstd=rstd.detach().view(B, G))
    if not backward:
        return r
    out.backward(inp["dout"].to(dtype))
    r["dy"] = y.grad
    r["dgamma"], r["dbeta"] = gam.grad, bet.grad
    r["dbias"] = y.grad.sum((0, 1))
    if with_ss:
        r["dscale"], r["dshift"] = ss.grad[:, :C], ss.grad[:, C:]
    return r


def ln_ref(inp, with_dres=True):
    """float64 closed form: out (rows permuted with perm), mean, rstd [V] (x's order), dx, dgamma"""
    V, C, perm = inp["case"]
    x, gam = inp["x"].double(), inp["gamma"].double()
    idx = perm_rows(V, perm, x.device)
    mean = x.mean(-1, keepdim=True)
    var = (x - mean).square().mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + EPS)
    xhat = (x - mean) * rstd
    out = torch.empty_like(x)
    out[idx] = xhat * gam
    dyx = inp["dy"].double()[idx]  # dy of voxel v lives at its output row
    g = dyx * gam
    dx = rstd * (g - g.mean(-1, keepdim=True) - xhat * (g * xhat).mean(-1, keepdim=True))
    if with_dres:
        dx = dx + inp["dres"].double()
    return dict(out=out, mean=mean[:, 0], rstd=rstd[:, 0], dx=dx, dgamma=(dyx * xhat).sum(0))


def ln_torch(inp, dtype, with_dres=True):
    V, C, perm = inp["case"]
    x = inp["x"].to(dtype).requires_grad_(True)
    gam = inp["gamma"].to(dtype).requires_grad_(True)
    idx = perm_rows(V, perm, x.device)
    o, mean, rstd = torch.native_layer_norm(x, (C,), gam, None, EPS)
    o.backward(inp["dy"].to(dtype)[idx])
    out = torch.empty_like(o)
    out[idx] = o.detach()
    dx = x.grad + inp["dres"].to(dtype) if with_dres else x.grad
    return dict(out=out, mean=mean.detach().view(V), rstd=rstd.detach().view(V), dx=dx, dgamma=gam.grad)


# ---------------------------------------------------------------------------------------------- slices
def gn_slices(t, G):
    """[B, rows, C] -> ([B * G, rows * C / G]: one (sample, group) per row, None, slice count) for judge_act"""
    B, rows, C = t.shape
    return t.reshape(B, rows, G, C // G).permute(0, 2, 1, 3).reshape(B * G, rows * (C // G)), None, B * G


def ln_slice_ids(V, perm, output_order, device="cpu"):
    """slice of every row of a [V, C] LayerNorm tensor: blocks of 64 consecutive voxels; with perm, blocks of whole
    pixels (a pixel's F frames stay in one slice, max(1, 64 // F) pixels per slice).  output_order: the tensor's rows
    are the permuted output rows (out), not x's (dx)."""
    v = torch.arange(V, device=device)
    if not perm:
        sid = v // LN_BLOCK
    else:
        f_, hw = perm
        pix = v // f_ if output_order else (v // (f_ * hw)) * hw + v % hw
        sid = pix // max(1, LN_BLOCK // f_)
    return sid, int(sid.max().item()) + 1


# ---------------------------------------------------------------------------------------------- judging
class Verdict:
    """worst figures of one judged result: ratio = err / tol (passes iff <= 1), err and the e32 that went with it
    (ename: what the reference's own error is called in print; tests/attn_ref.py's bf16 mode sets e16)"""
    ename = "e32"

    def __init__(self, name, ratio, err, e32, what):
        self.name, self.what = name, what
        self.ratio, self.err, self.e32 = (float(torch.as_tensor(x).detach()) for x in (ratio, err, e32))

    @property
    def ok(self):
        return self.ratio <= 1.0 and math.isfinite(self.ratio)

    def __str__(self):
        return f"{self.name}: err/tol {self.ratio:.3g} err {self.err:.3g} {self.ename} {self.e32:.3g} ({self.what})"


def _scatter(vals, sid, n, reduce):
    out = torch.zeros(n, dtype=torch.float64, device=vals.device)
    return out.index_add_(0, sid, vals) if reduce == "sum" else out.scatter_reduce_(0, sid, vals, "amax")


def _slice_err(k, r, sid, n):
    """per slice: relative L2 error and the per-element figure max |k - r| / (|r| + rms(slice)); a non-finite k gives
    inf.  sid: the slice of every row of k / r [rows, width]; None: every row is one slice."""
    r = r.double()
    d = k.double() - r
    d = torch.where(torch.isfinite(d), d, torch.full_like(d, float("inf")))
    if sid is None:
        r2, e2 = r.square().sum(-1), d.square().sum(-1)
        rms = torch.sqrt(r2 / r.shape[1])
        el = (d.abs() / (r.abs() + rms[:, None]).clamp_min(1e-300)).amax(-1)
    else:
        cnt = _scatter(torch.full((r.shape[0],), float(r.shape[1]), dtype=torch.float64, device=r.device), sid, n, "sum")
        r2 = _scatter(r.square().sum(-1), sid, n, "sum")
        e2 = _scatter(d.square().sum(-1), sid, n, "sum")
        rms = torch.sqrt(r2 / cnt.clamp_min(1))
        el = _scatter((d.abs() / (r.abs() + rms[sid][:, None]).clamp_min(1e-300)).amax(-1), sid, n, "amax")
    return torch.sqrt(e2) / torch.sqrt(r2).clamp_min(1e-300), el


def judge_act(name, k, r, sid, n, tol, r32=None):
    """Activation-shaped result k against the float64 r, both [rows, width] with the slice id of every row (sid None:
    every row is a slice of its own).  Two rules,
    each with the slice's own tol: relative L2 of the slice, and per element |k - r| <= tol * (|r| + rms(slice)).
    r32 (fp32 mode): PyTorch's float32 evaluation; tol = max(tol, 8 * e32) with e32 its relative L2 in the same slice."""
    l2, el = _slice_err(k, r, sid, n)
    e32 = _slice_err(r32, r, sid, n)[0] if r32 is not None else torch.zeros_like(l2)
    t = torch.maximum(torch.full_like(l2, tol), E32_MARGIN * e32)
    ratios = torch.stack((l2 / t, el / t))
    ratios = torch.where(torch.isnan(ratios), torch.full_like(ratios, float("inf")), ratios)
    w = int(ratios.argmax().item())
    rule, s = divmod(w, n)
    return Verdict(name, ratios[rule, s], (l2, el)[rule][s], e32[s], f"{'L2' if rule == 0 else 'element'} of slice {s}")


def judge_chan(name, k, r, tol, r32=None):
    """Per-channel result (a vector, or [B, C] judged row by row): |k_c - r_c| <= tol * rms(r) for every channel.
    r32: tol = max(tol, 8 * e32), e32 = the float32 evaluation's worst channel by the same measure."""
    r = r.double().reshape(-1, r.shape[-1])
    rms = r.square().mean(-1, keepdim=True).sqrt().clamp_min(1e-300)

    def err(x):
        e = (x.double().reshape(r.shape) - r).abs() / rms
        return torch.where(torch.isfinite(e), e, torch.full_like(e, float("inf"))).amax(-1)
    e = err(k)
    e32 = err(r32) if r32 is not None else torch.zeros_like(e)
    ratio = e / torch.maximum(torch.full_like(e, tol), E32_MARGIN * e32)
    s = int(ratio.argmax().item())
    return Verdict(name, ratio[s], e[s], e32[s], f"row {s}")


def judge_stats(name, mean, rstd, r, tol=TOL_STATS, r32=None):
    """(mean, rstd) per slice: |d mean| * rstd and |d rstd| / rstd against float64, each <= tol (fp32 mode:
    max(tol, 8 * e32) with PyTorch's float32 statistics)"""
    rm, rr = r["mean"].double().reshape(-1), r["rstd"].double().reshape(-1)

    def err(m_, s_):
        e = torch.stack(((m_.double().reshape(-1) - rm).abs() * rr, (s_.double().reshape(-1) - rr).abs() / rr))
        return torch.where(torch.isfinite(e), e, torch.full_like(e, float("inf")))
    e = err(mean, rstd)
    e32 = err(r32["mean"], r32["rstd"]).amax(0) if r32 is not None else torch.zeros_like(rm)
    ratio = e / torch.maximum(torch.full_like(e32, tol), E32_MARGIN * e32)
    w = int(ratio.argmax().item())
    q, s = divmod(w, rm.numel())
    return Verdict(name, ratio[q, s], e[q, s], e32[s], f"{'mean' if q == 0 else 'rstd'} of slice {s}")


def whole_l2(k, r):
    """the whole-tensor figure the older tests use (for the tests of judge's teeth)"""
    r = r.double()
    return (torch.linalg.vector_norm(k.double() - r) / torch.linalg.vector_norm(r).clamp_min(1e-30)).item()


def report(tag, verdicts, prefix="norm_parity"):
    """print every verdict and the worst on one line (the GPU run's lines are kept in profiles/norm_parity.txt;
    tests/attn_ref.py prints with the prefix attn_parity), then assert them all"""
    worst = max(verdicts, key=lambda v: v.ratio if math.isfinite(v.ratio) else float("inf"))
    print(f"{prefix} {tag}: worst err/tol {worst.ratio:.3g} err {worst.err:.3g} {worst.ename} {worst.e32:.3g} "
          f"[{worst.name}, {worst.what}]")
    bad = [str(v) for v in verdicts if not v.ok]
    assert not bad, f"{tag}: " + "; ".join(bad)
