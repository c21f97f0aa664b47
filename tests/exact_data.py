"""Exact integer data for the linear kernels (convs, GEMMs, reductions): inputs, preconditions, comparison, sweeps.

The kernels under test are linear.  With small integer-valued operands every bf16 x bf16 product is exact in fp32, every
partial sum is an integer far below 2^24 (so fp32 accumulation is exact in any order, split or MFMA grouping), and with
magnitudes at or below 256 every bf16-stored result is exactly representable.  The kernel must then equal a float64
reference bit for bit; one dropped, duplicated or mis-indexed term anywhere is a mismatch.

This is a plain module (no fixtures): tests/test_exact_host.py freezes the input regime and the kernel coverage of the
sweeps on the CPU, tests/test_gpu_exact.py runs the sweeps on the GPU.
"""
import itertools
import zlib

import torch
import torch.nn.functional as F

BF, F32 = torch.bfloat16, torch.float32
BF16_EXACT = 256          # every integer of magnitude <= 256 is a bf16 value (8 significand bits)
ACC_BOUND = 1 << 22       # sum |a||b| per fp32 accumulation: two bits under the 24-bit significand
FP32_INT = 1 << 24


# ------------------------------------------------------------------------------------------ generators
def ints(shape, amax, e2, gen):
    """uniform integers in [-amax, amax], thinned to zero with the probability that makes E[v^2] = e2; float64, CPU"""
    full = amax * (amax + 1) / 3.0          # E[u^2] of the uniform integer on [-amax, amax]
    keep = e2 / full
    assert 0.0 < keep <= 1.0 + 1e-12, (amax, e2)
    v = torch.randint(-amax, amax + 1, tuple(shape), generator=gen, dtype=torch.int64).double()
    if keep < 1.0:
        v = v * (torch.rand(tuple(shape), generator=gen, dtype=torch.float64) < keep)
    return v


X_AMAX, X_E2 = 2, 2.0     # activations and output gradients: {-2..2}, E[x^2] = 2
TERNARY_E2 = 2.0 / 3.0    # unthinned ternary weight


def weight_e2(K, target=1024.0, other_e2=X_E2):
    """E[w^2] of the ternary weight of a K-term contraction against operands of E[x^2] = other_e2, so that
    K E[x^2] E[w^2] <= target: the result's standard deviation is at most sqrt(target) (32 by default)"""
    return min(TERNARY_E2, target / (other_e2 * K))


def gen_for(*key):
    """a CPU generator seeded from the case's own parameters: the same data in every process (no use of hash(), which
    Python salts per process for strings), so a mismatch seen on one machine is regenerated on any other"""
    return torch.Generator().manual_seed(seed_for(*key))


def seed_for(*key):
    return zlib.crc32(repr(key).encode())


# ------------------------------------------------------------------------------------------ preconditions
def _amax(t):
    return float(t.abs().max()) if t.numel() else 0.0


def check_regime(ref, stored_bf16, abs_ref=None):
    """The preconditions of bitwise equality, asserted on the reference alone (conditions, not tolerances: if a seed
    breaks one, change the inputs).
    ref: the float64 reference tensors -- all integer-valued and below 2^24 in magnitude (exact as fp32);
    stored_bf16: every tensor the kernel stores in bf16, the value before a fused residual is added included:
    max |.| <= 256;
    abs_ref: sum |a||b| of every fp32 accumulation (the same op on |a|, |b|), as tensors or as scalar upper bounds such
    as K max|a| max|b|: each below 2^22."""
    for t in ref:
        assert torch.equal(t, t.round()), "reference is not integer-valued"
        assert _amax(t) < FP32_INT, _amax(t)
    for t in stored_bf16:
        assert torch.equal(t, t.round()), "bf16-stored reference is not integer-valued"
        assert _amax(t) <= BF16_EXACT, f"bf16-stored value of magnitude {_amax(t)} > {BF16_EXACT}"
    for a in ([] if abs_ref is None else abs_ref):
        m = _amax(a) if torch.is_tensor(a) else float(a)
        assert m < ACC_BOUND, f"sum |a||b| = {m} >= 2^22"


# ------------------------------------------------------------------------------------------ comparison
def assert_exact(got, want, name, spatial=None):
    """bitwise equality (as float64 on the CPU; NaN never equals).  The failure message localises the mismatch: count,
    bounding box per axis, the distinct values of each spatial index modulo 32 and 36 (the tile widths), and the first
    eight (index, got, want).  spatial: the spatial axes (default: 1 and 2 of a [N, H, W, C] tensor)."""
    g, w = got.detach().double().cpu(), want.detach().double().cpu()
    assert g.shape == w.shape, f"{name}: shape {tuple(g.shape)} != {tuple(w.shape)}"
    if torch.equal(g, w):
        return
    bad = (g != w) | g.isnan()
    idx = bad.nonzero()
    if spatial is None:
        spatial = (1, 2) if g.ndim == 4 else ()
    box = [(int(idx[:, a].min()), int(idx[:, a].max())) for a in range(g.ndim)]
    mods = {f"axis{a}%{m}": sorted(set((idx[:, a] % m).tolist())) for a in spatial for m in (32, 36)}
    first = [(tuple(i.tolist()), float(g[tuple(i)]), float(w[tuple(i)])) for i in idx[:8]]
    raise AssertionError(f"{name}: {idx.shape[0]} of {g.numel()} elements differ; shape {tuple(g.shape)}; bounding box "
                         f"per axis {box}; spatial index residues {mods}; first (index, got, want): {first}")


def poison(t):
    """NaN-fill an output or a caller-owned workspace before the launch: an element nobody wrote cannot pass"""
    return t.fill_(float("nan"))


def prefill(shape, gen):
    """small integers for a destination that accumulates (float64, CPU)"""
    return ints(shape, 3, 4.0, gen)


# ------------------------------------------------------------------------------------------ layouts
def to_cl(x):    # [N, C, H, W] -> [N, H, W, C]
    return x.permute(0, 2, 3, 1).contiguous()


def to_cf(x):    # [N, H, W, C] -> [N, C, H, W]
    return x.permute(0, 3, 1, 2).contiguous()


# ------------------------------------------------------------------------------------------ conv cases
# kind -> (kernel size, stride, padding, transposed)
KINDS = {"3x3": (3, 1, 1, False), "1x1": (1, 1, 0, False), "down": (4, 2, 1, False), "up": (4, 2, 1, True)}


def out_hw(kind, H, W):
    k, s, p, tr = KINDS[kind]
    if tr:
        return (H - 1) * s - 2 * p + k, (W - 1) * s - 2 * p + k
    return (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1


class ConvCase:
    """One conv layer on integer data with its float64 reference (forward, data, weight and bias gradients), the regime
    asserted on that reference.  Channels-last tensors, float64, CPU:
    x [Nb, H, W, c1 + c2], dy / y / res [Nb, Ho, Wo, cout], dx / dres like x, w in the module's layout
    ([cout, cin, 1, k, k], transposed: [cin, cout, 1, k, k]), dw like w, bias / db [cout] (None without a bias);
    dw0 / db0: the integers the gradient destinations hold before the call."""

    def __init__(self, kind, dtype, Nb, H, W, c1, c2, cout, bias=True, target=1024.0):
        k, s, p, tr = KINDS[kind]
        self.kind, self.dtype, self.shape, self.has_bias = kind, dtype, (Nb, H, W, c1, c2, cout), bias
        cin = c1 + c2
        Ho, Wo = out_hw(kind, H, W)
        gen = gen_for(kind, str(dtype), Nb, H, W, c1, c2, cout, bias)
        # K of the forward and of the data gradient (a transposed / strided pair uses a quarter of the taps per output
        # on one side; the full k^2 is the safe side for both)
        Kmax = k * k * max(cin, cout)
        self.x = ints((Nb, H, W, cin), X_AMAX, X_E2, gen)
        self.dy = ints((Nb, Ho, Wo, cout), X_AMAX, X_E2, gen)
        wshape = (cin, cout, 1, k, k) if tr else (cout, cin, 1, k, k)
        self.w = ints(wshape, 1, weight_e2(Kmax, target), gen)
        self.bias = ints((cout,), 3, 4.0, gen) if bias else None
        self.res = ints((Nb, Ho, Wo, cout), 3, 4.0, gen)
        self.dres = ints((Nb, H, W, cin), 3, 4.0, gen)
        self.dw0 = prefill(wshape, gen)
        self.db0 = prefill((cout,), gen) if bias else None
        xr = to_cf(self.x).requires_grad_(True)
        wr = self.w[:, :, 0].clone().requires_grad_(True)
        fn = F.conv_transpose2d if tr else F.conv2d
        y = fn(xr, wr, self.bias, s, p)
        gx, gw = torch.autograd.grad(y, (xr, wr), to_cf(self.dy))
        self.y, self.dx, self.dw = to_cl(y.detach()), to_cl(gx), gw.unsqueeze(2)
        self.db = self.dy.sum((0, 1, 2)) if bias else None
        M = Nb * Ho * Wo
        refs = [self.y, self.dx, self.dw] + ([self.db] if bias else [])
        stored = [self.y, self.y + self.res, self.dx, self.dx + self.dres]
        # scalar upper bounds of sum |a||b|: K max|x| max|w| (+ bias) for y and dx, M max|x| max|dy| for dW
        bounds = [Kmax * X_AMAX * 1 + 3, M * X_AMAX * X_AMAX]
        if dtype == BF:
            check_regime(refs, stored, bounds)
        else:  # fp32 storage: the fused residual sum must also stay an exact fp32 integer
            check_regime(refs + [self.y + self.res, self.dx + self.dres], [], bounds)


def conv_launches(kind, dtype, Nb, H, W, c1, c2, cout):
    """the (role, argument tuple) of every conv launch VN.conv_forward / VN.conv_backward make for this layer, as the
    host-only variant queries take them: (dtype, Nb, Hi, Wi, C1, C2, Ho, Wo, Cout, Co1, KH, KW, S, P, U)"""
    k, s, p, tr = KINDS[kind]
    cin = c1 + c2
    Ho, Wo = out_hw(kind, H, W)
    if tr:
        assert c2 == 0
        fwd = (dtype, Nb, H, W, cin, 0, Ho, Wo, cout, cout, k, k, 1, k - 1 - p, s)
        dgrad = (dtype, Nb, Ho, Wo, cout, 0, H, W, cin, cin, k, k, s, p, 1)
        wgrad = dgrad      # the weight gradient of the plain strided conv dOut -> x grid
    else:
        fwd = (dtype, Nb, H, W, c1, c2, Ho, Wo, cout, cout, k, k, s, p, 1)
        dgrad = (dtype, Nb, Ho, Wo, cout, 0, H, W, cin, c1 if c2 else cin, k, k, 1, k - 1 - p, s)
        wgrad = fwd
    return [("fwd", fwd), ("dgrad", dgrad), ("wgrad", wgrad)]


def conv_kernel_names(kind, dtype, Nb, H, W, c1, c2, cout, bias=True):
    """(forward kernel names, weight-gradient kernel names, weight-gradient split counts) of the layer's launches,
    from the library's host-only queries, with the bias request kernels.conv_wgrad makes"""
    from cesm_emulator_amd import kernels as K
    from cesm_emulator_amd._lib import lib
    fwd, wg, ns = set(), set(), []
    tr = KINDS[kind][3]
    for role, a in conv_launches(kind, dtype, Nb, H, W, c1, c2, cout):
        if role != "wgrad":
            fwd.add(K.conv_fwd_variant(*a))
        else:
            geo = (K._DT[a[0]],) + a[1:]
            rides = int(bias and not tr and bool(lib().cesm_conv_wgrad_bias_rides(*geo)))
            wg.add(K.conv_wgrad_variant(*a, with_bias=bool(rides)))
            ns.append(lib().cesm_conv_wgrad_nsplit(*geo, rides))
    return fwd, wg, ns


# ------------------------------------------------------------------------------------------ the sweeps
# Every entry: (kind, dtype, Nb, H, W, c1, c2, cout, bias).  H, W: the layer's input grid.
def _cases(kind, dtype, Nb, hw, chans, bias=(True,)):
    hw = list(hw)
    return [(kind, dtype, Nb, H, W, c1, c2, co, b) for (c1, c2, co) in chans for (H, W) in hw for b in bias]


FULL_H = (1, 2, 3, 7, 8, 9, 13, 14, 15, 16, 17)
FULL_W = (1, 4, 31, 32, 33, 35, 36, 37, 64, 65, 72, 73)
RED_H, RED_W = (1, 9, 15), (33, 36, 72, 73)
# a. 3x3 same-size convs, bf16, Nb = 3 (tile counts that are no multiple of 8: the padded grid has phantom tiles)
SWEEP_3X3_FULL = _cases("3x3", BF, 3, itertools.product(FULL_H, FULL_W), [(64, 0, 64)]) + \
    _cases("3x3", BF, 3, itertools.product(FULL_H, FULL_W), [(64, 0, 128)])
SWEEP_3X3_REDUCED = _cases("3x3", BF, 3, itertools.product(RED_H, RED_W), [(64, 128, 64), (128, 0, 64), (256, 0, 512)]) + \
    [("3x3", BF, 3, 9, 36, 512, 0, 512, True)]
# c. 4x4 stride-2 down and its transpose up on the low-resolution grid (Hl, Wl); plus the odd-size and concat cases
# that take the generic bf16 kernel and its parity form
S2_HL, S2_WL = (1, 2, 7, 8, 9), (1, 31, 32, 33, 36, 64, 66, 72)
SWEEP_S2 = [("down", BF, 2, 2 * Hl, 2 * Wl, C, 0, C, True) for C in (64, 128) for Hl in S2_HL for Wl in S2_WL] + \
    [("up", BF, 2, Hl, Wl, C, 0, C, True) for C in (64, 128) for Hl in S2_HL for Wl in S2_WL]
SWEEP_S2_GENERIC = [("down", BF, 2, 9, 11, 64, 0, 64, True), ("down", BF, 2, 9, 11, 64, 0, 128, True),
                    ("down", BF, 2, 8, 12, 64, 64, 64, True), ("down", BF, 2, 8, 12, 64, 128, 64, True)]
# d. 1x1 convs as [1, 1, M, C] rows
M_1X1 = (1, 63, 64, 65, 255, 256, 257, 1000, 3001)
CH_1X1 = [(64, 0, 64), (64, 0, 128), (64, 0, 192), (64, 0, 768), (128, 0, 256), (256, 0, 64), (256, 0, 256), (64, 64, 64)]
SWEEP_1X1 = _cases("1x1", BF, 1, [(1, M) for M in M_1X1], CH_1X1, bias=(True, False))
# e. fp32 generic kernels
SWEEP_FP32 = [(kind, F32, Nb, H, W, c1, c2, co, True)
              for (Nb, H, W) in ((2, 5, 7), (3, 9, 33))
              for (kind, c1, c2, co) in (("3x3", 64, 0, 64), ("3x3", 64, 0, 128), ("down", 64, 0, 64),
                                         ("down", 64, 0, 128), ("up", 64, 0, 64), ("up", 64, 0, 128),
                                         ("3x3", 64, 64, 64), ("3x3", 64, 64, 128))]
SWEEPS = {"3x3_full": SWEEP_3X3_FULL, "3x3_reduced": SWEEP_3X3_REDUCED, "s2": SWEEP_S2, "s2_generic": SWEEP_S2_GENERIC,
          "1x1": SWEEP_1X1, "fp32": SWEEP_FP32}

# the complete name tables of cesm_conv_fwd_variant / cesm_conv_wgrad_variant (csrc/conv_fwd.hip kConvFwdVariantName,
# csrc/conv_wgrad.hip)
FWD_NAMES = {
    "gemm1x1_kernel<128>", "gemm1x1_kernel<64>", "conv3x3p_kernel<32,7,true>", "conv3x3_bf16_kernel<36>",
    "conv3x3_bf16_kernel<32>", "conv_fwd_bf16_kernel<128,true>", "conv_fwd_bf16_kernel<64,true>",
    "conv_fwd_bf16_kernel<128>", "conv_fwd_bf16_kernel<64>", "conv_fwd_kernel<float,128>", "conv_fwd_kernel<float,64>",
    "convs2_bf16_kernel<36,down>", "convs2_bf16_kernel<32,down>", "convs2_bf16_kernel<36,up>",
    "convs2_bf16_kernel<32,up>", "conv3x3ws_kernel<32>", "conv3x3ws_kernel<36>"}
WGRAD_NAMES = {"wgrad3x3c64_kernel", "wgrad3x3w36c64_kernel", "wgrads2_bf16_kernel", "conv_wgrad_kernel<float>"} | \
    {f"wgrad_sq_kernel<{t}{b}>" for t in ("64,256", "256,256", "256,128") for b in ("", ",true")} | \
    {f"wgrad_wide_kernel<{bm},{b}>" for bm in (64, 128, 256) for b in ("false", "true")}
# conv_wgrad_kernel<__bf16> is the generic kernel's bf16 form: the planner reaches it only at M >= 2^31 output pixels
# (the wide kernel's 32-bit pixel index), more than a GPU test can allocate -- no sweep can contain it
WGRAD_NAME_BIG_M = "conv_wgrad_kernel<__bf16>"


# ------------------------------------------------------------------------------------------ the headroom band
# check_regime keeps sum |a||b| below 2^22, two bits under the fp32 significand, in case the MFMA adder aligns its
# addends to the largest one.  These cases sit in the band that margin leaves out, 2^22 <= max sum |a||b| < 2^24
# (asserted on the reference; every partial sum is then still an exact fp32 integer if the adder keeps 24 bits), as
# (amax, M) of a 64 -> 128 1x1 weight gradient with operands uniform on [-amax, amax] over M pixels.
HEADROOM_CASES = [(128, 1024), (256, 256), (256, 512)]
HEADROOM_CH = (64, 128)


def headroom_case(amax, M):
    """x [M, 64], dy [M, 128], dW = dy^T x and sum |dy||x| (float64, CPU), the band asserted"""
    cin, cout = HEADROOM_CH
    g = gen_for("headroom", amax, M)
    full = amax * (amax + 1) / 3.0
    x, dy = ints((M, cin), amax, full, g), ints((M, cout), amax, full, g)
    dw = torch.einsum("mo,mi->oi", dy, x)
    sabs = torch.einsum("mo,mi->oi", dy.abs(), x.abs())
    assert amax <= BF16_EXACT and torch.equal(dw, dw.round())
    assert ACC_BOUND <= _amax(sabs) < FP32_INT, _amax(sabs)
    return x, dy, dw, sabs
