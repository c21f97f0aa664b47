"""Classifier-free guidance on the GPU: cesm_cond_mask, cesm_{ddpm,ddim,dpmpp}_step_cfg, Diffusion(p_uncond=) in
training and guidance_scale= in every sampler entry, on the eager and the HIP-graph path.

Kernel tests (no network).  x, eps and out of a guided kernel have 2 B rows: eps rows [0, B) are eps_c, rows [B, 2B)
eps_u; x is read from rows [0, B) only (the tests fill rows [B, 2B) of x with NaN) and x_prev goes to both halves.
  1 equal halves: eps_u a bit copy of eps_c gives the unguided kernel's bits at every scale (fma(s, 0, e) is exact);
  2 exact combine: integer-valued eps in [-64, 64] and scales with at most one fractional bit make every step of the
    combine exact, so the guided kernel equals the unguided one on the float64-combined eps, bit for bit;
  3 random data against the float64 expression with eps_g = eps_u + s (eps_c - eps_u).  Bound, elementwise, with
    E = |eps_u| + |s| (|eps_c| + |eps_u|):  12 * 2^-24 * (|a x| + |b| E + |sigma z| (+ |c x0_last|)).  Derivation: the
    neighbours' (test_gpu_ddim, test_gpu_dpmpp) update costs <= 4 * 2^-24 of that sum (one rounding of each
    coefficient, one of each product, two additions), now with |eps_g| <= E; the combine's three roundings (the
    subtraction, and the FMA counted as product and sum) add at most 2^-24 (|eps_u| + 3 |s| (|eps_c| + |eps_u|)) to
    eps_g, times |b| at most 4 * 2^-24 |b| E; together 8 * 2^-24, times 1.5 for margin.
    The DDPM kernel's chain is longer: c = beta / s1 (1 rounding), p = c g (1), d = x - p (1), m = r d (1), then
    sqrt(pv) (1), its product with z (1) and the last sum (1).  In units of 2^-24: the term r c g collects c, p, d, m
    and the last sum, 5, plus the combine's <= 3 through E, 8 |r c| E; r x collects d, m and the last sum, 3 |r x|;
    the noise term collects the square root, its product and the last sum, 3 |sqrt(pv) z|.  So <= 8 * 2^-24 of
    |r x| + |r c| E + |sqrt(pv) z| as well, and the same 12 * 2^-24 holds it with the same 1.5 margin;
  4 in place (out is x, x0_out is x0_last) equals out of place; z / x0_last full of NaN where the unguided kernel does
    not read them leak nothing;
  5 cond_mask: kept rows are cond's bits, dropped rows +0.0 even where cond is NaN, aliased out, argument errors.
Network tests (ch_mults (1, 2, 4), [2, 1, 16, 24], T = 12, or 6 for the ancestral loop; oracle and product share weights).
  6 guidance_scale None and 1.0 are the call without it, bit for bit, RNG state included, and launch no guided kernel;
  7 guided graph == guided eager bit for bit;
  8 against a float64 loop around the CPU oracle that evaluates ref(x, cond) and ref(x, 0) and combines them: relative
    L2 < (|1 - s| + |s|) * 1e-4 -- the project's 1e-4 for loops of this length times the factor by which the combine
    can amplify the two evaluations' errors; at s = 0 also within 1e-4 of the unguided sample(cond = 0);
  9 GraphSampleStep keeps x2's halves equal and cond2's second half zero;
 10 a guided sample_ensemble chunk equals guided sample() on the same rows; paired counterfactual_delta composes.
Training tests (B = 2, window cond, fp32 and bf16).
 11 keep=[True, False] equals a hand-zeroed cond in the loss and every parameter gradient; all True equals no keep;
 12 the drawn keep is rand(B) >= p, the third draw; p_uncond = 0 and eval() draw nothing more than today;
 13 input_grads: a dropped sample's d cond is exactly zero.
"""
import pytest
import torch

from cesm_emulator_amd import counterfactual_delta, input_grads, kernels as K
from cesm_emulator_amd._lib import KernelError, call
from cesm_emulator_amd.model import UNet, Diffusion, GraphSampleStep
from oracle import ref_cpu as R
from test_gpu_ddim import LAYOUTS, TIMES as DDIM_TIMES
from test_gpu_dpmpp import TIMES as DPMPP_TIMES

pytestmark = pytest.mark.gpu

EPS24 = 2.0 ** -24
SHAPE = (2, 1, 16, 24)
B3 = 3
# V = 1 on the three layouts (17x29 scalar, 24x44 vector, 24x44 from a 4-byte aligned pointer), and once V = 3
CASES = [(1, H, W, mis) for H, W, mis in LAYOUTS] + [(3, 17, 29, False)]


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return (torch.linalg.vector_norm(a - b) / torch.linalg.vector_norm(b).clamp_min(1e-30)).item()


def seed(s):
    torch.manual_seed(s)
    torch.cuda.manual_seed(s)


@pytest.fixture(scope="module")
def sched(dev):
    """the 1000-step schedule on the device (the kernel tests need no network)"""
    return Diffusion(torch.nn.Identity()).to(dev)


@pytest.fixture(scope="module")
def nets(dev):
    """one oracle / product network pair with the same weights"""
    torch.manual_seed(1)
    ref = R.UNet(ch_mults=(1, 2, 4))
    prod = UNet(ch_mults=(1, 2, 4))
    prod.load_state_dict(ref.state_dict())
    return ref, prod.to(dev)


def product(nets, dev, T, cdt, **kw):
    prod = nets[1]
    prod.compute_dtype = cdt
    return Diffusion(prod, timesteps=T, **kw).to(dev)


def blank(dev, rows, V, H, W, misalign):
    """an uninitialised [rows,V,H,W] tensor; misalign: its storage starts one float past a 16-byte boundary"""
    n = rows * V * H * W
    buf = torch.empty(n + 1, device=dev)
    out = buf[1:].view(rows, V, H, W) if misalign else buf[:n].view(rows, V, H, W)
    assert (out.data_ptr() % 16 != 0) == misalign
    return out


def like(dev, src, misalign):
    out = blank(dev, *src.shape, misalign)
    out.copy_(src)
    return out


class Data:
    """inputs of one layout: x2 (rows [B, 2B) NaN: never read), eps2 = [eps_c, eps_u], z and x0_last with B rows"""

    def __init__(self, dev, V, H, W, misalign, kind, sd=3):
        g = torch.Generator(device=dev).manual_seed(sd)
        self.dev, self.mis, self.shape = dev, misalign, (V, H, W)

        def draw(rows):
            if kind == "int":
                return torch.randint(-64, 65, (rows, V, H, W), device=dev, generator=g).float()
            return torch.randn(rows, V, H, W, device=dev, generator=g)

        x = torch.randn(B3, V, H, W, device=dev, generator=g)
        ec = draw(B3)
        eu = ec.clone() if kind == "equal" else draw(B3)
        self.x2 = like(dev, torch.cat([x, torch.full_like(x, float("nan"))]), misalign)
        self.eps2 = like(dev, torch.cat([ec, eu]), misalign)
        self.z = like(dev, torch.randn(B3, V, H, W, device=dev, generator=g), misalign)
        self.h = like(dev, torch.randn(B3, V, H, W, device=dev, generator=g), misalign)
        self.x, self.ec, self.eu = self.x2[:B3], self.eps2[:B3], self.eps2[B3:]

    def eps_g(self, s):
        """the float64-combined eps as an fp32 tensor laid out like eps_c"""
        g = self.eu.double() + s * (self.ec.double() - self.eu.double())
        return like(self.dev, g.float(), self.mis), g

    def E(self, s):
        return self.eu.double().abs() + abs(s) * (self.ec.double().abs() + self.eu.double().abs())


def halves(out):
    assert out.shape[0] == 2 * B3
    assert torch.equal(out[:B3], out[B3:])
    return out[:B3]


def guided_and_plain(name, sched, D, s, eps_plain, tv, eta=None, z="z", h="h", inplace=False):
    """(guided x_prev [2B], guided x0 or None, unguided x_prev on eps_plain, unguided x0 or None) of one kernel"""
    dev, ac = D.dev, sched.alphas_cumprod
    ts = [torch.tensor(v, device=dev) for v in tv]
    z = {"z": D.z, "nan": torch.full_like(D.z, float("nan")), None: None}[z]
    h = {"h": D.h, "nan": torch.full_like(D.h, float("nan")), None: None}[h]
    x2 = like(dev, D.x2, D.mis) if inplace else D.x2
    kw = {"out": x2} if inplace else {}
    if name == "ddpm":
        got = K.ddpm_step_cfg(x2, D.eps2, z, ts[0], *sched._coefs(), s, **kw)
        want = None if eps_plain is None else K.ddpm_step(D.x, eps_plain, z, ts[0], *sched._coefs())
        return got, None, want, None
    if name == "ddim":
        got = K.ddim_step_cfg(x2, D.eps2, z, ts[0], ts[1], ac, eta, s, **kw)
        want = None if eps_plain is None else K.ddim_step(D.x, eps_plain, z, ts[0], ts[1], ac, eta)
        return got, None, want, None
    if inplace and h is not None:
        h = like(dev, h, D.mis)
        kw["x0_out"] = h
    got, got0 = K.dpmpp_step_cfg(x2, D.eps2, h, *ts, ac, s, **kw)
    if inplace:
        assert got is x2 and (h is None or got0 is h)
    want, want0 = (None, None) if eps_plain is None else K.dpmpp_step(D.x, eps_plain, h, *ts, ac)
    return got, got0, want, want0


def kernel_runs():
    """(name, times, eta) of every kernel case: DDPM on the DDIM t's, DDIM at eta 0 and 0.5, DPM-Solver++ with its
    t_last cases"""
    for tv, _ in DDIM_TIMES:
        yield "ddpm", (tv,), None
    for tv, tpv in DDIM_TIMES:
        for eta in (0.0, 0.5):
            yield "ddim", (tv, tpv), eta
    for tr in DPMPP_TIMES:
        yield "dpmpp", tr, None


# ------------------------------------------------------------------------------------------------ 1, 2: exact
@pytest.mark.parametrize("V,H,W,misalign", CASES)
def test_equal_halves_give_the_unguided_bits(dev, sched, V, H, W, misalign):
    D = Data(dev, V, H, W, misalign, "equal")
    assert torch.equal(D.ec, D.eu)
    for name, tv, eta in kernel_runs():
        for s in (0.0, 0.3, 1.0, 2.5):
            got, got0, want, want0 = guided_and_plain(name, sched, D, s, D.ec, tv, eta)
            assert torch.isfinite(got).all()
            assert torch.equal(halves(got), want), (name, tv, eta, s)
            if got0 is not None:
                assert got0.shape[0] == B3 and torch.equal(got0, want0), (name, tv, s)


@pytest.mark.parametrize("V,H,W,misalign", CASES)
def test_exact_combine_on_integer_eps(dev, sched, V, H, W, misalign):
    D = Data(dev, V, H, W, misalign, "int")
    for s in (0.0, 0.5, 1.5, 2.0, 3.0):
        eg, eg64 = D.eps_g(s)
        assert torch.equal(eg.double(), eg64)  # exact in fp32
        for name, tv, eta in kernel_runs():
            got, got0, want, want0 = guided_and_plain(name, sched, D, s, eg, tv, eta)
            assert torch.equal(halves(got), want), (name, tv, eta, s)
            if got0 is not None:
                assert torch.equal(got0, want0), (name, tv, s)
    # and the two halves are told apart: s = 0 is eps_u's result, s = 1 eps_c's
    tv, tpv = DDIM_TIMES[0]
    for s, e in ((0.0, D.eu), (1.0, D.ec)):
        got, _, want, _ = guided_and_plain("ddim", sched, D, s, like(dev, e, misalign), (tv, tpv), 0.0)
        assert torch.equal(halves(got), want)
    assert not torch.equal(D.ec, D.eu)


# ------------------------------------------------------------------------------------------------ 3: float64
def view4(c):
    return c.view(-1, 1, 1, 1)


@pytest.mark.parametrize("V,H,W,misalign", CASES)
def test_random_data_against_float64_expression(dev, sched, V, H, W, misalign):
    D = Data(dev, V, H, W, misalign, "random")
    xd, zd, hd = D.x.double(), D.z.double(), D.h.double()
    worst = {}
    for s in (0.0, 0.3, 2.5, 7.0):
        g64, E = D.eps_g(s)[1], D.E(s)
        for name, tv, eta in kernel_runs():
            got, got0, _, _ = guided_and_plain(name, sched, D, s, None, tv, eta)
            got = halves(got).double()
            ts = [torch.tensor(v, device=dev) for v in tv]
            if name == "ddpm":
                t = ts[0]
                r, sg = view4(sched.sqrt_recip_alphas[t].double()), view4(sched.posterior_variance[t].double().sqrt())
                c = view4(sched.betas[t].double() / sched.sqrt_one_minus_alphas_cumprod[t].double())
                ref = r * (xd - c * g64) + sg * zd
                mag = (r * xd).abs() + (r * c).abs() * E + (sg * zd).abs()
            elif name == "ddim":
                a, b, sg = (view4(v) for v in sched.ddim_coefs(ts[0], ts[1], eta))
                ref = a * xd + b * g64 + sg * zd
                mag = (a * xd).abs() + b.abs() * E + (sg * zd).abs()
            else:
                a, b, c, c1, c2 = (view4(v) for v in sched.dpmpp_coefs(*ts))
                ref = a * xd + b * g64 + c * hd
                mag = (a * xd).abs() + b.abs() * E + (c * hd).abs()
                err0 = (got0.double() - (c1 * xd + c2 * g64)).abs()
                bound0 = 12 * EPS24 * ((c1 * xd).abs() + c2.abs() * E)
                worst["dpmpp x0"] = max(worst.get("dpmpp x0", 0.0), (err0 / bound0.clamp_min(1e-300)).max().item())
                assert (err0 <= bound0).all(), (name, tv, s)
            err, bound = (got - ref).abs(), 12 * EPS24 * mag
            worst[name] = max(worst.get(name, 0.0), (err / bound.clamp_min(1e-300)).max().item())
            assert (err <= bound).all(), (name, tv, eta, s)
    print(f"{V}x{H}x{W} misalign={misalign}: worst |err| / bound " +
          ", ".join(f"{k} {v:.3f}" for k, v in sorted(worst.items())))


# ------------------------------------------------------------------------------------------------ 4: aliasing
@pytest.mark.parametrize("V,H,W,misalign", CASES)
def test_in_place_and_unread_buffers(dev, sched, V, H, W, misalign):
    D = Data(dev, V, H, W, misalign, "random")
    s = 2.5
    for name, tv, eta in kernel_runs():
        got, got0, _, _ = guided_and_plain(name, sched, D, s, None, tv, eta)
        gi, gi0, _, _ = guided_and_plain(name, sched, D, s, None, tv, eta, inplace=True)
        assert torch.equal(gi, got) and torch.equal(gi[:B3], gi[B3:]), (name, tv, eta)
        if got0 is not None:
            assert torch.equal(gi0, got0), (name, tv)
    # z is not read at eta = 0, nor when it is null; x0_last is not read without history
    tv, tpv = DDIM_TIMES[0]
    want = guided_and_plain("ddim", sched, D, s, None, (tv, tpv), 0.0, z=None)[0]
    got = guided_and_plain("ddim", sched, D, s, None, (tv, tpv), 0.0, z="nan")[0]
    assert torch.equal(got, want) and torch.isfinite(want).all()
    want = guided_and_plain("ddpm", sched, D, s, None, (tv,), z=None)[0]
    assert torch.isfinite(want).all()
    none = [-1, -1, -1]
    want = guided_and_plain("dpmpp", sched, D, s, None, (tv, tpv, none), h=None)
    got = guided_and_plain("dpmpp", sched, D, s, None, (tv, tpv, none), h="nan")
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    assert torch.isfinite(want[0]).all() and torch.isfinite(want[1]).all()
    # the mixed triple of test_gpu_dpmpp: only row 1 has a history
    t, tp, tl = (torch.tensor(v, device=dev) for v in DPMPP_TIMES[0])
    hn = like(dev, D.h, misalign)
    hn[0], hn[2] = float("nan"), float("nan")
    want = K.dpmpp_step_cfg(D.x2, D.eps2, D.h, t, tp, tl, sched.alphas_cumprod, s)
    got = K.dpmpp_step_cfg(D.x2, D.eps2, hn, t, tp, tl, sched.alphas_cumprod, s)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]) and torch.isfinite(want[0]).all()


def test_guided_kernel_argument_checks(dev, sched):
    x2, x = torch.zeros(4, 1, 4, 4, device=dev), torch.zeros(2, 1, 4, 4, device=dev)
    t, tp, tl = (torch.tensor(v, device=dev) for v in ([5, 5], [3, 3], [-1, 7]))
    ac = sched.alphas_cumprod
    st = torch.cuda.current_stream().cuda_stream
    p, q = x2.data_ptr(), x.data_ptr()
    tabs = [c.data_ptr() for c in sched._coefs()]
    nan, inf = float("nan"), float("inf")
    for B, HW, T, s in ((0, 16, 1000, 2.0), (2, 0, 1000, 2.0), (2, 16, 0, 2.0), (2, 16, 1000, -1.0),
                        (2, 16, 1000, nan), (2, 16, 1000, inf)):
        with pytest.raises(KernelError):
            call("cesm_ddim_step_cfg", p, p, 0, t.data_ptr(), tp.data_ptr(), ac.data_ptr(), 0.0, p, B, HW, T, s, st)
        with pytest.raises(KernelError):
            call("cesm_dpmpp_step_cfg", p, p, 0, t.data_ptr(), tp.data_ptr(), tl.data_ptr(), ac.data_ptr(), p, q, B, HW,
                 T, s, st)
        if T:
            with pytest.raises(KernelError):
                call("cesm_ddpm_step_cfg", p, p, 0, t.data_ptr(), *tabs, p, B, HW, s, st)
    with pytest.raises(KernelError):  # null eps
        call("cesm_ddim_step_cfg", p, 0, 0, t.data_ptr(), tp.data_ptr(), ac.data_ptr(), 0.0, p, 2, 16, 1000, 2.0, st)
    with pytest.raises(KernelError):  # null out
        call("cesm_ddpm_step_cfg", p, p, 0, t.data_ptr(), *tabs, 0, 2, 16, 2.0, st)
    torch.cuda.synchronize()
    # the bindings: shapes (2 B rows for x / eps / out, B for the rest) and dtypes
    with pytest.raises(RuntimeError):
        K.ddim_step_cfg(x2[:3], x2[:3], None, t, tp, ac, 0.0, 2.0)
    with pytest.raises(RuntimeError):
        K.ddim_step_cfg(x2, x, None, t, tp, ac, 0.0, 2.0)
    with pytest.raises(RuntimeError):
        K.ddim_step_cfg(x2, x2, x2, t, tp, ac, 0.5, 2.0)
    with pytest.raises(RuntimeError):
        K.ddim_step_cfg(x2, x2, None, t.repeat(2), tp, ac, 0.0, 2.0)
    with pytest.raises(RuntimeError):
        K.ddpm_step_cfg(x2, x2, None, t.int(), *sched._coefs(), 2.0)
    with pytest.raises(RuntimeError):
        K.dpmpp_step_cfg(x2, x2, x2, t, tp, tl, ac, 2.0)
    with pytest.raises(RuntimeError):
        K.dpmpp_step_cfg(x2, x2, None, t, tp, tl, ac, 2.0, x0_out=x2)
    with pytest.raises(ValueError):
        K.ddim_step_cfg(x2, x2, None, t, tp, ac, -1.0, 2.0)
    with pytest.raises(ValueError):
        K.ddim_step_cfg(x2, x2, None, t, tp, ac, 0.0, -2.0)


# ------------------------------------------------------------------------------------------------ 5: cond_mask
@pytest.mark.parametrize("shape,misalign", [((3, 1, 17, 29), False), ((3, 1, 24, 44), False), ((3, 1, 24, 44), True),
                                            ((3, 2, 3, 16, 24), False)])
def test_cond_mask(dev, shape, misalign):
    g = torch.Generator(device=dev).manual_seed(6)
    n = 1
    for v in shape:
        n *= v
    buf = torch.empty(n + 1, device=dev)
    cond = (buf[1:] if misalign else buf[:n]).view(shape)
    assert (cond.data_ptr() % 16 != 0) == misalign
    cond.copy_(torch.randn(shape, device=dev, generator=g))
    for kv in ([True, False, True], [False, False, False], [True, True, True], [False, True, False]):
        keep = torch.tensor(kv, device=dev)
        src = cond.clone() if not misalign else (torch.empty(n + 1, device=dev)[1:].view(shape).copy_(cond))
        for b, k in enumerate(kv):
            if not k:  # a dropped sample is not read: NaN and Inf there do not reach out
                src[b] = float("nan")
                src[b].view(-1)[::3] = float("inf")
        out = K.cond_mask(src, keep)
        assert out.shape == src.shape and out.dtype == torch.float32
        for b, k in enumerate(kv):
            if k:
                assert torch.equal(out[b], cond[b])
            else:
                assert bool((out[b] == 0).all()) and not bool(torch.signbit(out[b]).any())
        # aliased
        assert K.cond_mask(src, keep, out=src) is src
        assert torch.equal(src, out)


def test_cond_mask_argument_checks(dev):
    c = torch.zeros(2, 1, 4, 4, device=dev)
    k = torch.ones(2, dtype=torch.bool, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    for args in ((c.data_ptr(), k.data_ptr(), c.data_ptr(), 0, 16), (c.data_ptr(), k.data_ptr(), c.data_ptr(), 2, 0),
                 (0, k.data_ptr(), c.data_ptr(), 2, 16), (c.data_ptr(), 0, c.data_ptr(), 2, 16),
                 (c.data_ptr(), k.data_ptr(), 0, 2, 16)):
        with pytest.raises(KernelError):
            call("cesm_cond_mask", *args, st)
    with pytest.raises(RuntimeError):
        K.cond_mask(c, k.float())
    with pytest.raises(RuntimeError):
        K.cond_mask(c, k[:1])
    with pytest.raises(RuntimeError):
        K.cond_mask(c.double(), k)
    with pytest.raises(RuntimeError):
        K.cond_mask(c, k, out=c[:1])


# ------------------------------------------------------------------------------------------------ 6: unchanged path
SOLVERS = {"ddpm": dict(), "ddim0": dict(steps=5), "ddim": dict(steps=5, ddim_eta=0.7),
           "dpmpp2m": dict(steps=5, solver="dpmpp2m")}


def T_of(name):
    return 6 if name == "ddpm" else 12


@pytest.mark.parametrize("use_graph", [False, True])
@pytest.mark.parametrize("name", ["ddpm", "ddim", "dpmpp2m"])
def test_none_and_one_are_the_unguided_call(dev, nets, monkeypatch, name, use_graph):
    d = product(nets, dev, T_of(name), torch.bfloat16)
    kw = SOLVERS[name]
    g = torch.Generator(device=dev).manual_seed(2)
    cond = torch.randn(SHAPE, device=dev, generator=g)

    def refuse(*a, **k):
        raise AssertionError("a guided kernel was launched on the unguided path")

    seed(3)
    y0 = d.sample(cond, SHAPE, dev, use_graph=use_graph, **kw)
    state0 = torch.cuda.get_rng_state()
    e0 = d.sample_ensemble(cond, 2, use_graph=use_graph, **kw)
    for fn in ("ddpm_step_cfg", "ddim_step_cfg", "dpmpp_step_cfg", "cond_mask"):
        monkeypatch.setattr(K, fn, refuse)
    for gs in (None, 1.0, 1):
        seed(3)
        y = d.sample(cond, SHAPE, dev, use_graph=use_graph, guidance_scale=gs, **kw)
        assert torch.equal(torch.cuda.get_rng_state(), state0), gs
        assert torch.equal(y, y0), gs
        e = d.sample_ensemble(cond, 2, use_graph=use_graph, guidance_scale=gs, **kw)
        assert torch.equal(e, e0), gs
    if use_graph:
        step = GraphSampleStep(d, cond, torch.zeros(SHAPE, device=dev), guidance_scale=1.0,
                               ddim_eta=None if name == "ddpm" else kw.get("ddim_eta", 0.0),
                               solver=kw.get("solver", "ddim"))
        assert step.scale is None and step.x2 is None and step.cond2 is None and step.t2 is None


# ------------------------------------------------------------------------------------------------ 7: graph == eager
@pytest.mark.parametrize("cdt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("name", ["ddpm", "ddim0", "ddim", "dpmpp2m"])
def test_guided_graph_equals_guided_eager(dev, nets, name, cdt):
    d = product(nets, dev, T_of(name), cdt)
    kw = SOLVERS[name]
    g = torch.Generator(device=dev).manual_seed(2)
    conds = [torch.randn(SHAPE, device=dev, generator=g)]
    if cdt == torch.bfloat16:
        conds.append(torch.randn(2, 1, 3, 16, 24, device=dev, generator=g))  # a window
    for cond in conds:
        seed(7)
        y_eager = d.sample(cond, SHAPE, dev, use_graph=False, guidance_scale=2.0, **kw)
        state = torch.cuda.get_rng_state()
        seed(7)
        y_graph = d.sample(cond, SHAPE, dev, use_graph=True, guidance_scale=2.0, **kw)
        assert y_graph.shape == SHAPE and torch.isfinite(y_graph).all()
        assert torch.equal(y_graph, y_eager)
        # RNG use is that of the unguided call, and guidance changes the result
        assert torch.equal(torch.cuda.get_rng_state(), state)
        seed(7)
        y_plain = d.sample(cond, SHAPE, dev, use_graph=True, **kw)
        assert torch.equal(torch.cuda.get_rng_state(), state)
        assert not torch.equal(y_plain, y_graph)


def test_guided_graph_equals_guided_eager_two_variables(dev):
    torch.manual_seed(4)
    net = UNet(out_channels=2, ch_mults=(1, 2, 4)).to(dev)
    d = Diffusion(net, timesteps=12).to(dev)
    shape = (2, 2, 16, 24)
    g = torch.Generator(device=dev).manual_seed(2)
    cond = torch.randn(shape, device=dev, generator=g)
    x_T = torch.randn(shape, device=dev, generator=g)
    for kw in (SOLVERS["ddim"], SOLVERS["dpmpp2m"]):
        seed(7)
        y_eager = d.sample(cond, shape, dev, use_graph=False, x_T=x_T, guidance_scale=0.5, **kw)
        seed(7)
        y_graph = d.sample(cond, shape, dev, use_graph=True, x_T=x_T, guidance_scale=0.5, **kw)
        assert y_graph.shape == shape and torch.isfinite(y_graph).all()
        assert torch.equal(y_graph, y_eager)


# ------------------------------------------------------------------------------------------------ 8: oracle loop
SCALES = (0.0, 2.0)


@pytest.fixture(scope="module")
def oracle_runs(nets):
    """float64 loops around the CPU oracle network: per step eps_c = ref(x, cond) and eps_u = ref(x, 0), combined as
    eps_u + s (eps_c - eps_u); the updates of ddim_coefs (4 of 12, eta = 0.5), dpmpp_coefs (4 of 12, log-SNR grid) and
    the DDPM tables (T = 6)"""
    ref = nets[0]
    g = torch.Generator().manual_seed(11)
    cond = torch.randn(SHAPE, generator=g)
    x_T = torch.randn(SHAPE, generator=g)
    noise_seq = torch.randn(6, *SHAPE, generator=g)
    zero = torch.zeros_like(cond)

    def eps_of(x, tt, s):
        """both evaluations in one call of the oracle (its samples do not interact): rows [cond, 0]"""
        t = torch.full((2 * SHAPE[0],), tt, dtype=torch.long)
        xf = x.float()
        ec, eu = ref(torch.cat([xf, xf]), torch.cat([cond, zero]), t).double().chunk(2)
        return eu + s * (ec - eu)

    out = {}
    with torch.no_grad():
        d = Diffusion(torch.nn.Identity(), timesteps=12)
        for s in SCALES:
            tau = d.sample_schedule(4)
            x = x_T.double()
            for k, (tt, tp) in enumerate(zip(reversed(tau), reversed([-1] + tau[:-1]))):
                a, b, sg = d.ddim_coefs(tt, tp, 0.5)
                x = a * x + b * eps_of(x, tt, s) + sg * noise_seq[k].double()
            out["ddim", s] = x
            tau = d.sample_schedule(4, "logsnr")
            x, x0_last, tl = x_T.double(), torch.zeros(SHAPE, dtype=torch.float64), -1
            for tt, tp in zip(reversed(tau), reversed([-1] + tau[:-1])):
                eps = eps_of(x, tt, s)
                a, b, c, c1, c2 = d.dpmpp_coefs(tt, tp, tl)
                x, x0_last, tl = a * x + b * eps + c * x0_last, c1 * x + c2 * eps, tt
            out["dpmpp2m", s] = x
        d6 = Diffusion(torch.nn.Identity(), timesteps=6)
        for s in SCALES:
            x = x_T.double()
            for i, tt in enumerate(reversed(range(6))):
                r, b = d6.sqrt_recip_alphas[tt].double(), d6.betas[tt].double()
                s1, pv = d6.sqrt_one_minus_alphas_cumprod[tt].double(), d6.posterior_variance[tt].double()
                x = r * (x - b / s1 * eps_of(x, tt, s))
                if tt > 0:
                    x = x + pv.sqrt() * noise_seq[i].double()
            out["ddpm", s] = x
    return cond, x_T, noise_seq, out


ORACLE_KW = {"ddpm": dict(), "ddim": dict(steps=4, ddim_eta=0.5), "dpmpp2m": dict(steps=4, solver="dpmpp2m")}


@pytest.mark.parametrize("use_graph", [False, True])
@pytest.mark.parametrize("s", SCALES)
@pytest.mark.parametrize("name", ["ddpm", "ddim", "dpmpp2m"])
def test_guided_runs_match_oracle_loop_fp32(dev, nets, oracle_runs, name, s, use_graph):
    cond, x_T, noise_seq, want = oracle_runs
    d = product(nets, dev, T_of(name), torch.float32)
    kw = dict(ORACLE_KW[name], use_graph=use_graph, x_T=x_T)
    if name != "dpmpp2m":
        kw["noise_seq"] = noise_seq.to(dev) if name == "ddpm" else noise_seq[:4].to(dev)
    y = d.sample(cond.to(dev), SHAPE, dev, guidance_scale=s, **kw)
    err, gate = rel(y, want[name, s]), (abs(1 - s) + abs(s)) * 1e-4
    print(f"{name} s={s} fp32 vs the guided oracle loop (graph={use_graph}): rel {err:.3e} (gate {gate:.1e})")
    assert err < gate
    if s == 0.0:  # the unconditional sampler
        y0 = d.sample(torch.zeros(SHAPE, device=dev), SHAPE, dev, **kw)
        e0 = rel(y, y0)
        print(f"{name} s=0 vs the unguided sample(cond = 0): rel {e0:.3e}")
        assert e0 < 1e-4


# ------------------------------------------------------------------------------------------------ 9: the graph step
@pytest.mark.parametrize("name", ["ddpm", "ddim", "dpmpp2m"])
def test_graph_step_invariants(dev, nets, name):
    d = product(nets, dev, 12, torch.bfloat16)
    g = torch.Generator(device=dev).manual_seed(9)
    cond = torch.randn(2, 1, 3, 16, 24, device=dev, generator=g)
    x = torch.randn(SHAPE, device=dev, generator=g)
    eta = {"ddpm": None, "ddim": 0.5, "dpmpp2m": 0.0}[name]
    step = GraphSampleStep(d, cond, x, ddim_eta=eta, solver="dpmpp2m" if name == "dpmpp2m" else "ddim",
                           guidance_scale=2.0)
    Bn = SHAPE[0]

    def check():
        assert torch.equal(step.x2[:Bn], step.x2[Bn:])
        assert not bool(step.cond2[Bn:].any())
        assert torch.isfinite(step.x2).all()

    assert step.scale == 2.0
    assert step.x2.shape == (2 * Bn, *SHAPE[1:]) and step.cond2.shape == (2 * Bn, *cond.shape[1:])
    assert step.t2.shape == (2 * Bn,)
    for view, whole in ((step.x, step.x2), (step.cond, step.cond2), (step.t, step.t2)):
        assert view.data_ptr() == whole.data_ptr() and view.shape[0] == Bn
    for buf in (step.z, step.x0_last, step.t_prev, step.t_last):
        assert buf is None or buf.shape[0] == Bn
    assert torch.equal(step.x, x) and torch.equal(step.cond, cond)  # the warm-up steps are undone
    check()
    x_new, cond_new = torch.randn(SHAPE, device=dev, generator=g), torch.randn_like(cond)
    step.load(cond_new, x_new)
    assert torch.equal(step.x, x_new) and torch.equal(step.cond, cond_new)
    check()
    runs = {"ddpm": [(11,), (5,), (0,)], "ddim": [(11, 7), (7, 0), (0, -1)],
            "dpmpp2m": [(11, 7, -1), (7, 0, 11), (0, -1, 7)]}[name]
    for args in runs:
        if step.z is not None:
            step.z.normal_()
        step.run(*args)
        assert bool((step.t2 == args[0]).all())
        check()
    with pytest.raises(ValueError):
        step.load(cond_new, torch.zeros(4, 1, 16, 24, device=dev))


# ------------------------------------------------------------------------------------------------ 10: ensembles
def test_guided_ensemble_chunks_equal_guided_sample(dev, nets):
    d = product(nets, dev, 12, torch.float32)
    Bc, M, V, H, W = 2, 3, 1, 16, 24
    g = torch.Generator(device=dev).manual_seed(14)
    cond = torch.randn(Bc, V, H, W, device=dev, generator=g)
    x_T = torch.randn(Bc, M, V, H, W, device=dev, generator=g)
    noise = torch.randn(4, Bc, M, V, H, W, device=dev, generator=g)
    jobs = Bc * M
    rep, xf, nf = cond.repeat_interleave(M, 0), x_T.reshape(jobs, V, H, W), noise.reshape(4, jobs, V, H, W)
    for kw in (dict(steps=4, ddim_eta=0.5), dict(steps=4, solver="dpmpp2m")):
        for use_graph in (False, True):
            mb = 4  # chunks of 4 and 2 fields: network batches of 8 and 4
            ens = d.sample_ensemble(cond, M, member_batch=mb, x_T=x_T, noise_seq=noise, use_graph=use_graph,
                                    guidance_scale=2, **kw)
            flat = ens.view(jobs, V, H, W)
            for j0 in range(0, jobs, mb):
                j1 = min(j0 + mb, jobs)
                want = d.sample(rep[j0:j1], (j1 - j0, V, H, W), dev, use_graph=use_graph, x_T=xf[j0:j1],
                                noise_seq=nf[:, j0:j1], guidance_scale=2, **kw)
                assert torch.equal(flat[j0:j1], want), (kw, use_graph, j0)
            assert torch.isfinite(ens).all() and not torch.equal(ens[:, 0], ens[:, 1])
            plain = d.sample_ensemble(cond, M, member_batch=mb, x_T=x_T, noise_seq=noise, use_graph=use_graph, **kw)
            assert not torch.equal(plain, ens)


def test_guided_paired_counterfactual_delta(dev, nets):
    d = product(nets, dev, 12, torch.float32)
    g = torch.Generator(device=dev).manual_seed(13)
    cond = torch.randn(SHAPE, device=dev, generator=g)
    kw = dict(steps=4, ddim_eta=0.5, guidance_scale=2)
    seed(6)
    base = d.sample(cond, SHAPE, dev, **kw)
    for use_graph in ("0", "1"):
        mp = pytest.MonkeyPatch()
        mp.setenv("CESM_SAMPLE_GRAPH", use_graph)
        try:
            seed(6)
            same = counterfactual_delta(d, cond, scale=1.0, paired=True, **kw)
            seed(6)
            diff = counterfactual_delta(d, cond, scale=1.1, paired=True, **kw)
            seed(6)
            same_n = counterfactual_delta(d, cond, scale=1.0, paired=True, n_samples=2, **kw)
        finally:
            mp.undo()
        assert same.shape == SHAPE and diff.shape == SHAPE and same_n.shape == SHAPE
        print(f"guided paired (graph={use_graph}), scale = 1: max |delta| {same.abs().max().item():.3e}, "
              f"max |base| {base.abs().max().item():.3e}; scale = 1.1: max |delta| {diff.abs().max().item():.3e}")
        assert same.abs().max().item() <= 1e-4 * base.abs().max().item()
        assert same_n.abs().max().item() <= 1e-4 * base.abs().max().item()
        assert torch.isfinite(diff).all() and diff.abs().max().item() > 0
    # unpaired: two guided runs, base first
    seed(5)
    delta = counterfactual_delta(d, cond, scale=1.1, **kw)
    seed(5)
    b0 = d.sample(cond, SHAPE, dev, **kw)
    p0 = d.sample(cond * 1.1, SHAPE, dev, **kw)
    assert torch.equal(delta, p0 - b0)


# ------------------------------------------------------------------------------------------------ 11-13: training
def train_inputs(dev):
    g = torch.Generator(device=dev).manual_seed(21)
    x0 = torch.randn(SHAPE, device=dev, generator=g)
    cond = torch.randn(2, 1, 3, 16, 24, device=dev, generator=g)
    t = torch.tensor([3, 9], device=dev)
    noise = torch.randn(SHAPE, device=dev, generator=g)
    return x0, cond, t, noise


def loss_and_grads(d, x0, cond, **kw):
    d.zero_grad(set_to_none=True)
    loss = d.loss(x0, cond, **kw)
    loss.backward()
    grads = {n: p.grad.clone() for n, p in d.named_parameters() if p.grad is not None}
    d.zero_grad(set_to_none=True)
    return loss.detach().clone(), grads


def same(a, b):
    la, ga = a
    lb, gb = b
    assert torch.equal(la, lb)
    assert ga.keys() == gb.keys() and len(ga) > 10
    for n in ga:
        assert torch.equal(ga[n], gb[n]), n


@pytest.mark.parametrize("cdt", [torch.float32, torch.bfloat16])
def test_masked_loss_equals_hand_zeroed_cond(dev, nets, cdt):
    x0, cond, t, noise = train_inputs(dev)
    for d in (product(nets, dev, 12, cdt), product(nets, dev, 12, cdt, lat_weight=0.5, min_snr_gamma=5.0)):
        d.train()
        zeroed = cond.clone()
        zeroed[1] = 0
        got = loss_and_grads(d, x0, cond, t=t, noise=noise, keep=torch.tensor([True, False], device=dev))
        same(got, loss_and_grads(d, x0, zeroed, t=t, noise=noise))
        same(loss_and_grads(d, x0, cond, t=t, noise=noise, keep=[True, False]), got)  # a host list is taken too
        plain = loss_and_grads(d, x0, cond, t=t, noise=noise)
        same(loss_and_grads(d, x0, cond, t=t, noise=noise, keep=torch.tensor([True, True], device=dev)), plain)
        assert not torch.equal(plain[0], got[0])
        with pytest.raises(ValueError):
            d.loss(x0, cond, t=t, noise=noise, keep=torch.tensor([True], device=dev))
    c = d.loss_components(x0, cond, t=t, noise=noise, keep=[True, False])
    assert torch.equal(c["total"].detach(), got[0])
    d.zero_grad(set_to_none=True)


@pytest.mark.parametrize("cdt", [torch.float32, torch.bfloat16])
def test_keep_is_drawn_by_the_stated_rule(dev, nets, cdt):
    x0, cond, _, _ = train_inputs(dev)
    T, p, Bn = 12, 0.5, SHAPE[0]

    def draws(sd, with_keep):
        g = torch.Generator(device=dev).manual_seed(sd)
        t = torch.randint(0, T, (Bn,), device=dev, generator=g).long()
        noise = torch.randn(x0.shape, device=dev, dtype=x0.dtype, generator=g)
        keep = (torch.rand(Bn, device=dev, generator=g) >= p) if with_keep else None
        return t, noise, keep, g.get_state()

    # a seed whose draw keeps one sample and drops the other
    sd = next(s for s in range(100) if draws(s, True)[2].tolist() in ([True, False], [False, True]))
    t, noise, keep, state3 = draws(sd, True)
    state2 = draws(sd, False)[3]
    assert not torch.equal(state2, state3)
    with torch.no_grad():
        d = product(nets, dev, T, cdt, p_uncond=p)
        d.train()
        d.generator = torch.Generator(device=dev).manual_seed(sd)
        got = d.loss(x0, cond)
        assert torch.equal(d.generator.get_state(), state3)  # randint, randn, rand: three draws
        assert torch.equal(got, d.loss(x0, cond, t=t, noise=noise, keep=keep))
        assert torch.equal(d.generator.get_state(), state3)  # all three given: nothing drawn
        assert not torch.equal(got, d.loss(x0, cond, t=t, noise=noise, keep=~keep))
        # a given keep is not drawn again
        d.generator.manual_seed(sd)
        assert torch.equal(d.loss(x0, cond, keep=keep), got)
        assert torch.equal(d.generator.get_state(), state2)
        # eval(): nothing is drawn for the dropout and cond goes in whole
        d.eval()
        d.generator.manual_seed(sd)
        got_eval = d.loss(x0, cond)
        assert torch.equal(d.generator.get_state(), state2)
        d0 = product(nets, dev, T, cdt)  # p_uncond = 0: today's stream and today's result, in either mode
        for mode in (d0.train, d0.eval):
            mode()
            d0.generator = torch.Generator(device=dev).manual_seed(sd)
            got0 = d0.loss(x0, cond)
            assert torch.equal(d0.generator.get_state(), state2)
            assert torch.equal(got0, got_eval)
            assert torch.equal(got0, d0.loss(x0, cond, t=t, noise=noise))
        # the default generator is used when none is set
        d.train()
        d.generator = None
        seed(sd)
        assert torch.equal(d.loss(x0, cond), got)
    nets[1].train()  # the shared network as the other tests find it


@pytest.mark.parametrize("cdt", [torch.float32, torch.bfloat16])
def test_input_grads_of_a_dropped_sample_are_zero(dev, nets, cdt):
    x0, cond, t, noise = train_inputs(dev)
    d = product(nets, dev, 12, cdt)
    loss, dxt, dcond = input_grads(d, x0, cond, t=t, noise=noise, keep=[True, False])
    assert dcond.shape == cond.shape and dxt.shape == x0.shape
    assert bool((dcond[1] == 0).all()) and dcond[0].abs().max().item() > 0
    assert dxt[1].abs().max().item() > 0  # the state still matters to a dropped sample
    zeroed = cond.clone()
    zeroed[1] = 0
    l0, dxt0, dcond0 = input_grads(d, x0, zeroed, t=t, noise=noise)
    assert torch.equal(loss, l0) and torch.equal(dxt, dxt0) and torch.equal(dcond[0], dcond0[0])
    assert dcond0[1].abs().max().item() > 0  # without the mask the zeroed cond still has a gradient
    # loss.backward() with cond.requires_grad sees the same zero
    c = cond.clone().requires_grad_(True)
    d.loss(x0, c, t=t, noise=noise, keep=[True, False]).backward()
    assert bool((c.grad[1] == 0).all()) and c.grad[0].abs().max().item() > 0
    d.zero_grad(set_to_none=True)
    assert all(p.grad is None for p in d.parameters())
    from cesm_emulator_amd import saliency_wrt_cond
    sal = saliency_wrt_cond(d, x0, cond, t=t, noise=noise, keep=[True, False])
    assert bool((sal[1] == 0).all()) and sal[0].max().item() > 0
