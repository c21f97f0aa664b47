"""Few-step DDIM sampling on the GPU: cesm_ddim_step, Diffusion.ddim_step / sample(steps=, ddim_eta=) on the eager and
the HIP-graph path, counterfactual_delta.

* the update kernel vs the float64 expression a x + b eps + sigma z with Diffusion.ddim_coefs' coefficients.  Bound,
  elementwise: 8 * 2^-24 * (|a x| + |b eps| + |sigma z|) -- one rounding of each coefficient, one of each product and
  two additions give <= 4 * 2^-24 of that sum (contraction to FMA only lowers it), times 2 for margin.  Shapes: 17x29
  (odd, scalar path, two blocks per sample), 24x44 (16-byte path, two blocks per sample) and 24x44 from a pointer
  that is only 4-byte aligned (scalar path again);
* graph == eager bit for bit; eta = 0 draws no random number; steps=None is the ancestral loop whatever ddim_eta is;
* eta = 1 on the full grid against the ancestral sampler and few-step runs against a float64 loop around the CPU
  oracle network: relative L2 < 1e-4, the gate of test_gpu_sampler's oracle comparison for loops of this length.
"""
import pytest
import torch

from cesm_emulator_amd import counterfactual_delta, kernels as K
from cesm_emulator_amd._lib import KernelError, call
from cesm_emulator_amd.model import UNet, Diffusion, GraphSampleStep
from oracle import ref_cpu as R

pytestmark = pytest.mark.gpu

EPS24 = 2.0 ** -24
SHAPE = (2, 1, 16, 24)


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


def product(nets, dev, T, cdt):
    prod = nets[1]
    prod.compute_dtype = cdt
    return Diffusion(prod, timesteps=T).to(dev)


def make(dev, B, H, W, misalign, g):
    """[B,1,H,W] normal tensor; misalign: its storage starts one float past a 16-byte boundary"""
    n = B * H * W
    buf = torch.randn(n + 1, device=dev, generator=g)
    return buf[1:].view(B, 1, H, W) if misalign else buf[:n].view(B, 1, H, W)


def bound_and_ref(sched, x, eps, z, t, tp, eta):
    a, b, s = (c.view(-1, 1, 1, 1) for c in sched.ddim_coefs(t, tp, eta))
    xd, ed = x.double(), eps.double()
    ref = a * xd + b * ed
    mag = (a * xd).abs() + (b * ed).abs()
    if z is not None and eta > 0:
        ref = ref + s * z.double()
        mag = mag + (s * z.double()).abs()
    return ref, 8 * EPS24 * mag


LAYOUTS = [(17, 29, False), (24, 44, False), (24, 44, True)]
TIMES = [([999, 500, 1], [979, 0, -1]), ([0, 0, 0], [-1, -1, -1]), ([999, 7, 20], [0, -1, 19])]


@pytest.mark.parametrize("H,W,misalign", LAYOUTS)
def test_ddim_kernel_matches_float64_expression(dev, sched, H, W, misalign):
    g = torch.Generator(device=dev).manual_seed(3)
    B = 3
    x, eps, z = (make(dev, B, H, W, misalign, g) for _ in range(3))
    assert (x.data_ptr() % 16 != 0) == misalign
    ac = sched.alphas_cumprod
    for tv, tpv in TIMES:
        t, tp = torch.tensor(tv, device=dev), torch.tensor(tpv, device=dev)
        for eta in (0.0, 0.5, 1.0):
            for zz in (z, None):
                out = K.ddim_step(x, eps, zz, t, tp, ac, eta)
                ref, bound = bound_and_ref(sched, x, eps, zz, t, tp, eta)
                err = (out.double() - ref).abs()
                print(f"{H}x{W} misalign={misalign} t={tv} t_prev={tpv} eta={eta} z={zz is not None}: "
                      f"worst |err| / bound {(err / bound.clamp_min(1e-300)).max().item():.3f}")
                assert (err <= bound).all(), (tv, tpv, eta)
                # in place: bit for bit the out-of-place result
                xi = make(dev, B, H, W, misalign, g)
                xi.copy_(x)
                assert K.ddim_step(xi, eps, zz, t, tp, ac, eta, out=xi) is xi
                assert torch.equal(xi, out)


def test_ddim_kernel_noise_is_not_read_at_eta0(dev, sched):
    """eta = 0 drops the noise term without reading z: a z full of NaN changes nothing"""
    g = torch.Generator(device=dev).manual_seed(4)
    x, eps = (make(dev, 3, 17, 29, False, g) for _ in range(2))
    t, tp = torch.tensor([999, 500, 1], device=dev), torch.tensor([979, 0, -1], device=dev)
    nan = torch.full_like(x, float("nan"))
    assert torch.equal(K.ddim_step(x, eps, nan, t, tp, sched.alphas_cumprod, 0.0),
                       K.ddim_step(x, eps, None, t, tp, sched.alphas_cumprod, 0.0))


def test_ddim_kernel_argument_checks(dev, sched):
    x = torch.zeros(2, 1, 4, 4, device=dev)
    t, tp = torch.tensor([5, 5], device=dev), torch.tensor([3, 3], device=dev)
    ac = sched.alphas_cumprod
    st = torch.cuda.current_stream().cuda_stream
    for B, HW, T in ((0, 16, 1000), (2, 0, 1000), (2, 16, 0)):
        with pytest.raises(KernelError):
            call("cesm_ddim_step", x.data_ptr(), x.data_ptr(), 0, t.data_ptr(), tp.data_ptr(), ac.data_ptr(), 0.0,
                 x.data_ptr(), B, HW, T, st)
    with pytest.raises(ValueError):
        K.ddim_step(x, x, None, t, tp, ac, -1.0)
    with pytest.raises(RuntimeError):
        K.ddim_step(x, x, None, t[:1], tp, ac, 0.0)
    with pytest.raises(RuntimeError):
        K.ddim_step(x, x, None, t.int(), tp, ac, 0.0)


@pytest.mark.parametrize("tv", [999, 500, 0])
def test_ddim_kernel_recovers_x0(dev, sched, tv):
    """with the exact eps, one step t -> -1 at eta = 0 returns x0"""
    g = torch.Generator(device=dev).manual_seed(5)
    x0, eps = (make(dev, 3, 17, 29, False, g) for _ in range(2))
    t, tp = torch.full((3,), tv, device=dev), torch.full((3,), -1, device=dev)
    at = sched.alphas_cumprod[t].double().view(-1, 1, 1, 1)
    x_t = (at.sqrt() * x0.double() + (1 - at).sqrt() * eps.double()).float()
    out = K.ddim_step(x_t, eps, None, t, tp, sched.alphas_cumprod, 0.0)
    # x_t is rounded to fp32 once: the kernel's exact target is a x_t + b eps, which is x0 up to that rounding
    a, b, _ = (c.view(-1, 1, 1, 1) for c in sched.ddim_coefs(t, tp, 0.0))
    mag = (a * x_t.double()).abs() + (b * eps.double()).abs()
    err = (out.double() - x0.double()).abs()
    print(f"t={tv}: worst |out - x0| / bound {(err / (8 * EPS24 * mag)).max().item():.3f}")
    assert (err <= 8 * EPS24 * mag).all()


@pytest.mark.parametrize("eta", [0.0, 0.7])
@pytest.mark.parametrize("cdt", [torch.float32, torch.bfloat16])
def test_graph_equals_eager(dev, nets, cdt, eta):
    d = product(nets, dev, 12, cdt)
    g = torch.Generator(device=dev).manual_seed(2)
    cond = torch.randn(SHAPE, device=dev, generator=g)
    seed(7)
    y_eager = d.sample(cond, SHAPE, dev, use_graph=False, steps=5, ddim_eta=eta)
    seed(7)
    y_graph = d.sample(cond, SHAPE, dev, use_graph=True, steps=5, ddim_eta=eta)
    assert torch.isfinite(y_graph).all()
    assert torch.equal(y_graph, y_eager)


@pytest.mark.parametrize("eta", [0.0, 0.7])
def test_graph_equals_eager_window_cond(dev, nets, eta):
    d = product(nets, dev, 12, torch.bfloat16)
    g = torch.Generator(device=dev).manual_seed(2)
    cond = torch.randn(2, 1, 3, 16, 24, device=dev, generator=g)
    seed(7)
    y_eager = d.sample(cond, SHAPE, dev, use_graph=False, steps=5, ddim_eta=eta)
    seed(7)
    y_graph = d.sample(cond, SHAPE, dev, use_graph=True, steps=5, ddim_eta=eta)
    assert y_graph.shape == SHAPE and torch.isfinite(y_graph).all()
    assert torch.equal(y_graph, y_eager)


@pytest.mark.parametrize("use_graph", [False, True])
def test_eta0_draws_nothing(dev, nets, use_graph):
    d = product(nets, dev, 12, torch.bfloat16)
    g = torch.Generator(device=dev).manual_seed(2)
    cond = torch.randn(SHAPE, device=dev, generator=g)
    x_T = torch.randn(SHAPE, device=dev, generator=g)
    seed(1)
    before = torch.cuda.get_rng_state()
    y1 = d.sample(cond, SHAPE, dev, use_graph=use_graph, x_T=x_T, steps=5, ddim_eta=0.0)
    assert torch.equal(torch.cuda.get_rng_state(), before)
    seed(2)
    y2 = d.sample(cond, SHAPE, dev, use_graph=use_graph, x_T=x_T, steps=5, ddim_eta=0.0)
    assert torch.equal(y1, y2)


def test_graph_step_has_no_noise_buffer_at_eta0(dev, nets):
    d = product(nets, dev, 12, torch.bfloat16)
    x = torch.zeros(SHAPE, device=dev)
    step = GraphSampleStep(d, x, x.clone(), ddim_eta=0.0)
    assert step.z is None and step.t_prev is not None
    with pytest.raises(ValueError):
        step.run(5)
    with pytest.raises(ValueError):
        step.run(5, 5)


@pytest.mark.parametrize("use_graph", [False, True])
def test_full_grid_eta1_is_ddpm(dev, nets, use_graph):
    T = 6
    d = product(nets, dev, T, torch.float32)
    g = torch.Generator(device=dev).manual_seed(11)
    cond = torch.randn(SHAPE, device=dev, generator=g)
    x_T = torch.randn(SHAPE, device=dev, generator=g)
    noise_seq = torch.randn(T, *SHAPE, device=dev, generator=g)
    y_ddpm = d.sample(cond, SHAPE, dev, use_graph=use_graph, x_T=x_T, noise_seq=noise_seq)
    y_ddim = d.sample(cond, SHAPE, dev, use_graph=use_graph, x_T=x_T, noise_seq=noise_seq, steps=T, ddim_eta=1.0)
    err = rel(y_ddim, y_ddpm)
    print(f"steps = T, eta = 1 vs the ancestral sampler (graph={use_graph}): rel {err:.3e}")
    assert err < 1e-4


@pytest.fixture(scope="module")
def oracle_runs(nets):
    """steps = 4 of T = 12 with the CPU oracle network's eps and the update of Diffusion.ddim_coefs in float64"""
    ref = nets[0]
    T, steps = 12, 4
    d = Diffusion(torch.nn.Identity(), timesteps=T)
    g = torch.Generator().manual_seed(11)
    cond = torch.randn(SHAPE, generator=g)
    x_T = torch.randn(SHAPE, generator=g)
    noise_seq = torch.randn(steps, *SHAPE, generator=g)
    tau = d.sample_schedule(steps)
    assert tau == [0, 4, 7, 11]
    out = {}
    with torch.no_grad():
        for eta in (0.0, 0.5):
            x = x_T.double()
            for k, (tt, tp) in enumerate(zip(reversed(tau), reversed([-1] + tau[:-1]))):
                eps = ref(x.float(), cond, torch.full((SHAPE[0],), tt, dtype=torch.long)).double()
                a, b, s = d.ddim_coefs(tt, tp, eta)
                x = a * x + b * eps + s * noise_seq[k].double()
            out[eta] = x
    return cond, x_T, noise_seq, out


@pytest.mark.parametrize("use_graph", [False, True])
@pytest.mark.parametrize("eta", [0.0, 0.5])
def test_few_steps_match_oracle_loop_fp32(dev, nets, oracle_runs, eta, use_graph):
    cond, x_T, noise_seq, want = oracle_runs
    d = product(nets, dev, 12, torch.float32)
    y = d.sample(cond.to(dev), SHAPE, dev, use_graph=use_graph, x_T=x_T, noise_seq=noise_seq.to(dev), steps=4,
                 ddim_eta=eta)
    err = rel(y, want[eta])
    print(f"steps=4 eta={eta} fp32 vs the oracle loop (graph={use_graph}): rel {err:.3e}")
    assert err < 1e-4


@pytest.mark.parametrize("use_graph", [False, True])
def test_steps_none_is_untouched(dev, nets, use_graph):
    T = 6
    d = product(nets, dev, T, torch.bfloat16)
    g = torch.Generator(device=dev).manual_seed(12)
    cond = torch.randn(SHAPE, device=dev, generator=g)
    x_T = torch.randn(SHAPE, device=dev, generator=g)
    noise_seq = torch.randn(T, *SHAPE, device=dev, generator=g)
    y0 = d.sample(cond, SHAPE, dev, use_graph=use_graph, x_T=x_T, noise_seq=noise_seq)
    y1 = d.sample(cond, SHAPE, dev, use_graph=use_graph, x_T=x_T, noise_seq=noise_seq, steps=None, ddim_eta=0.3)
    assert torch.equal(y0, y1)
    # and with its own draws: same seeds, same result
    seed(3)
    y2 = d.sample(cond, SHAPE, dev, use_graph=use_graph)
    seed(3)
    y3 = d.sample(cond, SHAPE, dev, use_graph=use_graph, steps=None, ddim_eta=0.3)
    assert torch.equal(y2, y3)


def test_sample_argument_checks(dev, nets):
    d = product(nets, dev, 12, torch.bfloat16)
    cond = torch.zeros(SHAPE, device=dev)
    for steps in (0, 13):
        with pytest.raises(ValueError):
            d.sample(cond, SHAPE, dev, steps=steps)
    with pytest.raises(ValueError):
        d.sample(cond, SHAPE, dev, steps=4, ddim_eta=-0.5)
    x = torch.zeros(SHAPE, device=dev)
    with pytest.raises(ValueError):
        d.ddim_step(x, cond, torch.tensor([5, 5], device=dev), torch.tensor([5, 3], device=dev))
    with pytest.raises(ValueError):
        d.ddim_step(x, cond, torch.tensor([12, 5], device=dev), torch.tensor([3, 3], device=dev))


def test_counterfactual_delta(dev, nets):
    d = product(nets, dev, 12, torch.float32)
    g = torch.Generator(device=dev).manual_seed(13)
    cond = torch.randn(SHAPE, device=dev, generator=g)
    mask = (torch.rand(SHAPE, device=dev, generator=g) > 0.5).float()
    kw = dict(steps=4, ddim_eta=0.5)
    for m in (None, mask):
        cond2 = cond * 1.1 if m is None else cond * (1 + (1.1 - 1) * m)
        seed(5)
        delta = counterfactual_delta(d, cond, scale_mask=m, scale=1.1, **kw)
        seed(5)
        base = d.sample(cond, SHAPE, dev, **kw)
        pert = d.sample(cond2, SHAPE, dev, **kw)
        assert torch.equal(delta, pert - base)
    # paired: both halves share x_T and the step noise, so an unchanged cond gives (numerically) no difference
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
        finally:
            mp.undo()
        assert same.shape == SHAPE and diff.shape == SHAPE
        print(f"paired (graph={use_graph}), scale = 1: max |delta| {same.abs().max().item():.3e} "
              f"(exactly zero: {bool((same == 0).all())}), max |base| {base.abs().max().item():.3e}; "
              f"scale = 1.1: max |delta| {diff.abs().max().item():.3e}")
        assert same.abs().max().item() <= 1e-4 * base.abs().max().item()
        assert torch.isfinite(diff).all() and diff.abs().max().item() > 0
    # the full ancestral loop (steps=None) pairs too
    seed(6)
    same = counterfactual_delta(d, cond, scale=1.0, paired=True)
    assert same.abs().max().item() <= 1e-4 * base.abs().max().item()
