"""EMA of the weights, fused into the AdamW launch (csrc/misc.hip cesm_adamw_ema, cesm_emulator_amd/ema.py).

Kernel level: the EMA recurrence exactly on integer data (a), p / g / m / v / step bit-identical to the plain step
(b), a skipped step changes nothing (c), the warm-up schedule against a float64 oracle within a derived bound (d).
Model level: ema_model serves the current average and not a stale weight pack (e), attaching an EMA does not
change training (f), checkpoints carry it (g).
"""
import pytest
import torch

from cesm_emulator_amd import checkpoint as CK
from cesm_emulator_amd import kernels as K
from cesm_emulator_amd.ema import EMA, ema_decay
from cesm_emulator_amd.model import UNet, Diffusion
from cesm_emulator_amd.optim import FusedAdamW
from cesm_emulator_amd.train import make_ema, train_one_epoch, train_step

pytestmark = pytest.mark.gpu

SWEEP = 8192 * 256  # threads of the capped grid: one sweep of the scalar kernel
SIZES = [1, 255, 256, 4099, SWEEP + 77]
GUARD = 12345.0


def _sub(host, lead, dev):
    """device copy of `host` inside a larger buffer, `lead` floats past its (256-byte aligned) start, with guard
    values on both sides; returns (buffer, view)"""
    n = host.numel()
    buf = torch.full((lead + n + 8,), GUARD, dtype=host.dtype, device=dev)
    buf[lead:lead + n].copy_(host)
    return buf, buf[lead:lead + n]


def _guards_intact(buf, lead, n):
    return bool((buf[:lead] == GUARD).all()) and bool((buf[lead + n:] == GUARD).all())


def _counters(dev, step=0, n=0):
    return (torch.full((1,), step, dtype=torch.int32, device=dev), torch.full((1,), n, dtype=torch.int32, device=dev),
            torch.full((1,), float("nan"), dtype=torch.float32, device=dev))


# ------------------------------------------------------------------------------------------ a: exact recurrence
@pytest.mark.parametrize("lead", [0, 1, "ema"], ids=["aligned", "plus4bytes", "ema_plus4bytes"])
@pytest.mark.parametrize("beta", [0.5, 0.75])
@pytest.mark.parametrize("n", SIZES)
def test_ema_recurrence_exact_on_integers(dev, n, beta, lead):
    """lr = 0, g = m = v = 0: p must come back bit-equal and e follow e + (1 - beta)(p - e) exactly (every
    intermediate is a small multiple of 2^-6: exact in fp32, with or without FMA contraction).  lead = 1 puts every
    buffer 4 bytes past a 16-byte boundary, "ema" only the EMA buffer: a vectorised kernel has to notice both."""
    g = torch.Generator().manual_seed(n + int(beta * 100))
    p0 = torch.randint(-64, 65, (n,), generator=g).float()
    e0 = torch.randint(-64, 65, (n,), generator=g).float()
    l_all = 1 if lead == 1 else 0
    l_ema = 1 if lead in (1, "ema") else 0
    zeros = torch.zeros(n)
    (pb, p), (gb, gr), (mb, m), (vb, v) = (_sub(t, l_all, dev) for t in (p0, zeros, zeros, zeros))
    eb, e = _sub(e0, l_ema, dev)
    assert p.data_ptr() % 16 == 4 * l_all and e.data_ptr() % 16 == 4 * l_ema
    step, ema_n, omd = _counters(dev)
    ref = e0.double()
    for k in range(1, 4):
        info = K.grad_norm(gr, 0.0)
        K.adamw_ema(p, gr, m, v, info, 0.0, 0.9, 0.999, 1e-8, 0.0, step, False, e, ema_n, omd, beta, 0)
        ref = ref + (1.0 - beta) * (p0.double() - ref)
        assert torch.equal(p.cpu(), p0), f"p changed at step {k}"
        assert torch.equal(e.cpu().double(), ref), f"e differs from the float64 recurrence at step {k}"
    assert torch.equal(ref.float().double(), ref)  # the reference itself is exact in fp32
    assert int(step.item()) == 3 and int(ema_n.item()) == 3 and float(omd.item()) == 1.0 - beta
    assert not m.any() and not v.any() and not gr.any()
    for buf, ld in ((pb, l_all), (gb, l_all), (mb, l_all), (vb, l_all), (eb, l_ema)):
        assert _guards_intact(buf, ld, n), "write outside the buffer"


# ------------------------------------------------------------------------------------------ b: the step is unchanged
@pytest.mark.parametrize("lead", [0, 1], ids=["aligned", "plus4bytes"])  # the 128-bit and the scalar kernel
@pytest.mark.parametrize("use_clip", [False, True])
def test_step_bit_identical_to_plain_adamw(dev, use_clip, lead):
    n = SWEEP + 77
    g = torch.Generator().manual_seed(5)
    host = [torch.randn(n, generator=g), torch.randn(n, generator=g), 0.1 * torch.randn(n, generator=g),
            0.01 * torch.rand(n, generator=g)]
    a = [t.to(dev) for t in host]
    b = [_sub(t, lead, dev)[1] for t in host]
    e = _sub(torch.randn(n, generator=g), lead, dev)[1]
    assert b[0].data_ptr() % 16 == 4 * lead
    step_a, _, _ = _counters(dev, step=4)
    step_b, ema_n, omd = _counters(dev, step=4)
    hp = (2e-3, 0.9, 0.999, 1e-8, 1e-2)
    for k in range(2):
        info_a = K.grad_norm(a[1], 1.0 if use_clip else 0.0)
        info_b = K.grad_norm(b[1], 1.0 if use_clip else 0.0)
        K.adamw(*a, info_a, *hp, step_a, use_clip)
        K.adamw_ema(*b, info_b, *hp, step_b, use_clip, e, ema_n, omd, 0.999, 1)
        for name, x, y in zip("pgmv", a, b):
            assert torch.equal(x, y), f"{name} differs from the plain step at step {k + 1}"
        assert torch.equal(info_a, info_b) and torch.equal(step_a, step_b)
        assert not torch.equal(a[0], host[0].to(dev))  # a real step
    assert int(step_b.item()) == 6 and int(ema_n.item()) == 2


# ------------------------------------------------------------------------------------------ c: skipped step
def test_skipped_step_changes_nothing(dev):
    n = 4099
    g = torch.Generator().manual_seed(6)
    p, gr, m, v, e = (torch.randn(n, generator=g).to(dev) for _ in range(5))
    v.abs_()
    step, ema_n, omd = _counters(dev)
    hp = (1e-2, 0.9, 0.999, 1e-8, 1e-2)
    K.adamw_ema(p, gr, m, v, K.grad_norm(gr, 1.0), *hp, step, True, e, ema_n, omd, 0.9, 1)  # one applied step first
    before = [t.clone() for t in (p, gr, m, v, e, step, ema_n)]
    assert int(step.item()) == 1 and int(ema_n.item()) == 1
    info = K.grad_norm(gr, 1.0, torch.full((1,), float("nan"), device=dev))
    assert float(info[2].item()) == 0.0
    K.adamw_ema(p, gr, m, v, info, *hp, step, True, e, ema_n, omd, 0.9, 1)
    for name, x, y in zip(("p", "g", "m", "v", "e", "step", "ema_n"), before, (p, gr, m, v, e, step, ema_n)):
        assert torch.equal(x, y), f"{name} changed in a skipped step"


# ------------------------------------------------------------------------------------------ shared small model
SHAPE = (2, 1, 16, 24)
T_SAMPLE = 4


def _setup(dev, cdt, seed=1, lr=1e-2):
    torch.manual_seed(seed)
    net = UNet(ch_mults=(1, 2, 4)).to(dev)
    net.compute_dtype = cdt
    d = Diffusion(net, timesteps=T_SAMPLE).to(dev)
    opt = FusedAdamW(d.parameters(), lr=lr, weight_decay=1e-4, max_grad_norm=1.0)
    return net, d, opt


def _batch(dev, seed=0):
    g = torch.Generator().manual_seed(seed)
    x0 = torch.randn(*SHAPE, generator=g).to(dev)
    cond = torch.randn(2, 1, 2, 16, 24, generator=g).to(dev)
    t = torch.tensor([1, 3], device=dev)
    noise = torch.randn(*SHAPE, generator=g).to(dev)
    return x0, cond, t, noise


# ------------------------------------------------------------------------------------------ d: warm-up schedule
def test_warmup_schedule_against_float64_oracle(dev):
    """K = 8 real steps, beta = 0.999 with warm-up; after each the parameters are read back and a float64 oracle
    advanced: e <- e + float64(float32(1 - ema_decay(n))) (p - e).

    Bound: |e_gpu - e_ref| <= 5 K 2^-24 A elementwise, A = max(|p|, |e|) over the run (here taken per element, which
    is the tighter reading).  Derived, not measured: each step has at most three fp32 roundings (subtract, multiply,
    add) acting on magnitudes <= 2A, 2A and A, i.e. <= 5 * 2^-24 A of new error, and the previous error is carried
    with weight decay <= 1."""
    steps, beta = 8, 0.999
    net, d, opt = _setup(dev, torch.float32)
    opt.max_grad_norm = None
    ema = EMA(net, opt, beta=beta, warmup=True)
    # start the average away from the weights, so that every blend moves it (padding stays zero)
    ema.flat.mul_(torch.empty_like(ema.flat).uniform_(-2.0, 2.0))
    ref = ema.flat.double().cpu()
    amax = ref.abs()
    for k in range(1, steps + 1):
        opt.zero_grad()
        for q in opt.flat.params:
            q.grad.normal_()
        opt.step()
        ema.update()  # the reference loop's call: a no-op
        p = opt.flat.data.double().cpu()
        omd = float(torch.tensor(1.0 - ema_decay(k, beta), dtype=torch.float32).item())
        assert omd == float(ema._omd_dev.item()), f"step {k}: the device blends with another factor"
        amax = torch.maximum(amax, torch.maximum(p.abs(), ref.abs()))
        ref = ref + omd * (p - ref)
        got = ema.flat.double().cpu()
        amax = torch.maximum(amax, torch.maximum(ref.abs(), got.abs()))
        err, bound = (got - ref).abs(), 5.0 * k * 2.0 ** -24 * amax
        print(f"step {k}: max err / bound = {(err / bound.clamp_min(1e-300)).max().item():.3f}")
        assert bool((err <= bound).all()), f"step {k}: max excess {(err - bound).max().item():.3e}"
    assert ema.num_updates == steps and opt.step_count == steps
    assert not torch.equal(ema.flat, opt.flat.data)
    used = torch.zeros_like(ema.flat, dtype=torch.bool)
    for q, off in zip(opt.flat.params, opt.flat.offsets):
        used[off:off + q.numel()] = True
    assert not ema.flat[~used].any(), "padding of the EMA buffer must stay zero"


# ------------------------------------------------------------------------------------------ e: fresh weights served
@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("cdt", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_ema_model_serves_fresh_weights(dev, cdt, use_graph):
    net, d, opt = _setup(dev, cdt)
    ema = EMA(net, opt, beta=0.5, warmup=False)
    assert opt.ema is ema and not ema.ema_model.training and ema.ema_model.compute_dtype == cdt
    assert list(ema.ema_model.state_dict()) == list(net.state_dict())
    x0, cond5, t, noise = _batch(dev)
    g = torch.Generator().manual_seed(11)
    cond = torch.randn(*SHAPE, generator=g).to(dev)
    x_T = torch.randn(*SHAPE, generator=g).to(dev)
    nz = torch.randn(T_SAMPLE, *SHAPE, generator=g).to(dev)

    def sample():
        return d.sample(cond, SHAPE, dev, use_graph=use_graph, x_T=x_T, noise_seq=nz).clone()

    with ema.applied(d) as dd:
        assert dd is d and d.model is ema.ema_model
        s0 = sample()  # fills ema_model's pack cache with the initial weights
    assert d.model is net
    for _ in range(2):
        train_step(d, opt, x0, cond5, 1.0, t=t, noise=noise)
    with ema.applied(d):
        s1 = sample()
    assert d.model is net and ema.num_updates == 2
    raw = sample()
    torch.manual_seed(99)
    fresh = UNet(ch_mults=(1, 2, 4)).to(dev)
    fresh.load_state_dict(ema.ema_model.state_dict())
    fresh.compute_dtype = cdt
    fresh.eval()
    d.model = fresh
    want = sample()
    d.model = net
    assert torch.isfinite(s1).all()
    assert torch.equal(s1, want), "ema_model sampled from something else than its current weights (stale pack?)"
    assert not torch.equal(s1, s0) and not torch.equal(s1, raw)
    with pytest.raises(RuntimeError, match="boom"):
        with ema.applied(d):
            assert d.model is ema.ema_model
            raise RuntimeError("boom")
    assert d.model is net
    ema.detach()
    assert opt.ema is None


def test_ema_model_works_for_steps_and_input_grads(dev):
    """ema_model as diffusion.model for p_sample, ddim_step, few-step sampling and input_grads; all equal to a
    freshly built UNet holding the same weights"""
    from cesm_emulator_amd import input_grads
    net, d, opt = _setup(dev, torch.float32)
    ema = EMA(net, opt, beta=0.5, warmup=False)
    x0, cond5, t, noise = _batch(dev)
    train_step(d, opt, x0, cond5, 1.0, t=t, noise=noise)
    fresh = UNet(ch_mults=(1, 2, 4)).to(dev)
    fresh.load_state_dict(ema.ema_model.state_dict())
    fresh.compute_dtype = torch.float32
    fresh.eval()
    for q in fresh.parameters():
        q.requires_grad_(False)
    cond = cond5[:, :, 0].contiguous()

    def everything():
        return (d.p_sample(x0, cond, t, noise=noise), d.ddim_step(x0, cond, t, t - 1, eta=0.0),
                d.sample(cond, SHAPE, dev, use_graph=False, x_T=x0, steps=2),
                *input_grads(d, x0, cond5, t=t, noise=noise))

    with ema.applied(d):
        got = everything()
    d.model = fresh
    want = everything()
    d.model = net
    assert len(got) == len(want) >= 5
    for i, (a, b) in enumerate(zip(got, want)):
        assert torch.equal(a, b), i
    assert all(q.grad is None for q in ema.ema_model.parameters())


# ------------------------------------------------------------------------------------------ f: training unchanged
def test_attached_ema_does_not_change_training(dev):
    x0, cond5, t, noise = _batch(dev)

    def run(with_ema):
        net, d, opt = _setup(dev, torch.bfloat16, seed=3)
        ema = EMA(net, opt, beta=0.9, warmup=True) if with_ema else None
        losses = [train_step(d, opt, x0, cond5, 1.0, t=t, noise=noise).clone() for _ in range(3)]
        return opt, ema, losses

    opt_a, _, loss_a = run(False)
    opt_b, ema, loss_b = run(True)
    assert torch.equal(opt_a.flat.data, opt_b.flat.data)
    assert torch.equal(opt_a.exp_avg, opt_b.exp_avg) and torch.equal(opt_a.exp_avg_sq, opt_b.exp_avg_sq)
    assert all(torch.equal(x, y) for x, y in zip(loss_a, loss_b))
    assert opt_a.step_count == opt_b.step_count == 3 and ema.num_updates == 3
    assert all(q.grad is None and not q.requires_grad for q in ema.ema_model.parameters())
    assert not torch.equal(ema.flat, opt_b.flat.data)


def test_ema_argument_checks_on_device(dev):
    net, d, opt = _setup(dev, torch.float32)
    other = UNet(ch_mults=(1, 2, 4)).to(dev)
    with pytest.raises(ValueError, match="trainable parameters"):
        EMA(other, opt)
    assert opt.ema is None
    ema = make_ema(d, opt, {"ema": {"beta": 0.99, "warmup": False}})
    assert isinstance(ema, EMA) and ema.beta == 0.99 and ema.warmup is False and opt.ema is ema
    with pytest.raises(RuntimeError, match="already"):
        EMA(net, opt)
    ema.detach()
    with pytest.raises(ValueError, match="not attached"):
        train_one_epoch(d, [], opt, dev, ema=ema)
    n = 8
    bufs = [torch.zeros(n, device=dev) for _ in range(5)]
    step, ema_n, omd = _counters(dev)
    info = K.grad_norm(bufs[1], 0.0)
    with pytest.raises(RuntimeError, match="shape"):
        K.adamw_ema(*bufs[:4], info, 0.0, 0.9, 0.999, 1e-8, 0.0, step, False, bufs[4][:4], ema_n, omd, 0.5, 0)
    with pytest.raises(RuntimeError, match="dtype"):
        K.adamw_ema(*bufs[:4], info, 0.0, 0.9, 0.999, 1e-8, 0.0, step, False, bufs[4], ema_n.float(), omd, 0.5, 0)
    with pytest.raises(ValueError, match="beta"):
        K.adamw_ema(*bufs[:4], info, 0.0, 0.9, 0.999, 1e-8, 0.0, step, False, bufs[4], ema_n, omd, 1.0, 0)


# ------------------------------------------------------------------------------------------ g: checkpoints
CFG = {"unet": {"in_channels": 2, "out_channels": 1, "base_ch": 64, "ch_mults": [1, 2, 4], "groups": 8},
       "train": {"timesteps": T_SAMPLE, "beta_schedule": "linear"}}


def test_checkpoint_round_trip_with_ema(dev, tmp_path, capsys):
    net, d, opt = _setup(dev, torch.float32)
    ema = EMA(net, opt, beta=0.75, warmup=False)
    x0, cond5, t, noise = _batch(dev)
    for _ in range(2):
        train_step(d, opt, x0, cond5, 1.0, t=t, noise=noise)
    with_ema, without = tmp_path / "with.pt", tmp_path / "without.pt"
    CK.save_checkpoint(with_ema, d, opt, 3, CFG, ema=ema)
    CK.save_checkpoint(without, d, opt, 3, CFG)
    ck = torch.load(with_ema, weights_only=True)
    assert set(ck) == {"epoch", "model", "diffusion_buffers", "optimizer", "config", "ema"}
    assert set(ck["ema"]) == {"model", "beta", "warmup", "num_updates"}
    assert set(torch.load(without, weights_only=True)) == set(ck) - {"ema"}

    net2, d2, opt2 = _setup(dev, torch.float32, seed=77)
    ema2 = EMA(net2, opt2)  # other defaults: everything must come from the file
    assert CK.load_checkpoint(with_ema, net2, d2, opt2, device=dev, ema=ema2) == 4
    assert torch.equal(ema2.flat, ema.flat) and torch.equal(opt2.flat.data, opt.flat.data)
    assert (ema2.num_updates, ema2.beta, ema2.warmup) == (2, 0.75, False)
    for (k, a), (k2, b) in zip(ema.ema_model.state_dict().items(), ema2.ema_model.state_dict().items()):
        assert k == k2 and torch.equal(a, b), k

    d_ema, cfg = CK.load_diffusion_from_checkpoint(with_ema, device=dev, use_ema=True)
    d_raw, _ = CK.load_diffusion_from_checkpoint(with_ema, device=dev)
    assert cfg == CFG and not d_ema.training and not any(q.requires_grad for q in d_ema.parameters())
    want_ema, want_raw = ema.ema_model.state_dict(), net.state_dict()
    assert list(d_ema.model.state_dict()) == list(want_ema) == list(want_raw)
    for k, a in d_ema.model.state_dict().items():
        assert torch.equal(a, want_ema[k]), k
    for k, a in d_raw.model.state_dict().items():
        assert torch.equal(a, want_raw[k]), k
    assert any(not torch.equal(want_ema[k], want_raw[k]) for k in want_raw)
    with pytest.raises(KeyError, match="without.pt"):
        CK.load_diffusion_from_checkpoint(without, device=dev, use_ema=True)

    # the original and the restored pair continue identically
    for o in (opt, opt2):
        o.zero_grad()
        for q in o.flat.params:
            q.grad.fill_(0.25)
        o.step()
    assert torch.equal(ema2.flat, ema.flat) and torch.equal(opt2.flat.data, opt.flat.data)
    assert ema2.num_updates == 3

    # a checkpoint without the key: the EMA starts over from the loaded weights, and the loader says so
    capsys.readouterr()
    CK.load_checkpoint(without, net2, d2, opt2, device=dev, ema=ema2)
    assert "re-initialised" in capsys.readouterr().out
    assert ema2.num_updates == 0 and torch.equal(ema2.flat, opt2.flat.data)
    bad = ema.state_dict()
    bad["model"].pop(next(iter(bad["model"])))
    with pytest.raises(KeyError):
        ema2.load_state_dict(bad)
    bad = ema.state_dict()
    k0 = next(iter(bad["model"]))
    bad["model"][k0] = bad["model"][k0][..., :1]
    with pytest.raises(ValueError, match="shape"):
        ema2.load_state_dict(bad)
