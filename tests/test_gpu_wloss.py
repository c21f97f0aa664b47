"""Weighted loss on the GPU (csrc/misc.hip cesm_wloss / cesm_wloss_bwd, Diffusion.loss_components, the loaders' row
offsets and the training loop's metric logger).

Every expected value is computed here, in float64 on the CPU, from the formulas of the kernel's contract:
  c(b, h) = (1 - lam) + lam w[row0[b] + h],  mse_raw = mean d^2,  mse_lat = mean w d^2,  total = mean a c d^2,
  dpred = gscale (2 / n) a c d,  d = pred - noise.
Every tensor the wrappers allocate starts as NaN (the `poisoned` fixture), so an element a kernel leaves out shows."""
import numpy as np
import pytest
import torch

from cesm_emulator_amd import data as DA
from cesm_emulator_amd import kernels as K
from cesm_emulator_amd.model import UNet, Diffusion
from cesm_emulator_amd.optim import FusedAdamW
from cesm_emulator_amd.train import rank_generator, train_one_epoch, train_step

pytestmark = pytest.mark.gpu

F32_THIRD = float(torch.tensor(1.0 / 3.0, dtype=torch.float32))


@pytest.fixture(autouse=True)
def poisoned(monkeypatch):
    def empty(shape, dtype, device):
        t = torch.empty(shape, dtype=dtype, device=device)
        return t.fill_(float("nan")) if t.is_floating_point() else t
    monkeypatch.setattr(K, "empty", empty)


def ref64(pred, noise, w, row0, a, lam, gscale=1.0):
    """(out [3], dpred) in float64 on the CPU; row0 / a None as in the kernel"""
    B, V, H, W = pred.shape
    d = pred.double() - noise.double()
    r0 = [0] * B if row0 is None else [int(v) for v in row0]
    wr = torch.stack([w.double()[r:r + H] for r in r0]).view(B, 1, H, 1)
    assert wr.shape[2] == H, "row window leaves the grid"
    av = torch.ones(B, dtype=torch.float64) if a is None else a.double()
    c = (1.0 - lam) + lam * wr
    ac = av.view(B, 1, 1, 1) * c
    n = d.numel()
    out = torch.stack([(d * d).sum(), (wr * d * d).sum(), (ac * d * d).sum()]) / n
    return out, gscale * (2.0 / n) * ac * d


def exact_case(shape, Hg_extra, seed):
    """integer pred / noise with |d| <= 8, w multiples of 1/4 in [0, 2], a in {1/4, 1/2, 1}, random in-range row0"""
    B, V, H, W = shape
    g = torch.Generator().manual_seed(seed)
    pred = torch.randint(-4, 5, shape, generator=g).float()
    noise = torch.randint(-4, 5, shape, generator=g).float()
    w = torch.randint(0, 9, (H + Hg_extra,), generator=g).float() / 4
    row0 = torch.randint(0, Hg_extra + 1, (B,), generator=g)
    a = torch.tensor([0.25, 0.5, 1.0])[torch.randint(0, 3, (B,), generator=g)]
    return pred, noise, w, row0, a


def lead_view(host, lead, dev):
    """device copy of `host` that starts `lead` floats past a 256-byte aligned address"""
    buf = torch.zeros(host.numel() + lead, dtype=host.dtype, device=dev)
    v = buf[lead:].view(host.shape)
    v.copy_(host)
    assert v.data_ptr() % 16 == (4 * lead) % 16 and v.is_contiguous()
    return v


# ------------------------------------------------------------------------------------------ 1: exact data
# [4,1,192,288]: 768 rows of 72 16-byte accesses; [16,1,192,288] is added because the row loop of the kernels (three
# rows per block at this width, at most 512 blocks) iterates only from 1536 rows on
FWD_SHAPES = [(2, 2, 4, 8), (2, 1, 8, 64), (3, 2, 5, 7), (4, 1, 192, 288), (16, 1, 192, 288), (1, 1, 2, 1100),
              (2, 1, 3, 1030)]
LEADS = {(2, 1, 8, 64): (0, 1), (2, 2, 4, 8): (0, 2)}  # 4 / 8 bytes off a 16-byte boundary: the scalar path, W % 4 == 0


@pytest.mark.parametrize("shape", FWD_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_exact_on_integer_data(dev, shape):
    """Bit for bit.  With lam = 1/2 every coefficient a c is a multiple of 1/32 in [1/8, 3/2] and every term a c d^2 a
    multiple of 1/32 that is at most 96, so a partial sum over m elements is exact in fp32 while 96 * 32 * m < 2^24,
    m <= 5461; a block of the kernel adds at most 6 rows of 288 (or one of 1100) here, and the final sum is in double.
    The three scalars must equal float32(float64 sum / n).  dpred is exact where n is a power of two (2 g / n then is),
    for gscale 1 and 1/2; elsewhere each element is within 1e-6 relative of the float64 value: at most 8 fp32
    roundings of 2^-24 each on the chain 2 g / n * a * c * d make 4.8e-7."""
    lam = 0.5
    B, V, H, W = shape
    n = B * V * H * W
    pred, noise, w, row0, a = exact_case(shape, 3, seed=n)
    for lead in LEADS.get(shape, (0,)):
        p, q = lead_view(pred, lead, dev), lead_view(noise, lead, dev)
        args = (p, q, w.to(dev), row0.to(dev), a.to(dev), lam)
        want, _ = ref64(pred, noise, w, row0, a, lam)
        units = want * n * 32  # the three sums in units of 1/32: whole numbers (up to the division's rounding)
        assert float((units - units.round()).abs().max()) < 1e-3 and float(units.max()) < 2.0 ** 50
        got = K.wloss(*args).cpu()
        print(shape, lead, got.tolist(), want.tolist())
        assert torch.equal(got, want.float()), (got.tolist(), want.tolist())
        assert len({float(v) for v in got}) == 3  # the three sums are three different numbers
        for gs in (1.0, 0.5):
            _, dwant = ref64(pred, noise, w, row0, a, lam, gs)
            dgot = K.wloss_bwd(*args, torch.tensor([gs], device=dev)).cpu()
            assert dgot.shape == pred.shape and dgot.dtype == torch.float32
            if n & (n - 1) == 0:
                assert torch.equal(dgot.double(), dwant), f"dpred not exact, gscale {gs}"
            else:
                err = (dgot.double() - dwant).abs()
                worst = float((err / dwant.abs()).nan_to_num().max())
                assert bool((err <= 1e-6 * dwant.abs()).all()), f"gscale {gs}: max rel {worst:.2e}"
            assert bool((dgot != 0).any())


# ------------------------------------------------------------------------------------------ 2: null arguments
@pytest.mark.parametrize("shape", [(2, 1, 8, 64), (3, 2, 5, 7)], ids=["vector", "scalar"])
def test_null_arguments(dev, shape):
    B, V, H, W = shape
    g = torch.Generator().manual_seed(3)
    pred, noise = torch.randn(shape, generator=g).to(dev), torch.randn(shape, generator=g).to(dev)
    w = (2 * torch.rand(H + 2, generator=g)).to(dev)
    row0 = torch.tensor([2, 0, 1][:B], device=dev)
    a = torch.rand(B, generator=g).to(dev)
    one = torch.ones(1, device=dev)
    ones, zeros = torch.ones(B, device=dev), torch.zeros(B, dtype=torch.int64, device=dev)
    assert torch.equal(K.wloss(pred, noise, w, row0, None, 0.5), K.wloss(pred, noise, w, row0, ones, 0.5))
    assert torch.equal(K.wloss_bwd(pred, noise, w, row0, None, 0.5, one),
                       K.wloss_bwd(pred, noise, w, row0, ones, 0.5, one))
    assert torch.equal(K.wloss(pred, noise, w, None, a, 0.5), K.wloss(pred, noise, w, zeros, a, 0.5))
    assert torch.equal(K.wloss_bwd(pred, noise, w, None, a, 0.5, one),
                       K.wloss_bwd(pred, noise, w, zeros, a, 0.5, one))
    assert not torch.equal(K.wloss(pred, noise, w, None, a, 0.5), K.wloss(pred, noise, w, row0, a, 0.5))
    out = K.wloss(pred, noise, w, row0, None, 0.0).cpu()
    assert out[2] == out[0] and out[1] != out[0]  # lam = 0 and no a: total is mse_raw, bit for bit
    want, _ = ref64(pred.cpu(), noise.cpu(), w.cpu(), row0.cpu(), None, 0.0)
    assert torch.allclose(out.double(), want, rtol=1e-6, atol=0.0)


def test_wrapper_argument_checks(dev):
    pred, noise = torch.zeros(2, 1, 4, 8, device=dev), torch.zeros(2, 1, 4, 8, device=dev)
    w = torch.ones(4, device=dev)
    with pytest.raises(RuntimeError, match="shape"):
        K.wloss(pred, noise[:, :, :2].contiguous(), w, None, None, 0.5)
    with pytest.raises(RuntimeError, match="shape"):
        K.wloss(pred, noise, w[:3].contiguous(), None, None, 0.5)
    with pytest.raises(RuntimeError, match="shape"):
        K.wloss(pred, noise, w, torch.zeros(3, dtype=torch.int64, device=dev), None, 0.5)
    with pytest.raises(RuntimeError, match="dtype"):
        K.wloss(pred, noise, w, torch.zeros(2, dtype=torch.int32, device=dev), None, 0.5)
    with pytest.raises(RuntimeError, match="dtype"):
        K.wloss(pred, noise, w, None, torch.ones(2, dtype=torch.float64, device=dev), 0.5)
    with pytest.raises(RuntimeError, match="contiguous"):
        K.wloss(pred.transpose(2, 3), noise, w, None, None, 0.5)
    with pytest.raises(RuntimeError, match="device"):
        K.wloss(pred, noise, w.cpu(), None, None, 0.5)
    with pytest.raises(ValueError, match="lam"):
        K.wloss(pred, noise, w, None, None, 1.5)
    with pytest.raises(RuntimeError, match="shape"):
        K.wloss_bwd(pred, noise, w, None, None, 0.5, torch.ones(2, device=dev))


# ------------------------------------------------------------------------------------------ 3: crops
def test_crop_offsets_select_the_grid_rows(dev, monkeypatch):
    """Hg = 12, H = 4, row0 = [0, 3, 8] (the last window ends at the grid's end) on exact integer data: the batch must
    give what the three samples give one by one with the sliced weights and no offset.  One sample has n_b = 32
    elements, so out_b is exact and the batch's scalars are float32(sum_b out_b * 32 / 96); with gscale = fl32(1/3)
    the single-sample scale 2 g / 32 has the bits of the batch's 2 / 96, so dpred agrees bit for bit."""
    B, V, H, W, Hg = 3, 1, 4, 8, 12
    pred, noise, w, _, a = exact_case((B, V, H, W), Hg - H, seed=5)
    assert w.numel() == Hg and len(set(w[8:].tolist()) | set(w[:4].tolist())) > 1
    row0 = [0, 3, 8]
    pd, nd, wd, ad = pred.to(dev), noise.to(dev), w.to(dev), a.to(dev)
    got = K.wloss(pd, nd, wd, torch.tensor(row0, device=dev), ad, 0.5).cpu()
    dgot = K.wloss_bwd(pd, nd, wd, torch.tensor(row0, device=dev), ad, 0.5, torch.ones(1, device=dev)).cpu()
    acc = torch.zeros(3, dtype=torch.float64)
    for b, r in enumerate(row0):
        sl = wd[r:r + H].clone()
        ob = K.wloss(pd[b:b + 1], nd[b:b + 1], sl, None, ad[b:b + 1], 0.5).cpu()
        acc += ob.double() * (V * H * W)
        db = K.wloss_bwd(pd[b:b + 1], nd[b:b + 1], sl, None, ad[b:b + 1], 0.5,
                         torch.tensor([F32_THIRD], device=dev)).cpu()
        assert torch.equal(dgot[b:b + 1], db), f"sample {b}"
    assert torch.equal(got, (acc / (B * V * H * W)).float())
    want, dwant = ref64(pred, noise, w, row0, a, 0.5)
    assert torch.equal(got, want.float())
    assert torch.allclose(dgot.double(), dwant, rtol=1e-6, atol=0.0)

    # through Diffusion: a CPU row0 past the grid raises before anything is launched
    calls = []
    monkeypatch.setattr(K, "call", lambda name, *args: calls.append(name))
    d = Diffusion(torch.nn.Identity(), lat_weight=0.5, lat=np.linspace(-90.0, 90.0, Hg)).to(dev)
    with pytest.raises(ValueError, match="row0"):
        d.loss_components(pd[:1], None, row0=[9])
    with pytest.raises(ValueError, match="row0"):
        d.loss(pd[:1], None, row0=torch.tensor([9]))
    assert calls == []


# ------------------------------------------------------------------------------------------ 4: determinism
def test_two_calls_give_identical_bits(dev):
    shape = (4, 1, 192, 288)
    g = torch.Generator().manual_seed(9)
    pred, noise = torch.randn(shape, generator=g).to(dev), torch.randn(shape, generator=g).to(dev)
    w = (2 * torch.rand(192, generator=g)).to(dev)
    a = torch.rand(4, generator=g).to(dev)
    gs = torch.full((1,), 0.7, device=dev)
    o1, d1 = K.wloss(pred, noise, w, None, a, 0.3), K.wloss_bwd(pred, noise, w, None, a, 0.3, gs)
    torch.empty(1 << 22, device=dev).normal_()  # other work in between
    o2, d2 = K.wloss(pred, noise, w, None, a, 0.3), K.wloss_bwd(pred, noise, w, None, a, 0.3, gs)
    assert torch.equal(o1, o2) and torch.equal(d1, d2)
    want, dwant = ref64(pred.cpu(), noise.cpu(), w.cpu(), None, a.cpu(), 0.3, 0.7)
    # 221184 terms: fp32 partials of <= 864 terms each (relative error <= 864 * 2^-24 = 5.2e-5 in the worst case,
    # ~ sqrt of that for random data), then double
    assert torch.allclose(o1.cpu().double(), want, rtol=5.2e-5, atol=0.0)
    assert torch.allclose(d1.cpu().double(), dwant, rtol=1e-6, atol=0.0)


# ------------------------------------------------------------------------------------------ shared small model
SHAPE_HW = (16, 24)


def _net(dev, V, seed=1):
    torch.manual_seed(seed)
    net = UNet(out_channels=V, ch_mults=(1, 2, 4)).to(dev)
    net.compute_dtype = torch.float32
    return net


def _batch(dev, V, seed=0):
    H, W = SHAPE_HW
    g = torch.Generator().manual_seed(seed)
    x0 = torch.randn(2, V, H, W, generator=g).to(dev)
    cond = torch.randn(2, V, 2, H, W, generator=g).to(dev)
    t = torch.tensor([1, 3], device=dev)
    noise = torch.randn(2, V, H, W, generator=g).to(dev)
    return x0, cond, t, noise


def _grads(net):
    out = {k: p.grad.clone() for k, p in net.named_parameters() if p.grad is not None}
    for p in net.parameters():
        p.grad = None
    return out


# ------------------------------------------------------------------------------------------ 5: through the network
@pytest.mark.parametrize("V", [1, 2])
def test_loss_components_through_the_network(dev, V):
    """fp32 compute, fixed t and noise, lat_weight = 0.5, gamma = 5 on a 4-step schedule (a = [0.0005.., 1] does not
    matter: any a in (0, 1]).  Forward gate 1e-5 relative against the float64 formula applied to the network's own
    eps; gradient gate 1.2e-5 relative L2 per parameter against eps.backward(gradient = float64 dpred rounded to
    fp32)."""
    net = _net(dev, V)
    d = Diffusion(net, timesteps=4, lat_weight=0.5, min_snr_gamma=5.0).to(dev)
    x0, cond, t, noise = _batch(dev, V)
    comps = d.loss_components(x0, cond, t=t, noise=noise)
    assert set(comps) == {"mse_raw", "mse_lat", "cond_loss", "total"}
    assert all(v.ndim == 0 and v.is_cuda for v in comps.values())
    assert comps["total"].requires_grad and not any(comps[k].requires_grad for k in ("mse_raw", "mse_lat", "cond_loss"))
    assert float(comps["cond_loss"]) == 0.0
    comps["total"].backward()
    got = _grads(net)

    x_t, _ = d.q_sample(x0, t, noise)
    eps = d.model(x_t, cond, t)
    H = SHAPE_HW[0]
    lat = torch.linspace(-90.0, 90.0, H, dtype=torch.float64)
    w = torch.cos(torch.deg2rad(lat)).clamp_min(0.0)
    w = w / (w.mean() + 1e-8)
    ac = d.alphas_cumprod.double().cpu()
    a = torch.minimum(torch.ones(4, dtype=torch.float64), 5.0 * (1.0 - ac) / ac)[t.cpu()]
    assert float(a.min()) < 1.0
    want, dref = ref64(eps.detach().cpu(), noise.cpu(), w, None, a, 0.5)
    for i, k in enumerate(("mse_raw", "mse_lat", "total")):
        rel = abs(float(comps[k].detach()) - float(want[i])) / abs(float(want[i]))
        print(f"V={V} {k}: {float(comps[k].detach()):.8f} vs {float(want[i]):.8f} rel {rel:.2e}")
        assert rel <= 1e-5, k
    assert len({float(comps[k].detach()) for k in ("mse_raw", "mse_lat", "total")}) == 3
    eps.backward(gradient=dref.float().to(dev))
    ref = _grads(net)
    assert set(got) == set(ref) and len(got) > 10
    worst = 0.0
    for k in ref:
        den = ref[k].double().norm()
        err = (got[k].double() - ref[k].double()).norm()
        rel = float(err / den) if float(den) > 0 else float(err)
        worst = max(worst, rel)
        assert rel <= 1.2e-5, (k, rel)
    print(f"V={V}: worst parameter-gradient rel L2 {worst:.2e}")
    # loss() is the same number, and draws as the plain loss does
    assert torch.equal(d.loss(x0, cond, t=t, noise=noise).detach(), comps["total"].detach())
    plain = Diffusion(net, timesteps=4).to(dev)
    d.generator, plain.generator = rank_generator(dev, 4, 0), rank_generator(dev, 4, 0)
    d.loss(x0, cond), plain.loss(x0, cond)
    assert torch.equal(d.generator.get_state(), plain.generator.get_state())


# ------------------------------------------------------------------------------------------ 6: default path
def test_default_path_is_the_plain_mse(dev):
    net = _net(dev, 1)
    d = Diffusion(net, timesteps=4).to(dev)
    x0, cond, t, noise = _batch(dev, 1)
    runs = []
    for _ in range(2):
        loss = d.loss(x0, cond, t, noise)
        loss.backward()
        runs.append((loss.detach().clone(), _grads(net)))
    x_t, _ = d.q_sample(x0, t, noise)
    eps = d.model(x_t, cond, t).detach()
    assert torch.equal(runs[0][0], K.mse(eps, noise))
    assert torch.equal(runs[0][0], runs[1][0])
    assert set(runs[0][1]) == set(runs[1][1]) and len(runs[0][1]) > 10
    for k, g in runs[0][1].items():
        assert torch.equal(g, runs[1][1][k]), k
    # ... and a weighted loss with nothing to weigh agrees with it to rounding (it runs the other kernel, which adds
    # the 768 non-negative terms in another order: either fp32 summation tree is at most 12 deep, + 3 roundings per
    # term and for the mean -> 15 * 2^-24 = 9e-7 each, 1.8e-6 between the two)
    comps = d.loss_components(x0, cond, t=t, noise=noise)
    assert comps["total"].detach() == comps["mse_raw"]
    assert abs(float(comps["total"].detach()) - float(runs[0][0])) <= 1.8e-6 * float(runs[0][0])


# ------------------------------------------------------------------------------------------ 7: training loop
class _Log:
    def __init__(self, loader):
        self.rows, self.row0, self.loader = [], [], loader

    def log(self, epoch, step, mse_raw, mse_lat, cond_loss, total):
        self.rows.append((epoch, step, mse_raw, mse_lat, cond_loss, total))
        self.row0.append(self.loader.last_row0.clone())


def _fields(T=6, M=2, H=12, W=16, seed=2):
    g = np.random.default_rng(seed)
    return (g.standard_normal((T, M, H, W)).astype(np.float32), g.standard_normal((T, M, H, W)).astype(np.float32))


def _loop_setup(dev):
    torch.manual_seed(4)
    net = UNet(ch_mults=(1, 2)).to(dev)
    d = Diffusion(net, timesteps=50, lat_weight=0.5, min_snr_gamma=5.0, lat=np.linspace(-90.0, 90.0, 12)).to(dev)
    d.generator = rank_generator(dev, 7, 0)
    opt = FusedAdamW(d.parameters(), lr=1e-3, max_grad_norm=1.0)
    cond, tgt = _fields()
    ld = DA.DeviceWindowLoader(cond, tgt, 3, 4, dev, crop_hw=(4, 8), time_reverse_p=0.5, seed=0)
    return net, d, opt, ld


def _expected_row0(ld, epoch=0):
    """column 4 of the sampler's item rows, drawn in the loader's order (the caller seeds numpy)"""
    batches = DA.shard_indices(len(ld.sampler), ld.bs, 0, 1, True, ld.seed, epoch)
    return [torch.from_numpy(ld.sampler.items(b)[:, 4].copy()) for b in batches]


def test_training_loop_logs_components_and_passes_row_offsets(dev):
    net, d, opt, ld = _loop_setup(dev)
    assert ld.last_row0.numel() == 0 and len(ld) == 2
    log = _Log(ld)
    np.random.seed(21)
    mean = train_one_epoch(d, ld, opt, dev, 1.0, use_amp=False, epoch=3, metric_logger=log)
    assert len(log.rows) == 2 and [r[:2] for r in log.rows] == [(3, 1), (3, 2)]
    for r in log.rows:
        assert all(isinstance(v, float) and np.isfinite(v) for v in r[2:]) and len(r[2:]) == 4
        assert r[3] != r[2] and r[4] == 0.0
    assert mean == (log.rows[0][5] + log.rows[1][5]) / 2
    np.random.seed(21)
    want = _expected_row0(ld)
    assert len(want) == 2 and all(torch.equal(a, b) for a, b in zip(log.row0, want))
    assert all(r.dtype == torch.int64 and not r.is_cuda and tuple(r.shape) == (4,) for r in log.row0)
    assert len({int(v) for r in want for v in r}) > 1  # the crops really differ

    # replay: the same start, the same numpy and t / eps seeds; before each step the loss of the batch is taken with
    # loss_components, then the generator is put back and the step made
    net2, d2, opt2, ld2 = _loop_setup(dev)
    d2.train()
    net2.compute_dtype = torch.float32
    np.random.seed(21)
    for k, (cond, x0) in enumerate(ld2):
        state = d2.generator.get_state()
        c = d2.loss_components(x0, cond, row0=ld2.last_row0)
        assert float(c["total"].detach()) == log.rows[k][5], f"step {k + 1}"
        assert float(c["mse_raw"]) == log.rows[k][2] and float(c["mse_lat"]) == log.rows[k][3]
        shifted = d2.loss_components(x0, cond, row0=(ld2.last_row0 + 1) % 9)
        d2.generator.set_state(state)
        loss, comps = train_step(d2, opt2, x0, cond, 1.0, row0=ld2.last_row0, return_components=True)
        assert tuple(comps.shape) == (4,) and comps.is_cuda and comps.tolist() == list(log.rows[k][2:])
        assert torch.equal(loss, comps[3])
        assert float(shifted["mse_raw"]) != float(c["mse_raw"])  # other draws: the generator had moved on
    assert torch.equal(opt.flat.data, opt2.flat.data)

    # the plain loss through the same logger: mse_lat repeats the loss
    net3, d3, opt3, ld3 = _loop_setup(dev)
    d3 = Diffusion(net3, timesteps=50).to(dev)
    log3 = _Log(ld3)
    np.random.seed(21)
    train_one_epoch(d3, ld3, opt3, dev, 1.0, use_amp=False, metric_logger=log3)
    assert len(log3.rows) == 2 and all(r[2] == r[3] == r[5] and r[4] == 0.0 for r in log3.rows)


def test_pinned_loader_reports_the_yielded_batch(dev):
    """the pinned loader prepares batch k + 1 before it yields batch k: last_row0 must be batch k's"""
    cond, tgt = _fields()
    ld = DA.PinnedWindowLoader(cond, tgt, 3, 4, dev, crop_hw=(4, 8), time_reverse_p=0.5, seed=0)
    assert ld.last_row0.numel() == 0
    np.random.seed(33)
    seen = []
    for c, x in ld:
        seen.append((ld.last_row0.clone(), x.clone()))
    np.random.seed(33)
    batches = DA.shard_indices(len(ld.sampler), ld.bs, 0, 1, True, ld.seed, 0)
    items = [ld.sampler.items(b) for b in batches]
    assert len(seen) == 2 and not np.array_equal(items[0][:, 4], items[1][:, 4])
    for (r0, x), it in zip(seen, items):
        assert r0.dtype == torch.int64 and not r0.is_cuda and r0.tolist() == it[:, 4].tolist()
        for n, (t0, m, anchor, rev, i, j) in enumerate(it):  # and the offsets are those of the data it came with
            assert torch.equal(x[n, 0].cpu(), torch.from_numpy(tgt[anchor, m, i:i + 4, j:j + 8]))
