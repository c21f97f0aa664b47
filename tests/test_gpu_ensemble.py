"""Drawing and judging ensembles on the GPU: Diffusion.sample_ensemble (chunks, graph reuse, RNG), ensemble_stats /
EnsembleVerifier on sampled ensembles, train.validate_ensemble over a cropping loader, counterfactual_delta(n_samples=).

Tiny network (ch_mults (1, 2, 4), 16 x 24).  The float64 reference is tests/test_ensemble_host.ref64."""
import numpy as np
import pytest
import torch

from cesm_emulator_amd import EnsembleVerifier, counterfactual_delta, ensemble_stats
from cesm_emulator_amd import data as DA
from cesm_emulator_amd import model as MODEL
from cesm_emulator_amd.model import UNet, Diffusion, latitude_weights
from cesm_emulator_amd.train import validate_ensemble
from test_ensemble_host import ref64

pytestmark = pytest.mark.gpu

B, M, V, H, W = 2, 3, 1, 16, 24


def seed(s):
    torch.manual_seed(s)
    torch.cuda.manual_seed(s)


@pytest.fixture(scope="module")
def net(dev):
    torch.manual_seed(1)
    return UNet(ch_mults=(1, 2, 4)).to(dev)


def diffusion(net, dev, T, cdt, **kw):
    net.compute_dtype = cdt
    return Diffusion(net, timesteps=T, **kw).to(dev)


def inputs(dev, n_noise, cond_frames=None, s=0):
    g = torch.Generator().manual_seed(s)
    cshape = (B, V, H, W) if cond_frames is None else (B, V, cond_frames, H, W)
    cond = torch.randn(cshape, generator=g).to(dev)
    x_T = torch.randn(B, M, V, H, W, generator=g).to(dev)
    noise = torch.randn(n_noise, B, M, V, H, W, generator=g).to(dev)
    return cond, x_T, noise


@pytest.fixture
def captures(monkeypatch):
    """counts GraphSampleStep constructions"""
    made = []
    orig = MODEL.GraphSampleStep.__init__

    def init(self, *a, **kw):
        made.append(1)
        orig(self, *a, **kw)
    monkeypatch.setattr(MODEL.GraphSampleStep, "__init__", init)
    return made


# ------------------------------------------------------------------------------------------ 1: chunks == sample()
CASES = [dict(T=50, steps=3, eta=0.0), dict(T=50, steps=3, eta=0.5), dict(T=4, steps=None, eta=0.0)]


@pytest.mark.parametrize("cdt", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("case", CASES, ids=["ddim_eta0", "ddim_eta05", "ddpm4"])
def test_every_chunk_equals_sample_on_its_rows(dev, net, captures, cdt, case):
    """With x_T and noise_seq given, chunk [j0, j1) of the b-major job list must equal, bit for bit,
    sample(cond.repeat_interleave(M, 0)[j0:j1], x_T=..., noise_seq=...): eager and graph, member_batch None / 4 / 3."""
    d = diffusion(net, dev, case["T"], cdt)
    n_noise = case["T"] if case["steps"] is None else case["steps"]
    cond, x_T, noise = inputs(dev, n_noise)
    jobs = B * M
    rep = cond.repeat_interleave(M, 0)
    xf, nf = x_T.reshape(jobs, V, H, W), noise.reshape(n_noise, jobs, V, H, W)
    kw = dict(steps=case["steps"], ddim_eta=case["eta"])
    for use_graph in (False, True):
        for mb, want_captures in ((None, 1), (4, 2), (3, 1)):
            del captures[:]
            ens = d.sample_ensemble(cond, M, member_batch=mb, x_T=x_T, noise_seq=noise, use_graph=use_graph, **kw)
            assert tuple(ens.shape) == (B, M, V, H, W) and ens.dtype == torch.float32 and ens.is_contiguous()
            assert len(captures) == (want_captures if use_graph else 0), (mb, use_graph, len(captures))
            flat = ens.view(jobs, V, H, W)
            step = jobs if mb is None else mb
            for j0 in range(0, jobs, step):
                j1 = min(j0 + step, jobs)
                want = d.sample(rep[j0:j1], (j1 - j0, V, H, W), dev, use_graph=use_graph, x_T=xf[j0:j1],
                                noise_seq=nf[:, j0:j1], **kw)
                assert torch.equal(flat[j0:j1], want), (use_graph, mb, j0)
            assert bool(torch.isfinite(ens).all()) and float(ens.std()) > 0
            # members of one condition differ (their x_T differ), and the hooks were not written to
            assert not torch.equal(ens[:, 0], ens[:, 1])


def test_chunk_sizes_observed_not_gated(dev, net):
    """Whether two different chunk sizes give the same bits depends on the batch-invariance of the network kernels;
    observed and printed (DESIGN records it), not gated."""
    d = diffusion(net, dev, 50, torch.float32)
    cond, x_T, noise = inputs(dev, 3)
    runs = {mb: d.sample_ensemble(cond, M, steps=3, member_batch=mb, x_T=x_T, noise_seq=noise) for mb in (None, 4, 1)}
    for mb in (4, 1):
        same = torch.equal(runs[None], runs[mb])
        err = float((runs[None] - runs[mb]).abs().max())
        print(f"member_batch {mb} vs one chunk (fp32, 3 DDIM steps): bit-equal {same}, max |diff| {err:.3e}")


def test_rng_use_is_chunk_by_chunk_and_sample_is_unchanged(dev, net):
    """Without hooks: x_T of chunk 0, its step noise, x_T of chunk 1, ...; sample() before and after a sample_ensemble
    call on the same Diffusion gives the same bits under the same seed."""
    d = diffusion(net, dev, 50, torch.float32)
    cond, _, _ = inputs(dev, 1)
    seed(3)
    before = d.sample(cond, (B, V, H, W), dev, steps=3, ddim_eta=0.5)
    seed(4)
    ens = d.sample_ensemble(cond, M, steps=3, ddim_eta=0.5, member_batch=4)
    seed(3)
    after = d.sample(cond, (B, V, H, W), dev, steps=3, ddim_eta=0.5)
    assert torch.equal(before, after)
    # the draws of the call above, restated: per chunk randn(x_T), then one randn_like per executed step but the last
    seed(4)
    rep = cond.repeat_interleave(M, 0)
    for j0, j1 in ((0, 4), (4, 6)):
        xT = torch.randn((j1 - j0, V, H, W), device=dev)
        nz = torch.stack([torch.randn((j1 - j0, V, H, W), device=dev) for _ in range(2)] +
                         [torch.zeros((j1 - j0, V, H, W), device=dev)])
        want = d.sample(rep[j0:j1], (j1 - j0, V, H, W), dev, steps=3, ddim_eta=0.5, x_T=xT, noise_seq=nz)
        assert torch.equal(ens.view(B * M, V, H, W)[j0:j1], want), j0


def test_window_cond_works(dev, net):
    d = diffusion(net, dev, 50, torch.float32)
    cond, x_T, _ = inputs(dev, 1, cond_frames=3)
    ens = d.sample_ensemble(cond, M, steps=2, x_T=x_T, member_batch=4)
    assert tuple(ens.shape) == (B, M, V, H, W)
    rep, xf = cond.repeat_interleave(M, 0), x_T.reshape(B * M, V, H, W)
    for j0, j1 in ((0, 4), (4, 6)):
        want = d.sample(rep[j0:j1], (j1 - j0, V, H, W), dev, steps=2, x_T=xf[j0:j1])
        assert torch.equal(ens.view(B * M, V, H, W)[j0:j1], want), j0
    # the window matters: another frame order gives another ensemble
    other = d.sample_ensemble(cond.flip(2), M, steps=2, x_T=x_T, member_batch=4)
    assert not torch.equal(other, ens)


# ------------------------------------------------------------------------------------------ 2: judging a sample
def check_scalars(got, ens_list, obs_list, w, row0_list, M):
    """scalars of a result dict against the float64 formulas on the same ensembles: the accumulated columns within 1e-5
    relative (the fp32-kernel gate), the histogram within 1e-5 of sum w unless a comparison is within rounding"""
    acc = None
    near = False
    for ens, obs, r0 in zip(ens_list, obs_list, row0_list):
        r = ref64(ens, obs, w, r0)
        acc = r["acc"] if acc is None else acc + r["acc"]
        near = near or bool(((ens.cpu().double() - obs.cpu().double()[:, None]).abs() < 2.0 ** -20).any())
    sw = acc[:, 0]
    want = {"mse": acc[:, 1] / sw, "var": acc[:, 2] / sw, "crps": acc[:, 3] / sw}
    want["rmse"], want["spread"] = want["mse"].sqrt(), want["var"].sqrt()
    want["ssr"] = ((M + 1) / M * want["var"] / want["mse"]).sqrt()
    for k, v in want.items():
        rel = float(((got[k].cpu() - v).abs() / v.abs()).max())
        print(f"{k}: {got[k].cpu().tolist()} vs {v.tolist()} rel {rel:.2e}")
        assert rel <= 1e-5, k
    hist = got["rank_hist"].cpu()
    assert tuple(hist.shape) == (acc.shape[0], M + 1) and float((hist.sum(1) - 1).abs().max()) <= 1e-12
    if not near:
        assert float((hist - acc[:, 4:] / sw[:, None]).abs().max()) <= 1e-5
    return want


def test_stats_and_verifier_on_a_sampled_ensemble(dev, net):
    lat = np.linspace(-80.0, 80.0, H + 4)
    d = diffusion(net, dev, 50, torch.float32)
    cond, x_T, _ = inputs(dev, 1)
    seed(6)
    ens = d.sample_ensemble(cond, M, steps=2)
    obs = torch.randn(B, V, H, W, device=dev)
    row0 = [0, 4]
    w = latitude_weights(lat)
    r = ensemble_stats(ens, obs, lat=lat, row0=row0)
    ref = ref64(ens, obs, w, row0)
    for k in ("mean", "var", "crps"):
        e = float((r["maps"][k].cpu().double() - ref[k]).norm() / ref[k].norm())
        assert e <= 1e-5, (k, e)
    assert torch.equal(r["maps"]["rank"].cpu().long(), ref["rank"])
    check_scalars(r, [ens], [obs], w, [row0], M)
    assert ensemble_stats(ens, obs, lat=lat, row0=row0, maps=False)["maps"] is None
    no = ensemble_stats(ens, lat=lat, row0=row0)
    assert no["mse"] is None and no["maps"]["crps"] is None and torch.equal(no["var"], r["var"])
    # uniform weights without lat
    u = ensemble_stats(ens, obs)
    check_scalars(u, [ens], [obs], torch.ones(H), [None], M)
    # the verifier over two updates = both batches in the formula; reset() starts over
    v = EnsembleVerifier(M, V, lat=lat, device=dev)
    obs2 = torch.randn(B, V, H, W, device=dev)
    v.update(ens, obs, row0=row0)
    v.update(ens, obs2, row0=torch.tensor([2, 1], device=dev))
    check_scalars(v.result(), [ens, ens], [obs, obs2], w, [row0, [2, 1]], M)
    v.reset()
    v.update(ens, obs, row0=row0)
    assert all(torch.equal(v.result()[k], r[k]) for k in ("mse", "var", "crps", "rank_hist", "ssr"))


# ------------------------------------------------------------------------------------------ 3: validation loop
def _fields(T=6, Mf=2, Hf=24, Wf=32, s=2):
    g = np.random.default_rng(s)
    return (g.standard_normal((T, Mf, Hf, Wf)).astype(np.float32), g.standard_normal((T, Mf, Hf, Wf)).astype(np.float32))


class _Shifted:
    """a loader whose reported crop rows are off by `by`"""

    def __init__(self, loader, by, mod):
        self.loader, self.by, self.mod = loader, by, mod
        self.last_row0 = loader.last_row0

    def __iter__(self):
        for item in self.loader:
            self.last_row0 = (self.loader.last_row0 + self.by) % self.mod
            yield item


def test_validate_ensemble_over_a_cropping_loader(dev, net):
    lat = np.linspace(-85.0, 85.0, 24)
    d = diffusion(net, dev, 50, torch.float32, lat=lat)
    cf, tf = _fields()
    ld = DA.DeviceWindowLoader(cf, tf, 3, 2, dev, crop_hw=(H, W), time_reverse_p=0.5, seed=0)
    assert len(ld) == 4

    def run(loader):
        np.random.seed(21)
        seed(8)
        return validate_ensemble(d, loader, M, steps=2, ddim_eta=0.5, member_batch=4, max_batches=2)

    got = run(ld)
    # the same ensembles again: same numpy crops, same torch draws
    np.random.seed(21)
    seed(8)
    ens_l, obs_l, row0_l = [], [], []
    for k, (cond, x0) in enumerate(ld):
        if k == 2:
            break
        ens_l.append(d.sample_ensemble(cond, M, steps=2, ddim_eta=0.5, member_batch=4).clone())
        obs_l.append(x0.clone())
        row0_l.append(ld.last_row0.clone())
    assert len({int(v) for r in row0_l for v in r}) > 1  # the crops really differ
    check_scalars(got, ens_l, obs_l, latitude_weights(lat), row0_l, M)
    again = run(ld)
    assert all(torch.equal(got[k], again[k]) for k in got)
    wrong = run(_Shifted(ld, 3, 24 - H + 1))
    assert not torch.equal(wrong["crps"], got["crps"]) and not torch.equal(wrong["mse"], got["mse"])


# ------------------------------------------------------------------------------------------ 4: counterfactual
def test_counterfactual_delta_with_members(dev, net):
    """n_samples = 3, paired: the member mean of pert - base where member m of both ensembles shares x_T and noise.
    Bit-equal to one sampler batch [cond x 3, cond2 x 3] fed the same draws; against three separate paired runs of
    batch 2 B (another batch size: the network kernels' batch-invariance is not established) the gate is 1e-3 relative
    L2: the fp32 parity gate of a forward is 1e-5, two steps double it, and the delta of a 10 % change in cond is a
    difference of fields about ten times its own size -- 2e-4, with a margin of 5.  n_samples = 1 is today's call."""
    d = diffusion(net, dev, 50, torch.float32)
    cond, _, _ = inputs(dev, 1)
    seed(12)
    got = counterfactual_delta(d, cond, steps=2, ddim_eta=0.5, paired=True, n_samples=3)
    assert tuple(got.shape) == (B, V, H, W) and float(got.abs().max()) > 0
    seed(12)
    n = B * 3
    xT = torch.randn((n, V, H, W), device=dev)
    nz = torch.stack([torch.randn((n, V, H, W), device=dev), torch.zeros((n, V, H, W), device=dev)])
    cond2 = cond * 1.1
    both = torch.cat([cond.repeat_interleave(3, 0), cond2.repeat_interleave(3, 0)])
    x = d.sample(both, (2 * n, V, H, W), dev, steps=2, ddim_eta=0.5, x_T=xT.repeat(2, 1, 1, 1),
                 noise_seq=nz.repeat(1, 2, 1, 1, 1))
    want = x[n:].view(B, 3, V, H, W).mean(1) - x[:n].view(B, 3, V, H, W).mean(1)
    assert torch.equal(got, want)
    deltas = []
    for m in range(3):
        xm, nm = xT.view(B, 3, V, H, W)[:, m], nz.view(2, B, 3, V, H, W)[:, :, m]
        base = d.sample(cond, (B, V, H, W), dev, steps=2, ddim_eta=0.5, x_T=xm, noise_seq=nm)
        pert = d.sample(cond2, (B, V, H, W), dev, steps=2, ddim_eta=0.5, x_T=xm, noise_seq=nm)
        deltas.append((pert - base).double())
    by_hand = torch.stack(deltas).mean(0)
    rel = float((got.double() - by_hand).norm() / by_hand.norm())
    print(f"paired n_samples=3 vs three paired runs: rel L2 {rel:.2e}")
    assert rel <= 1e-3
    # unpaired n > 1: base ensemble first, then the perturbed one
    seed(13)
    un = counterfactual_delta(d, cond, steps=2, n_samples=3)
    seed(13)
    base = d.sample_ensemble(cond, 3, steps=2).mean(1)
    pert = d.sample_ensemble(cond2, 3, steps=2).mean(1)
    assert torch.equal(un, pert - base)
    # n_samples = 1: bit-equal to the call without the argument, paired or not
    for paired in (False, True):
        seed(14)
        a = counterfactual_delta(d, cond, steps=2, ddim_eta=0.5, paired=paired)
        seed(14)
        b = counterfactual_delta(d, cond, steps=2, ddim_eta=0.5, paired=paired, n_samples=1)
        assert torch.equal(a, b)
    with pytest.raises(ValueError, match="n_samples"):
        counterfactual_delta(d, cond, steps=2, n_samples=0)
