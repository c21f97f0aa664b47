"""Training data path: dataset_single_member.py's windowed sampler + the train.py load → device copy.

Two device feeds, both producing the reference's batches `cond [B,1,K,h,w]`, `x0 [B,1,h,w]`:

* `DeviceWindowLoader` — the z-scored (T, M, H, W) fields live in HBM (2.2 GB each for the full
  CESM2-LE grid, a rounding error in 288 GB); per batch the host only draws the item parameters
  (t0, member, anchor, reverse flag, crop offsets — same numpy RNG order as the reference
  `__getitem__`) and the `cesm_window_gather` kernel assembles the batch on device.
* `PinnedWindowLoader` — host-resident fields: items are gathered on the host into pinned
  double-buffers and copied with non-blocking H2D copies on a side stream, overlapped with the
  previous step's compute and ordered with events.

`load_cond_and_target` restates train.py:600-650 for .npy/.npz inputs (NetCDF readers — xarray,
netCDF4 — are not in this image); z-scoring uses the reference's single global mean/std.

Multi-variable fields (T, M, C, H, W) and the random sample modes go through the same two loaders: the
host draws explicit frame indices per item (`WindowSampler.draw`) and `cesm_window_gather_mv` (or its numpy
twin `host_gather_mv`) assembles `cond [B,V,K,h,w]`, `x0 [B,V,h,w]`.  `load_fields` loads and z-scores
per variable and returns the statistics (`norm`) that `denormalize` and the checkpoint carry;
`loader_from_config` builds either loader from a config's `dataset` / `train` sections.  With `cond_channels=Cc` (a
model built with `UNet(cond_channels=Cc)`) the loaders take Cc `cond_select` indices into the forcing variables and
assemble `cond [B,Cc,K,h,w]` (`cesm_window_gather_mc` where Cc differs from V).
"""
from __future__ import annotations

import numpy as np
import torch

from . import kernels as K


def zscore(a):
    """train.py:640-646: one global mean/std per array (std + 1e-8)."""
    m, s = float(a.mean()), float(a.std() + 1e-8)
    return ((a - m) / s).astype(np.float32), m, s


def load_cond_and_target(cond_file, target_file, cond_var=None, target_var=None, normalize=True):
    """(T, M, H, W) float32 arrays from .npy / .npz files (key = var name, or the only array)."""
    def _load(path, var):
        if str(path).endswith(".nc"):
            raise RuntimeError("NetCDF input needs xarray/netCDF4, which this image lacks: convert to .npz")
        obj = np.load(path, allow_pickle=False)
        if isinstance(obj, np.lib.npyio.NpzFile):
            arr = obj[var] if var is not None else obj[obj.files[0]]
        else:
            arr = obj
        arr = np.asarray(arr, dtype=np.float32)
        if arr.ndim == 5:
            arr = arr[:, :, 0]
        if arr.ndim != 4:
            raise ValueError(f"expected (T, M, H, W) data in {path}, got shape {arr.shape}")
        return arr

    c = _load(cond_file, cond_var)
    t = _load(target_file, target_var)
    if normalize:
        c, _, _ = zscore(c)
        t, _, _ = zscore(t)
    return c, t


def load_fields(cond_file, target_file, cond_vars=None, target_vars=None, normalize=True):
    """Multi-variable load: (cond [T, M, Vc, H, W], tgt [T, M, V, H, W], norm) from .npy / .npz files.  A variable
    argument is a name or a list of names ((T, M, H, W) arrays stacked in that order), or one key (None: the only
    array) that holds a (T, M, C, H, W) array.  Z-scoring is per variable: mean and std + 1e-8 over that variable's
    plane -- with one variable the reference's global statistics, bit for bit what zscore() gives.  norm is a dict of
    plain lists (cond_vars, target_vars, cond_mean, cond_std, target_mean, target_std; mean 0 and std 1 without
    normalize): what save_checkpoint(norm=) stores and denormalize() takes."""
    def _load(path, names):
        if str(path).endswith(".nc"):
            raise RuntimeError("NetCDF input needs xarray/netCDF4, which this image lacks: convert to .npz")
        obj = np.load(path, allow_pickle=False)
        many = isinstance(names, (list, tuple))
        keys = list(names) if many else [names]
        planes = []
        for key in keys:
            if isinstance(obj, np.lib.npyio.NpzFile):
                if key is None:
                    key = obj.files[0]
                arr = obj[key]
            else:
                arr = obj
            arr = np.asarray(arr, dtype=np.float32)
            if arr.ndim == 5 and not many:
                n = arr.shape[2]
                return arr, [str(key)] if n == 1 else [f"{key}[{c}]" for c in range(n)]
            if arr.ndim != 4:
                raise ValueError(f"expected (T, M, H, W) data for {key!r} in {path}, got shape {arr.shape}")
            planes.append(arr)
        return np.stack(planes, axis=2), [str(k) for k in keys]

    def _norm(a):
        out, mean, std = np.empty_like(a), [], []
        for c in range(a.shape[2]):
            if normalize:
                out[:, :, c], m, s = zscore(a[:, :, c])
            else:
                out[:, :, c], m, s = a[:, :, c], 0.0, 1.0
            mean.append(m)
            std.append(s)
        return out, mean, std

    c, cn = _load(cond_file, cond_vars)
    t, tn = _load(target_file, target_vars)
    c, cm, cs = _norm(c)
    t, tm, ts = _norm(t)
    norm = {"cond_vars": cn, "target_vars": tn, "cond_mean": cm, "cond_std": cs, "target_mean": tm, "target_std": ts}
    return c, t, norm


def denormalize(x, norm, which="target"):
    """Physical units of a z-scored target tensor: x [B, V, H, W] or [B, M, V, H, W] (an ensemble) times
    norm["target_std"][v] plus norm["target_mean"][v], in x's dtype; which="cond" uses the cond statistics."""
    mean, std = norm[f"{which}_mean"], norm[f"{which}_std"]
    if x.ndim not in (4, 5) or x.shape[-3] != len(mean):
        raise ValueError(f"denormalize: x must be [B, V, H, W] or [B, M, V, H, W] with V = {len(mean)}, got "
                         f"{tuple(x.shape)}")
    m = torch.tensor(mean, dtype=x.dtype, device=x.device).view(-1, 1, 1)
    s = torch.tensor(std, dtype=x.dtype, device=x.device).view(-1, 1, 1)
    return x * s + m


class WindowSampler:
    """Item-parameter draws of WindowedAllMembersDataset_random, all three sample modes:
    dataset_single_member.py:91-102 (index -> t0/anchor/member), :104-150 (_choose_times), :180 (time reversal draw),
    :156-166 (crop draw).  Uses numpy's global RNG in the reference's per-item order: the _choose_times draws, then the
    reversal draw, then the crop draws.  item() / items() are the consecutive mode's compact form (t0, m, anchor, rev,
    i, j); draw() serves every mode with explicit frame indices."""

    def __init__(self, T, M, H, W, K, center=True, crop_hw=None, crop_mode="random", time_reverse_p=0.5,
                 sample_mode="consecutive", *, window_radius=5, keep_chronology=True, causal=False,
                 allow_replace=False):
        if sample_mode not in ("consecutive", "random_window", "random_global"):
            raise ValueError(f"sample_mode must be consecutive, random_window or random_global, got {sample_mode!r}")
        if K < 2:
            raise ValueError("K must be >= 2")
        self.T, self.M, self.H, self.W, self.K = T, M, H, W, int(K)
        self.center = bool(center)
        self.crop = None if not crop_hw else (min(int(crop_hw[0]), H), min(int(crop_hw[1]), W))
        self.crop_mode = crop_mode
        self.p = float(time_reverse_p)
        self.sample_mode = sample_mode
        self.window_radius = int(window_radius)
        self.keep_chronology = bool(keep_chronology)
        self.causal = bool(causal)
        self.allow_replace = bool(allow_replace)  # sticky: turned on for good once a pool runs short (:127-128)
        if self.causal and self.center:
            self.center = False
        self.num_units = max(1, T - self.K + 1) if sample_mode == "consecutive" else T

    def __len__(self):
        return self.num_units * self.M

    @property
    def hw(self):
        return self.crop if self.crop else (self.H, self.W)

    def _reverse_draw(self):
        return 1 if (self.p > 0.0 and np.random.rand() < self.p) else 0

    def _crop_draw(self):
        i = j = 0
        if self.crop:
            h, w = self.crop
            if self.crop_mode == "center":
                i, j = max(0, (self.H - h) // 2), max(0, (self.W - w) // 2)
            else:
                i = 0 if self.H == h else np.random.randint(0, self.H - h + 1)
                j = 0 if self.W == w else np.random.randint(0, self.W - w + 1)
        return i, j

    def item(self, idx):
        if self.sample_mode != "consecutive":
            raise ValueError(f"item() is the consecutive mode's (t0, m, anchor, rev, i, j); sample_mode "
                             f"{self.sample_mode!r} needs draw()")
        m, t0 = idx % self.M, idx // self.M
        anchor = t0 + (self.K // 2) if self.center else t0 + self.K - 1
        anchor = int(np.clip(anchor, 0, self.T - 1))
        rev = self._reverse_draw()
        i, j = self._crop_draw()
        return [t0, m, anchor, rev, i, j]

    def items(self, indices):
        return np.asarray([self.item(int(k)) for k in indices], dtype=np.int64).reshape(-1, 6)

    def _choose_times(self, t0, anchor):
        """dataset_single_member.py:104-150: the K frame indices of one item, the anchor at K // 2 (center) or last"""
        K = self.K
        if self.sample_mode == "consecutive":
            return np.arange(t0, t0 + K, dtype=np.int64)
        if self.sample_mode == "random_global":
            pool = np.arange(0, self.T, dtype=np.int64)
        else:
            pool = np.arange(max(0, anchor - self.window_radius), min(self.T - 1, anchor + self.window_radius) + 1,
                             dtype=np.int64)
        if self.causal:
            pool = pool[pool <= anchor]
        pool_wo = pool[pool != anchor]
        need = K - 1
        if (not self.allow_replace) and pool_wo.size < need:
            self.allow_replace = True
        if self.allow_replace:
            sampled = (np.full((need,), anchor, dtype=np.int64) if pool_wo.size == 0
                       else np.random.choice(pool_wo, size=need, replace=True))
        else:
            sampled = np.random.choice(pool_wo, size=need, replace=False)
        times = np.concatenate([sampled, np.array([anchor], dtype=np.int64)])
        if self.keep_chronology:
            times.sort()
        if self.center:
            times = np.roll(times, K // 2 - int(np.where(times == anchor)[0][0]))
        elif pool_wo.size:
            times = np.array([t for t in times if t != anchor] + [anchor], dtype=np.int64)
        # else: an empty pool (causal at anchor 0) made every frame the anchor.  The reference's filter then leaves ONE
        # frame, a window no batch can hold; here the window keeps its K frames, all of them the anchor.
        return times

    def draw(self, indices):
        """(times [n, K], meta [n, 4] = (member, anchor, i, j)) int64 arrays of the items `indices`, in any sample mode;
        the time reversal is already applied to the times row (what cesm_window_gather_mv / host_gather_mv take).
        The grid row of each sample's row 0 is meta[:, 2]."""
        n, K, mid = len(indices), self.K, self.K // 2
        times, meta = np.empty((n, K), dtype=np.int64), np.empty((n, 4), dtype=np.int64)
        for r, idx in enumerate(indices):
            idx = int(idx)
            m, u = idx % self.M, idx // self.M
            if self.sample_mode == "consecutive":
                t0 = u
                anchor = t0 + mid if self.center else t0 + K - 1
            else:
                anchor = u
                t0 = max(0, min(anchor - mid, self.T - K))
            anchor = int(np.clip(anchor, 0, self.T - 1))
            tt = self._choose_times(t0, anchor)
            if self._reverse_draw():
                tt = np.concatenate([tt[:mid][::-1], tt[mid:mid + 1], tt[mid + 1:][::-1]]) if self.center else tt[::-1]
            i, j = self._crop_draw()
            times[r] = tt
            meta[r] = (m, anchor, i, j)
        return times, meta


def row0_of(items):
    """the crop row offsets of item rows (column 4: the grid row of each sample's row 0; zeros without a crop) as an
    int64 CPU tensor [n] -- what Diffusion.loss(..., row0=) takes"""
    return torch.from_numpy(np.ascontiguousarray(np.asarray(items, dtype=np.int64).reshape(-1, 6)[:, 4]))


def host_gather(cond, tgt, items, K, h, w, center, out_c, out_x):
    """Host-side batch assembly for the pinned path: out_c [n,1,K,h,w], out_x [n,1,h,w] (numpy
    views of pinned buffers) from (T,M,H,W) fields and item rows (t0, m, anchor, rev, i, j)."""
    for n, (t0, m, anchor, rev, i, j) in enumerate(items):
        cw = cond[t0:t0 + K, m, i:i + h, j:j + w]
        if rev:
            if center:
                mid = K // 2
                cw = np.concatenate([cw[:mid][::-1], cw[mid:mid + 1], cw[mid + 1:][::-1]], axis=0)
            else:
                cw = cw[::-1]
        out_c[n, 0] = cw
        out_x[n, 0] = tgt[anchor, m, i:i + h, j:j + w]


def host_gather_mv(cond, tgt, times, meta, csel, h, w, out_c, out_x):
    """numpy twin of cesm_window_gather_mv / cesm_window_gather_mc for the pinned path: out_c [n, Cc, K, h, w], out_x
    [n, V, h, w] (numpy views of pinned buffers) from cond (T, M, Vc, H, W), tgt (T, M, V, H, W), times [n, K], meta
    [n, 4] = (member, anchor, i, j) and the Cc forcing-plane indices csel (Cc = len(csel): V without cond_channels)."""
    csel = np.asarray(csel, dtype=np.int64)
    if out_c.shape[1] != len(csel) or out_x.shape[1] != tgt.shape[2]:
        raise ValueError(f"host_gather_mv: out_c has {out_c.shape[1]} planes for {len(csel)} cond_select indices, "
                         f"out_x {out_x.shape[1]} for {tgt.shape[2]} target variables")
    for n, (tt, (m, anchor, i, j)) in enumerate(zip(times, meta)):
        for v, c in enumerate(csel):
            out_c[n, v] = cond[tt, m, c, i:i + h, j:j + w]
        out_x[n] = tgt[anchor, m, :, i:i + h, j:j + w]


MAX_COND = K.STEM_MAX_COND


def resolve_cond_select(cond_select, Vc, V, cond_channels=None):
    """The V forcing-plane indices that feed the stem's V cond channels: identity when Vc == V, all zeros when there is
    one forcing, anything else has to be given.  cond_channels = Cc (a model built with UNet(cond_channels=Cc)): Cc
    indices into the Vc forcing variables instead, identity when Vc == Cc, else they have to be given."""
    if cond_channels is not None:
        Cc = cond_channels
        if isinstance(Cc, bool) or not isinstance(Cc, int) or not 1 <= Cc <= MAX_COND:
            raise ValueError(f"cond_channels must be None or 1 … {MAX_COND}, got {Cc!r}")
        if cond_select is None:
            if Vc != Cc:
                raise ValueError(f"cond has {Vc} variables and the model takes {Cc} conditioning maps: give "
                                 f"cond_select= ({Cc} indices into the {Vc} cond variables)")
            cond_select = range(Cc)
        sel = [int(c) for c in cond_select]
        if len(sel) != Cc:
            raise ValueError(f"cond_select needs one index per conditioning map ({Cc}), got {sel}")
        for c in sel:
            if not 0 <= c < Vc:
                raise ValueError(f"cond_select = {c} outside [0, {Vc - 1}]")
        return sel
    if cond_select is None:
        if Vc == V:
            cond_select = range(V)
        elif Vc == 1:
            cond_select = [0] * V
        else:
            raise ValueError(f"cond has {Vc} variables and the target {V}: give cond_select= ({V} indices into the "
                             f"{Vc} cond variables)")
    sel = [int(c) for c in cond_select]
    if len(sel) != V:
        raise ValueError(f"cond_select needs one index per target variable ({V}), got {sel}")
    for c in sel:
        if not 0 <= c < Vc:
            raise ValueError(f"cond_select = {c} outside [0, {Vc - 1}]")
    return sel


def _fields_5d(cond, tgt):
    """(cond, tgt, legacy): fp32 arrays; legacy is True for the single-variable layout (T, M, H, W) (a 5-D pair with one
    variable each is squeezed to it), else both are (T, M, C, H, W)."""
    cond = np.asarray(cond, dtype=np.float32)
    tgt = np.asarray(tgt, dtype=np.float32)
    if cond.ndim not in (4, 5) or tgt.ndim not in (4, 5):
        raise ValueError(f"expected (T, M, H, W) or (T, M, C, H, W) fields, got {cond.shape} and {tgt.shape}")
    if cond.ndim == 5 and tgt.ndim == 5 and cond.shape[2] == 1 and tgt.shape[2] == 1:
        cond, tgt = cond[:, :, 0], tgt[:, :, 0]
    if cond.ndim == 4 and tgt.ndim == 4:
        if cond.shape != tgt.shape:
            raise ValueError(f"cond {cond.shape} and target {tgt.shape} differ")
        return cond, tgt, True
    cond = cond[:, :, None] if cond.ndim == 4 else cond
    tgt = tgt[:, :, None] if tgt.ndim == 4 else tgt
    if cond.shape[:2] != tgt.shape[:2] or cond.shape[3:] != tgt.shape[3:]:
        raise ValueError(f"cond {cond.shape} and target {tgt.shape} differ in T, M, H or W")
    return cond, tgt, False


def shard_indices(n, batch_size, rank=0, world=1, shuffle=True, seed=0, epoch=0, drop_last=False):
    """DistributedSampler semantics (train.py:1002): seeded permutation per epoch, padded to a
    multiple of world, rank-strided; then cut into batches."""
    if shuffle:
        g = torch.Generator()
        g.manual_seed(seed + epoch)
        idx = torch.randperm(n, generator=g).tolist()
    else:
        idx = list(range(n))
    total = -(-n // world) * world
    idx = (idx + idx[: total - n])[:total] if total > n else idx
    mine = idx[rank:total:world]
    batches = [mine[k:k + batch_size] for k in range(0, len(mine), batch_size)]
    if drop_last and batches and len(batches[-1]) < batch_size:
        batches = batches[:-1]
    return batches


class DeviceWindowLoader:
    """HBM-resident fields + device gather kernel; iterate -> (cond [B,V,K,h,w], x0 [B,V,h,w]); with cond_channels=Cc
    (a model built with UNet(cond_channels=Cc)) cond is [B,Cc,K,h,w] from Cc cond_select indices, through
    cesm_window_gather_mc where Cc != V.
    (T, M, H, W) fields, or (T, M, 1, H, W), in consecutive mode: V = 1 through cesm_window_gather, as ever.
    (T, M, C, H, W) fields with more than one variable, or a random sample mode: cesm_window_gather_mv; cond_select
    names the forcing plane of each of the V cond channels (resolve_cond_select).
    last_row0: the crop row offsets (row0_of) of the batch last yielded."""

    def __init__(self, cond, tgt, K, batch_size, device, center=True, crop_hw=None, crop_mode="random",
                 time_reverse_p=0.5, shuffle=True, seed=0, rank=0, world=1, *, cond_select=None,
                 sample_mode="consecutive", window_radius=5, keep_chronology=True, causal=False, allow_replace=False,
                 cond_channels=None):
        cond, tgt, single = _fields_5d(cond, tgt)
        self.legacy = single and sample_mode == "consecutive" and cond_channels is None
        if single and not self.legacy:
            cond, tgt = cond[:, :, None], tgt[:, :, None]
        T, M, H, W = cond.shape[0], cond.shape[1], cond.shape[-2], cond.shape[-1]
        self.csel = None if self.legacy else resolve_cond_select(cond_select, cond.shape[2], tgt.shape[2],
                                                                 cond_channels)
        # cond_channels maps that are not one per target variable: the gather with the plane counts separated
        self.split = not self.legacy and len(self.csel) != tgt.shape[2]
        self.sampler = WindowSampler(T, M, H, W, K, center, crop_hw, crop_mode, time_reverse_p, sample_mode,
                                     window_radius=window_radius, keep_chronology=keep_chronology, causal=causal,
                                     allow_replace=allow_replace)
        self.cond = torch.from_numpy(np.ascontiguousarray(cond)).to(device)
        self.tgt = torch.from_numpy(np.ascontiguousarray(tgt)).to(device)
        self.bs, self.device = batch_size, device
        self.shuffle, self.seed, self.rank, self.world = shuffle, seed, rank, world
        self.epoch = 0
        self._items_host = torch.empty((batch_size, 6), dtype=torch.int64).pin_memory() if self.legacy else None
        self.last_row0 = torch.zeros(0, dtype=torch.int64)

    def set_epoch(self, e):
        self.epoch = e

    def __len__(self):
        return len(shard_indices(len(self.sampler), self.bs, self.rank, self.world, False))

    def batch(self, indices):
        h, w = self.sampler.hw
        if not self.legacy:
            times, meta = self.sampler.draw(indices)
            self.last_row0 = torch.from_numpy(np.ascontiguousarray(meta[:, 2]))
            gather = K.window_gather_mc if self.split else K.window_gather_mv
            return gather(self.cond, self.tgt, torch.from_numpy(times), torch.from_numpy(meta), self.csel, h, w)
        it = self.sampler.items(indices)
        self.last_row0 = row0_of(it)
        n = it.shape[0]
        host = self._items_host[:n]
        host.copy_(torch.from_numpy(it))
        dev_items = host.to(self.device, non_blocking=True)
        return K.window_gather(self.cond, self.tgt, dev_items, self.sampler.K, h, w, self.sampler.center)

    def __iter__(self):
        for b in shard_indices(len(self.sampler), self.bs, self.rank, self.world, self.shuffle, self.seed,
                               self.epoch):
            cw, x0 = self.batch(b)
            yield cw, x0


class PinnedWindowLoader:
    """Host-resident fields; host gather into pinned double-buffers, H2D on a side stream; the same fields, arguments
    and batches as DeviceWindowLoader.
    last_row0: the crop row offsets (row0_of) of the batch last yielded, not of the one being prefetched."""

    def __init__(self, cond, tgt, K, batch_size, device, center=True, crop_hw=None, crop_mode="random",
                 time_reverse_p=0.5, shuffle=True, seed=0, rank=0, world=1, *, cond_select=None,
                 sample_mode="consecutive", window_radius=5, keep_chronology=True, causal=False, allow_replace=False,
                 cond_channels=None):
        cond, tgt, single = _fields_5d(cond, tgt)
        self.legacy = single and sample_mode == "consecutive" and cond_channels is None
        if single and not self.legacy:
            cond, tgt = cond[:, :, None], tgt[:, :, None]
        self.cond, self.tgt = cond, tgt
        T, M, H, W = cond.shape[0], cond.shape[1], cond.shape[-2], cond.shape[-1]
        V = 1 if self.legacy else tgt.shape[2]
        self.csel = None if self.legacy else resolve_cond_select(cond_select, cond.shape[2], V, cond_channels)
        Cc = V if self.legacy else len(self.csel)
        self.sampler = WindowSampler(T, M, H, W, K, center, crop_hw, crop_mode, time_reverse_p, sample_mode,
                                     window_radius=window_radius, keep_chronology=keep_chronology, causal=causal,
                                     allow_replace=allow_replace)
        self.bs, self.device = batch_size, device
        self.shuffle, self.seed, self.rank, self.world = shuffle, seed, rank, world
        self.epoch = 0
        h, w = self.sampler.hw
        self.stream = torch.cuda.Stream(device=device)
        self.host = [(torch.empty((batch_size, Cc, K, h, w)).pin_memory(),
                      torch.empty((batch_size, V, h, w)).pin_memory()) for _ in range(2)]
        self.dev = [(torch.empty((batch_size, Cc, K, h, w), device=device),
                     torch.empty((batch_size, V, h, w), device=device)) for _ in range(2)]
        self.done = [None, None]
        self.last_row0 = torch.zeros(0, dtype=torch.int64)

    def set_epoch(self, e):
        self.epoch = e

    def _draw_and_fill(self, slot, indices):
        """draws the items of one batch and gathers them into the slot's host buffers; returns (n, row0)"""
        hc, hx = self.host[slot]
        h, w = self.sampler.hw
        if self.legacy:
            items = self.sampler.items(indices)
            host_gather(self.cond, self.tgt, items, self.sampler.K, h, w, self.sampler.center, hc.numpy(), hx.numpy())
            return items.shape[0], row0_of(items)
        times, meta = self.sampler.draw(indices)
        host_gather_mv(self.cond, self.tgt, times, meta, self.csel, h, w, hc.numpy(), hx.numpy())
        return meta.shape[0], torch.from_numpy(np.ascontiguousarray(meta[:, 2]))

    def __iter__(self):
        batches = shard_indices(len(self.sampler), self.bs, self.rank, self.world, self.shuffle, self.seed,
                                self.epoch)
        main = torch.cuda.current_stream(self.device)

        def issue(k):
            slot = k % 2
            if self.done[slot] is not None:
                self.done[slot].synchronize()  # host buffer free once its previous copy finished
            n, row0 = self._draw_and_fill(slot, batches[k])
            with torch.cuda.stream(self.stream):
                self.stream.wait_stream(main)  # device buffer no longer read by compute
                dc, dx = self.dev[slot]
                hc, hx = self.host[slot]
                dc[:n].copy_(hc[:n], non_blocking=True)
                dx[:n].copy_(hx[:n], non_blocking=True)
                ev = torch.cuda.Event()
                ev.record(self.stream)
            self.done[slot] = ev
            return slot, n, row0

        if not batches:
            return
        pending = issue(0)
        for k in range(len(batches)):
            slot, n, row0 = pending
            main.wait_event(self.done[slot])
            if k + 1 < len(batches):
                pending = issue(k + 1)  # overlaps the consumer's compute on batch k
            dc, dx = self.dev[slot]
            self.last_row0 = row0
            yield dc[:n], dx[:n]


def loader_from_config(cfg, cond, tgt, device, kind="device", cond_select=None, shuffle=True, rank=0, world=1,
                       cond_channels=None):
    """The loader of a config (config/baseline, config/more_blocks): window and sampling options from cfg["dataset"]
    (K, center, crop_hw, crop_mode, time_reverse_p, sample_mode and, where present, window_radius, keep_chronology,
    causal, allow_replace), batch_size and seed from cfg["train"].  kind: "device" (DeviceWindowLoader) or "pinned"
    (PinnedWindowLoader); cond / tgt as those take them, e.g. from load_fields.  cond_channels: None reads
    cfg["unet"]["cond_channels"] where the config has one (the model's), else as the loaders take it."""
    kinds = {"device": DeviceWindowLoader, "pinned": PinnedWindowLoader}
    if kind not in kinds:
        raise ValueError(f"kind must be 'device' or 'pinned', got {kind!r}")
    ds, tr = cfg["dataset"], cfg.get("train", {})
    extra = {k: ds[k] for k in ("window_radius", "keep_chronology", "causal", "allow_replace") if k in ds}
    if cond_channels is None:
        cond_channels = cfg.get("unet", {}).get("cond_channels")
    if cond_channels is not None:
        extra["cond_channels"] = cond_channels
    return kinds[kind](cond, tgt, ds["K"], tr.get("batch_size", 1), device, center=ds.get("center", True),
                       crop_hw=tuple(ds["crop_hw"]) if ds.get("crop_hw") else None,
                       crop_mode=ds.get("crop_mode", "random"), time_reverse_p=ds.get("time_reverse_p", 0.5),
                       shuffle=shuffle, seed=tr.get("seed", 0), rank=rank, world=world, cond_select=cond_select,
                       sample_mode=ds.get("sample_mode", "consecutive"), **extra)
