"""Training-image input pipeline: UnsupervisedDataset (lib/dataset.py:86-127)
with the per-image augmentation on the GPU.

Host: glob the roots like the reference (`*.*g` at every depth), decode + Resize with PIL
(torchvision's Resize on a PIL image is PIL's bilinear resize, so this step is the
reference's own code path) in a thread pool that prefetches the next batch while the
current step runs; the uint8 HWC batch goes to HBM from pinned memory.

GPU (`pg_augment_u8`, pggan_amd/csrc/augment.hip): RandomHorizontalFlip(0.5),
ColorJitter(0.2, 0.2, 0.2, 0.01), ToTensor, Normalize(0.5, 0.5) in one pass over the
batch (three launches).  The random parameters are drawn on the host with a torch CPU
generator in torchvision's call order per image -- `torch.rand(1) < p` for the flip, then
ColorJitter.get_params: `torch.randperm(4)`, brightness, contrast, saturation, hue
`torch.empty(1).uniform_(lo, hi)` -- so a generator in the same state draws the same
parameters as the reference's transform.  The jitter is the reference's PIL path
(ImageEnhance blends and PIL's uint8 HSV hue shift, uint8 after every op) in Pillow's own
arithmetic: the output equals the reference transform byte for byte (tests/test_augment.py).

HBM cache (`HbmImageCache`): decode + Resize is deterministic and runs before every random
op (lib/dataset.py:102-112), so the resized uint8 image of a dataset index is the same in
every epoch.  The loader keeps it in HBM after its first decode (per stage: the target size
changes with the stage) and gathers later batches from there, so after the first epoch the
host decode -- 344 img/s from 1024^2 PNG on the box's 16 threads, below the step's rate at
every stage (profiles/r4_loader.json) -- no longer bounds training.  The bytes the augmentation
reads are the ones it would have decoded, so the output stays byte-exact.  Sizes: 3 S^2 bytes
per image (3 MiB at 1024^2, 192 KiB at 256^2); a DP rank caches only its own shard.

Source cache (`HbmSourceCache`, config hbm_source_cache_gb, opt-in): the cache above starts
empty at every stage, so the first epoch of each of the 9 stages decodes every file again, and
only the Resize differs.  With the source cache the decoded image is kept at source size in HBM
too, and a stage's image comes from `pg_resize_bilinear_u8` (pggan_amd/csrc/resize.hip): Pillow's
8-bit BILINEAR resize is integer arithmetic on fixed-point coefficient tables (`resize_coeffs`
builds them in float64 as libImaging/Resample.c does), so the kernel's bytes are PIL's
(tests/test_gpu_resize.py) and no stage after the first touches the disk or the host threads.
"""
from __future__ import annotations

import functools
import glob
import math
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

# ColorJitter(0.2, 0.2, 0.2, 0.01) ranges (lib/dataset.py:110), flip probability (:108)
JITTER = dict(brightness=(0.8, 1.2), contrast=(0.8, 1.2), saturation=(0.8, 1.2), hue=(-0.01, 0.01))
FLIP_P = 0.5
PSTRIDE = 12   # floats per image in the pg_augment_u8 parameter table


def image_paths(roots):
    """lib/dataset.py:89-99: `*.*g` directly under each root and in every subdirectory."""
    paths = []
    for r in roots or []:
        paths += glob.glob(f"{r}/*.*g")
        for root, dirs, _ in os.walk(r):
            for d in dirs:
                paths += glob.glob(f"{root}/{d}/*.*g")
    return paths


def load_u8(path, size):
    """Decode + Resize((size, size)) (lib/dataset.py:107) -> uint8 [size, size, 3]."""
    from PIL import Image
    im = Image.open(path).convert("RGB").resize((size, size), Image.BILINEAR)
    return np.asarray(im, dtype=np.uint8)


def load_src_u8(path):
    """Decode only -> uint8 [H, W, 3] at the file's own size (what load_u8 resizes)."""
    from PIL import Image
    return np.array(Image.open(path).convert("RGB"), dtype=np.uint8)   # a writable copy: pinned next


def image_size(path):
    """(H, W) from the file's header; nothing is decoded."""
    from PIL import Image
    with Image.open(path) as im:
        w, h = im.size
    return h, w


RESIZE_BITS = 32 - 8 - 2   # Pillow's PRECISION_BITS: 8-bit pixels, 2 bits of headroom


@functools.lru_cache(maxsize=None)
def resize_coeffs(in_size, out_size):
    """The coefficient tables of Pillow's 8-bit BILINEAR resize of one axis, in_size ->
    out_size (libImaging/Resample.c precompute_coeffs + normalize_coeffs_8bpc, operation for
    operation in float64: Python floats are C doubles) -> (k int32 [out, ksize], bounds int32
    [out, 2] = (first tap, tap count)); taps past the count are 0.  Output pixel xx is
    clip8((2^21 + sum_x pixel[xmin + x] * k[xx, x]) >> 22)."""
    scale = in_size / out_size
    fs = max(scale, 1.0)
    support = fs                       # bilinear: support 1.0 * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    k = np.zeros((out_size, ksize), np.int32)
    bounds = np.zeros((out_size, 2), np.int32)
    for xx in range(out_size):
        c = (xx + 0.5) * scale
        xmin = max(int(c - support + 0.5), 0)
        xmax = min(int(c + support + 0.5), in_size) - xmin
        w = [max(0.0, 1.0 - abs((x + xmin - c + 0.5) / fs)) for x in range(xmax)]
        ww = 0.0
        for v in w:
            ww += v
        for x, v in enumerate(w):
            if ww != 0.0:
                v /= ww
            k[xx, x] = int(0.5 + v * (1 << RESIZE_BITS))
        bounds[xx] = (xmin, xmax)
    k.setflags(write=False)
    bounds.setflags(write=False)
    return k, bounds


_DEV_COEFFS = {}   # (in, out, device) -> the tables on the device, uploaded once


def device_resize_coeffs(in_size, out_size, device):
    """resize_coeffs(in_size, out_size) as device tensors; None when the axis keeps its size
    (Pillow skips that pass)."""
    if in_size == out_size:
        return None
    key = (in_size, out_size, str(device))
    t = _DEV_COEFFS.get(key)
    if t is None:
        k, b = resize_coeffs(in_size, out_size)
        t = _DEV_COEFFS[key] = (torch.from_numpy(k.copy()).to(device),
                                torch.from_numpy(b.copy()).to(device))
    return t


def draw_params(B, gen):
    """Per-image flip / ColorJitter parameters in torchvision's draw order -> fp32 [B, 12]:
    {flip, brightness, contrast, saturation, hue, fn_idx[4], 1 - contrast, 1 - saturation, 0}
    (the last three are not read by the PIL-path kernel; the table layout is the ABI's)."""
    p = np.zeros((B, PSTRIDE), np.float32)
    for b in range(B):
        flip = bool(torch.rand(1, generator=gen) < FLIP_P)
        fn_idx = torch.randperm(4, generator=gen)
        f = [float(torch.empty(1).uniform_(*JITTER[k], generator=gen))
             for k in ("brightness", "contrast", "saturation", "hue")]
        p[b, 0] = 1.0 if flip else 0.0
        p[b, 1:5] = f
        p[b, 5:9] = fn_idx.numpy()
        p[b, 9] = 1.0 - f[1]
        p[b, 10] = 1.0 - f[2]
    return p


class ImageFolderDataset:
    """The image list of UnsupervisedDataset; `load(i)` decodes + resizes one image."""

    def __init__(self, roots, scale_index=0):
        self.paths = image_paths(roots)
        self.size = 2 ** (scale_index + 2)

    def __len__(self):
        return len(self.paths)

    def load(self, i):
        return load_u8(self.paths[i], self.size)

    def load_src(self, i):
        return load_src_u8(self.paths[i])


class HbmImageCache:
    """The decoded + resized uint8 images of one dataset at one size, in HBM: slot table
    (dataset index -> row of `buf`, -1 = not cached) and rows filled in first-decode order
    until `budget_bytes` is used (the rest is decoded on the host every time)."""

    def __init__(self, n, size, device, budget_bytes):
        per = 3 * size * size
        self.cap = int(max(0, min(n, budget_bytes // per)))
        self.size = size
        self.slot = np.full(n, -1, dtype=np.int64)
        self.used = 0
        self.buf = (torch.empty(self.cap, size, size, 3, dtype=torch.uint8, device=device)
                    if self.cap else None)

    def slots(self, idx):
        return [int(self.slot[i]) for i in idx]

    def insert(self, idx, dev_imgs):
        """Store rows dev_imgs[k] (uint8 [m, S, S, 3] on the device) for dataset indices idx
        while there is room; returns how many were stored."""
        k = 0
        for j, i in enumerate(idx):
            if self.slot[i] >= 0 or self.used >= self.cap:
                continue
            self.buf[self.used].copy_(dev_imgs[j])
            self.slot[i] = self.used
            self.used += 1
            k += 1
        return k


class HbmSourceCache:
    """The decoded RGB images of a dataset at their source size, in HBM: one flat uint8 buffer
    of `budget_bytes`, images keyed by path at 16-byte aligned offsets in first-decode order
    until the budget is used.  Room is reserved from the header's size when a decode is
    submitted (`reserve`), the pixels arrive later (`fill`); an image that no longer fits is
    not cached and keeps the host path.  The cache belongs to the model, not to a stage: every
    stage's BatchLoader resizes from it on the GPU (pg_resize_bilinear_u8)."""

    ALIGN = 16

    def __init__(self, device, budget_bytes):
        self.dev = torch.device(device)
        self.budget = int(max(0, budget_bytes))
        self.buf = torch.empty(self.budget, dtype=torch.uint8, device=self.dev)
        self.entries = {}    # path -> [offset, H, W, filled]
        self.used = 0        # bytes reserved so far (the next offset)

    def reserve(self, path, size_fn=image_size):
        """The entry of `path`, reserving room for it on first sight; None if it does not fit."""
        e = self.entries.get(path)
        if e is None:
            h, w = size_fn(path)
            nbytes = 3 * h * w
            if self.used + nbytes > self.budget:
                return None
            e = self.entries[path] = [self.used, h, w, False]
            self.used = (self.used + nbytes + self.ALIGN - 1) // self.ALIGN * self.ALIGN
        return e

    def filled(self, path):
        e = self.entries.get(path)
        return e is not None and e[3]

    def fill(self, path, dev_img):
        """Store the decoded image (uint8 [H, W, 3] on the device) in its reserved slot."""
        off, h, w, _ = e = self.entries[path]
        if tuple(dev_img.shape) != (h, w, 3):
            raise RuntimeError(f"pggan_amd: {path} decodes to {tuple(dev_img.shape)}, its header "
                               f"said {(h, w, 3)}")
        self.buf[off:off + 3 * h * w].copy_(dev_img.reshape(-1), non_blocking=True)
        e[3] = True


def default_cache_bytes(device, fraction=0.4):
    """HBM for the image cache: `fraction` of the device's free memory now."""
    dev = torch.device(device)
    if dev.type != "cuda":
        return 0
    free, _ = torch.cuda.mem_get_info(dev)
    return int(free * fraction)


class BatchLoader:
    """Decode/resize in `workers` host threads (PIL releases the GIL), one batch ahead;
    flip + jitter + normalize on the GPU.  `next(indices, prefetch=None)` returns the fp32
    NCHW [-1, 1] batch on `device` and starts decoding `prefetch` (the next indices).
    cache_bytes > 0: decoded images are kept in an HbmImageCache and later batches gather
    them there (no decode, no host-to-device copy); None: default_cache_bytes.
    source_cache: an HbmSourceCache shared by the loaders of every stage.  An image with a slot
    there is decoded at most once per run, without the resize; its stage-size image comes from
    `ops.resize_u8` straight into the batch (one call per distinct source shape), with the same
    bytes as the host's PIL resize.  An image without room there takes the host path."""

    def __init__(self, dataset, device, ops, seed=0, workers=None, gen=None, cache_bytes=None,
                 source_cache=None):
        """gen: the torch CPU generator the augmentation parameters are drawn from (shared
        across the loaders of successive stages); default a new one seeded with `seed`."""
        self.ds, self.dev, self.ops = dataset, torch.device(device), ops
        if not hasattr(ops, "augment_u8"):
            raise RuntimeError("pggan_amd: the input pipeline needs the HIP library (augment_u8)")
        if source_cache is not None and not hasattr(ops, "resize_u8"):
            raise RuntimeError("pggan_amd: the source cache needs the HIP library (resize_u8)")
        self.src_cache = source_cache
        self._rws = None
        self.pool = ThreadPoolExecutor(max_workers=workers or min(16, os.cpu_count() or 1))
        self.gen = gen if gen is not None else torch.Generator().manual_seed(seed)
        self._pending = {}       # dataset index -> future of its decoded image
        self._ws = None
        # the cache is allocated at the SECOND batch: the first one is drawn before the stage's
        # training step has allocated its buffers (ProgressiveGAN.train_step builds the engine
        # after load_next_batch), so a default budget sized from free memory then would take
        # memory the step needs.  cache_bytes=0 turns it off (opt-out).
        self._cache_bytes = cache_bytes
        self._calls = 0
        self.cache = None
        self.decoded = 0         # images decoded on the host so far

    def _make_cache(self):
        b = self._cache_bytes
        if b is None:
            b = default_cache_bytes(self.dev)
        if b > 0:
            self.cache = HbmImageCache(len(self.ds), self.ds.size, self.dev, b)

    def _cached(self, i):
        return self.cache is not None and self.cache.slot[i] >= 0

    def _submit(self, idx):
        """Start what index i still needs from the host: nothing (cached at this stage, or its
        source is in HBM), the decode alone (a source slot to fill), or decode + resize."""
        for i in idx:
            i = int(i)
            if i in self._pending or self._cached(i):
                continue
            if self.src_cache is not None:
                path = self.ds.paths[i]
                if self.src_cache.filled(path):
                    continue
                if self.src_cache.reserve(path) is not None:
                    self._pending[i] = (True, self.pool.submit(self.ds.load_src, i))
                    continue
            self._pending[i] = (False, self.pool.submit(self.ds.load, i))

    def _upload(self, arr):
        t = torch.from_numpy(arr)
        if self.dev.type == "cuda":
            t = t.pin_memory()
        return t.to(self.dev, non_blocking=True)

    def _resize_from_source(self, rows, idx, src):
        """Rows `rows` of the batch `src` [B, S, S, 3] from the source cache: one resize_u8
        call per distinct source shape."""
        S, sc = self.ds.size, self.src_cache
        groups = {}
        for k in rows:
            off, h, w, _ = sc.entries[self.ds.paths[idx[k]]]
            groups.setdefault((h, w), []).append((off, k * 3 * S * S))
        for (h, w), offs in groups.items():
            so = torch.tensor([o for o, _ in offs], dtype=torch.int64).to(self.dev)
            do = torch.tensor([d for _, d in offs], dtype=torch.int64).to(self.dev)
            self._rws = self.ops.resize_u8(sc.buf, so, h, w, S,
                                           device_resize_coeffs(w, S, self.dev),
                                           device_resize_coeffs(h, S, self.dev), src, do,
                                           ws=self._rws)

    def next(self, idx, prefetch=None):
        if self._calls == 1:
            self._make_cache()
        self._calls += 1
        idx = [int(i) for i in idx]
        self._submit(idx)
        B, S = len(idx), self.ds.size
        miss = [k for k, i in enumerate(idx) if not self._cached(i)]
        src = torch.empty(B, S, S, 3, dtype=torch.uint8, device=self.dev)
        if miss:
            got = {k: self._pending.pop(idx[k]) for k in miss if idx[k] in self._pending}
            self.decoded += len(got)
            for k, (is_src, fut) in got.items():        # decoded at source size: into its slot
                if is_src and not self.src_cache.filled(self.ds.paths[idx[k]]):
                    self.src_cache.fill(self.ds.paths[idx[k]], self._upload(fut.result()))
            host_rows = [k for k, (is_src, _) in got.items() if not is_src]
            gpu_rows = [k for k in miss if k not in host_rows]
            if gpu_rows:
                self._resize_from_source(gpu_rows, idx, src)
            if host_rows:
                dev_miss = self._upload(np.stack([got[k][1].result() for k in host_rows]))
                src[torch.tensor(host_rows, device=self.dev)] = dev_miss
            if self.cache is not None:
                self.cache.insert([idx[k] for k in miss], [src[k] for k in miss])
        self._gather_cached([k for k in range(B) if k not in miss], idx, src)
        if prefetch is not None:
            self._submit(prefetch)
        return self._augment(src)

    def _gather_cached(self, hit, idx, src):
        """Rows `hit` of the batch `src` from the stage's cache."""
        if hit:
            rows = torch.tensor([int(self.cache.slot[idx[k]]) for k in hit], device=self.dev)
            if len(hit) == src.shape[0]:
                torch.index_select(self.cache.buf, 0, rows, out=src)
            else:
                src[torch.tensor(hit, device=self.dev)] = self.cache.buf.index_select(0, rows)

    def raw_u8(self, idx):
        """The un-augmented images of `idx`, uint8 [B, S, S, 3] on the device: byte for byte
        what next() augments, from wherever it is already (the stage's cache, the source cache
        through resize_u8), else decoded now.  A read-only side door (nearest-neighbour search
        over the training set): draws nothing from `gen`, counts as no call, fills neither
        cache and leaves the pending prefetches alone."""
        idx = [int(i) for i in idx]
        B, S = len(idx), self.ds.size
        src = torch.empty(B, S, S, 3, dtype=torch.uint8, device=self.dev)
        hit = [k for k in range(B) if self._cached(idx[k])]
        gpu_rows = [k for k in range(B) if k not in hit and self.src_cache is not None and
                    self.src_cache.filled(self.ds.paths[idx[k]])]
        host_rows = [k for k in range(B) if k not in hit and k not in gpu_rows]
        if gpu_rows:
            self._resize_from_source(gpu_rows, idx, src)
        if host_rows:
            arrs = list(self.pool.map(self.ds.load, [idx[k] for k in host_rows]))
            src[torch.tensor(host_rows, device=self.dev)] = self._upload(np.stack(arrs))
        self._gather_cached(hit, idx, src)
        return src

    def _augment(self, src):
        """Flip + jitter + normalize of a uint8 batch, parameters from `gen`."""
        B, S = src.shape[0], src.shape[1]
        params = torch.from_numpy(draw_params(B, self.gen)).to(self.dev, non_blocking=True)
        out = torch.empty(B, 3, S, S, dtype=torch.float32, device=self.dev)
        self._ws = self.ops.augment_u8(src, params, out, ws=self._ws)
        return out

    def close(self):
        """Stop the decode threads; pending prefetches are cancelled; the stage's cache is
        freed (a source cache stays with its owner; a slot reserved there for a cancelled
        decode is filled by the next loader that asks for the image)."""
        self._pending = {}
        self.cache = None
        self.pool.shutdown(wait=False, cancel_futures=True)
