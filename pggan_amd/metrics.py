"""Validation metric: the PGGAN paper's sliced Wasserstein distance (SWD) between two image
sets, on 7x7x3 patches of the Laplacian pyramid (Karras et al. 2018, section 5 / appendix;
DESIGN.md "Validation: sliced Wasserstein distance").

The pyramid, the patch gather (with the Laplacian evaluated at the patch pixels only), the
per-channel statistics, the projections and the sorted-L1 sum run in the library
(csrc/swd.hip through the op set's swd_* methods).  The host side owns the bookkeeping and
the random draws -- patch centres and directions, from seeded torch CPU generators -- and
calls torch.sort for the sort.

    m = SlicedWasserstein(ops, 256, 4096)
    for batch in reals: m.feed("real", batch)      # fp32 [B, 3, 256, 256] in [-1, 1]
    for batch in fakes: m.feed("fake", batch)
    m.result()   # {256: v, 128: v, 64: v, 32: v, 16: v, "avg": v}, x 1e3 as the paper prints

And the paper's second figure, the multi-scale structural similarity between pairs of images of
one set (MultiScaleSSIM below; csrc/msssim.hip through the op set's msssim_* methods).

And its nearest-neighbour figure: the training images closest to given images in pixel space
(NearestNeighbours below; csrc/nn.hip through the op set's nn_* methods).

And, beyond the paper, the radial power spectrum of a set of images, the network-free check of
a generator's high frequencies (PowerSpectrum below; csrc/spectrum.hip through the op set's
spectrum_profile).
"""
from __future__ import annotations

import functools

import numpy as np
import torch

DESC = 147                   # 7 x 7 x 3 values per descriptor
SETS = ("real", "fake")
SORT_INDEX_BYTES = 1 << 30   # torch.sort also returns int64 indices: rows are sorted in chunks


def _mix(*key):
    """One 63-bit generator seed from a tuple of small non-negative integers."""
    h = 0x9E3779B97F4A7C15
    for k in key:
        h = ((h ^ (int(k) + 0x632BE59BD9B4E019)) * 0xFF51AFD7ED558CCD) % (1 << 64)
        h ^= h >> 32
    return h >> 1


def draw_positions(seed, level, first, count, size, per_image):
    """Patch centres (y, x), uniform in [3, size - 3), of images first .. first + count - 1 of
    a set at pyramid level `level`: int32 [count * per_image, 2].  Every image has its own
    stream keyed by (seed, level, index of the image in its set), so how the images are
    batched does not matter.  Image i of the reals and image i of the fakes get the same
    centres (common random numbers: no bias, less variance, and two identical sets are at
    distance exactly 0)."""
    g = torch.Generator()
    out = torch.empty(count, per_image, 2, dtype=torch.int32)
    for i in range(count):
        g.manual_seed(_mix(seed, 1, level, first + i))
        out[i] = torch.randint(3, size - 3, (per_image, 2), generator=g, dtype=torch.int32)
    return out.view(-1, 2)


def draw_directions(seed, repeats, dirs):
    """fp32 [repeats, 147, dirs]: N(0, 1) columns scaled to unit L2 norm, drawn and normalised
    in float64."""
    g = torch.Generator().manual_seed(_mix(seed, 2))
    d = torch.randn(repeats, DESC, dirs, generator=g, dtype=torch.float64)
    return (d / d.square().sum(dim=1, keepdim=True).sqrt()).float()


class SlicedWasserstein:
    """SWD x 1e3 per pyramid level (resolution .. 16) between `n_images` reals and as many
    fakes.  Memory: two [n_images * per_image, 147] fp32 descriptor buffers per level
    (1.2 GB each at the paper's 16384 images) and, in result(), two [dirs, n] projections."""

    def __init__(self, ops, resolution, n_images, nhood=7, per_image=128, repeats=4, dirs=128,
                 seed=0, quantize=True):
        R = int(resolution)
        if R < 16 or R & (R - 1):
            raise ValueError(f"SlicedWasserstein: resolution must be a power of two >= 16, got {R}")
        if nhood != 7:
            raise ValueError("SlicedWasserstein: the kernels gather 7x7 neighbourhoods (nhood=7)")
        if min(n_images, per_image, repeats, dirs) < 1:
            raise ValueError("SlicedWasserstein: n_images, per_image, repeats, dirs must be >= 1")
        self.ops, self.R, self.n_images, self.K = ops, R, int(n_images), int(per_image)
        self.repeats, self.P, self.seed, self.quantize = int(repeats), int(dirs), int(seed), bool(quantize)
        self.sizes = [R >> l for l in range(R.bit_length() - 4)]       # R, R/2, .., 16
        self.device = None               # that of the first images fed
        self.count = {w: 0 for w in SETS}
        self.desc = self.dirs = None
        self._pyr = []

    def _alloc(self, device):
        self.device = device
        n = self.n_images * self.K
        self.desc = {w: [torch.empty(n, DESC, dtype=torch.float32, device=device)
                         for _ in self.sizes] for w in SETS}
        self.dirs = draw_directions(self.seed, self.repeats, self.P).to(device)

    def feed(self, which, images):
        if which not in SETS:
            raise ValueError(f"SlicedWasserstein.feed: which must be one of {SETS}, got {which!r}")
        if images.dim() != 4 or tuple(images.shape[1:]) != (3, self.R, self.R):
            raise ValueError(f"SlicedWasserstein.feed: expected [B, 3, {self.R}, {self.R}], got "
                             f"{tuple(images.shape)}")
        B, first = images.shape[0], self.count[which]
        if first + B > self.n_images:
            raise ValueError(f"SlicedWasserstein.feed: {first} + {B} {which} images exceed "
                             f"n_images = {self.n_images}")
        if B == 0:
            return
        if self.desc is None:
            self._alloc(images.device)
        x = images.detach().to(torch.float32).contiguous()
        if not self._pyr or self._pyr[0].shape[0] < B:
            self._pyr = [torch.empty(B, 3, s, s, dtype=torch.float32, device=self.device)
                         for s in self.sizes[1:]]
        pyr = [x] + [t[:B] for t in self._pyr]
        for l in range(len(self.sizes) - 1):
            self.ops.swd_pyr_down(pyr[l], pyr[l + 1], self.quantize and l == 0)
        for l, s in enumerate(self.sizes):
            pos = draw_positions(self.seed, l, first, B, s, self.K)
            if int(pos.min()) < 3 or int(pos.max()) >= s - 3:     # the kernel trusts them
                raise ValueError(f"SlicedWasserstein.feed: patch centres outside [3, {s - 3})")
            pos = pos.to(self.device)
            coarse = pyr[l + 1] if l + 1 < len(self.sizes) else None
            out = self.desc[which][l][first * self.K:(first + B) * self.K]
            self.ops.swd_descriptors(pyr[l], coarse, pos, out, self.K, self.quantize and l == 0)
        self.count[which] = first + B

    def result(self):
        for w in SETS:
            if self.count[w] != self.n_images:
                raise RuntimeError(f"SlicedWasserstein.result: {self.count[w]} of {self.n_images} "
                                   f"{w} images fed")
        n, P, dev = self.n_images * self.K, self.P, self.device
        acc = torch.zeros(len(self.sizes), dtype=torch.float32, device=dev)
        stat = torch.empty(4, 3, dtype=torch.float32, device=dev)
        proj = [torch.empty(P, n, dtype=torch.float32, device=dev) for _ in SETS]
        rows = max(1, SORT_INDEX_BYTES // (8 * n))
        for l in range(len(self.sizes)):
            for k, w in enumerate(SETS):
                self.ops.swd_stats(self.desc[w][l], stat[2 * k], stat[2 * k + 1])
            for r in range(self.repeats):
                for k, w in enumerate(SETS):
                    self.ops.swd_project(self.desc[w][l], stat[2 * k], stat[2 * k + 1],
                                         self.dirs[r], proj[k])
                for r0 in range(0, P, rows):
                    a, b = (torch.sort(t[r0:r0 + rows], dim=1).values for t in proj)
                    self.ops.swd_l1(a, b, n, acc[l:l + 1])
        vals = [float(v) / (self.repeats * P * n) * 1e3 for v in acc.cpu().tolist()]
        out = dict(zip(self.sizes, vals))
        out["avg"] = sum(vals) / len(vals)
        return out


# ---------------------------------------------------------------------------------- MS-SSIM
MSSSIM_SCALES = 5
MSSSIM_WINDOW = 11           # taps per axis at scales of at least that side
MSSSIM_SIGMA = 1.5           # of the 11-tap window; shorter windows scale it with their length


def msssim_taps(size):
    """The 1-D Gaussian window of a scale of side `size`: T = min(11, size) taps centred on
    (T - 1) / 2 (half-integer positions for an even T), sigma = 1.5 T / 11, normalised to sum 1
    in float64; returned as fp32 (what the kernel takes)."""
    T = min(MSSSIM_WINDOW, int(size))
    sigma = MSSSIM_SIGMA * T / MSSSIM_WINDOW
    d = np.arange(T, dtype=np.float64) - (T - 1) / 2.0
    g = np.exp(-d * d / (2.0 * sigma * sigma))
    return (g / g.sum()).astype(np.float32)


class MultiScaleSSIM:
    """The PGGAN paper's diversity figure: multi-scale structural similarity (Wang et al. 2003;
    five scales, 11x11 Gaussian windows, 8-bit images) between `n_pairs` pairs of images of one
    stream, consecutive images paired (0,1), (2,3), ..  (DESIGN.md "Validation: MS-SSIM").
    Every scale is one launch of the library (csrc/msssim.hip through the op set's msssim_*
    methods) that also writes the next scale's 2x2-pooled pair; the host side pairs the images up.

        m = MultiScaleSSIM(ops, 256, 10000)
        for batch in fakes: m.feed(batch)       # fp32 [B, 3, 256, 256] in [-1, 1]
        m.result()                              # mean over the pairs, in [0, 1]

    quantize=False takes the images as they are, on the 0..255 scale.  Work buffers: the four
    pooled scales of a batch's pairs, allocated once for the largest batch seen."""

    def __init__(self, ops, resolution, n_pairs, quantize=True):
        R = int(resolution)
        if R < 16 or R & (R - 1):
            raise ValueError(f"MultiScaleSSIM: resolution must be a power of two >= 16, got {R}")
        if int(n_pairs) < 1:
            raise ValueError("MultiScaleSSIM: n_pairs must be >= 1")
        self.ops, self.R, self.n_pairs, self.quantize = ops, R, int(n_pairs), bool(quantize)
        self.sizes = [R >> s for s in range(MSSSIM_SCALES)]
        self.taps = [msssim_taps(s) for s in self.sizes]
        self.counts = [3 * (s - len(t) + 1) ** 2 for s, t in zip(self.sizes, self.taps)]
        self.fed = 0                 # images taken so far, the held one included
        self.sums = None             # [5, n_pairs, 2] on the device of the first images fed
        self._held = None            # a trailing odd image waiting for its partner
        self._pool = []              # per later scale [2, P, 3, S, S] for the largest P seen

    def feed(self, images):
        if images.dim() != 4 or tuple(images.shape[1:]) != (3, self.R, self.R):
            raise ValueError(f"MultiScaleSSIM.feed: expected [B, 3, {self.R}, {self.R}], got "
                             f"{tuple(images.shape)}")
        B = images.shape[0]
        if self.fed + B > 2 * self.n_pairs:
            raise ValueError(f"MultiScaleSSIM.feed: {self.fed} + {B} images exceed 2 * n_pairs = "
                             f"{2 * self.n_pairs}")
        if B == 0:
            return
        x = images.detach().to(torch.float32)
        if self.sums is None:
            self.sums = torch.zeros(MSSSIM_SCALES, self.n_pairs, 2, dtype=torch.float32,
                                    device=x.device)
        first = (self.fed - (self._held is not None)) // 2      # pairs done so far
        if self._held is not None:
            x = torch.cat([self._held, x])
            self._held = None
        self.fed += B
        P = x.shape[0] // 2
        if x.shape[0] % 2:
            self._held = x[-1:].clone()
        if P == 0:
            return
        x = x[:2 * P].contiguous()
        if not self._pool or self._pool[0].shape[1] < P:
            self._pool = [torch.empty(2, P, 3, s, s, dtype=torch.float32, device=x.device)
                          for s in self.sizes[1:]]
        a, b = x[0::2], x[1::2]
        for s in range(MSSSIM_SCALES):
            last = s == MSSSIM_SCALES - 1
            pa, pb = (None, None) if last else (self._pool[s][0, :P], self._pool[s][1, :P])
            self.ops.msssim_scale(a, b, self.taps[s], self.quantize and s == 0,
                                  self.sums[s, first:first + P], pa, pb)
            a, b = pa, pb

    def _check_full(self, what):
        if self.fed != 2 * self.n_pairs:
            raise RuntimeError(f"MultiScaleSSIM.{what}: {self.fed} of {2 * self.n_pairs} images fed")

    def values(self):
        """The per-pair values, fp32 [n_pairs]."""
        self._check_full("values")
        out = torch.empty(self.n_pairs, dtype=torch.float32, device=self.sums.device)
        self.ops.msssim_combine(self.sums, self.counts, out)
        return out

    def result(self):
        """The mean over the pairs, taken in float64."""
        self._check_full("result")
        return float(self.values().double().mean().item())


# ------------------------------------------------------------------------ nearest neighbours
NN_MAX_K = 16
NN_NONE = (1 << 63) - 1      # d^2 of a slot beyond the database size; its index is -1


class NearestNeighbours:
    """The k training images nearest to each query image: exact squared L2 between the 8-bit
    images box-pooled to `compare` x `compare`, in integers (DESIGN.md "Validation: nearest
    training images"; csrc/nn.hip through the op set's nn_* methods).  Ties go to the lower
    index; how the database is split into feeds does not matter.

        m = NearestNeighbours(ops, 256, 3)
        m.set_queries(fakes)                        # fp32 [Q, 3, 256, 256] in [-1, 1]
        for first, batch in database: m.feed(batch, first)     # or uint8 [B, 256, 256, 3]
        idx, d2 = m.result()                        # int64 [Q, k]; (-1, INT64_MAX) past the end

    Memory: the queries' rows, Q x 3 compare^2 bytes; a feed's rows live for the call."""

    def __init__(self, ops, resolution, k, compare=64):
        R, Rc, k = int(resolution), int(compare), int(k)
        if R < 8 or R & (R - 1):
            raise ValueError(f"NearestNeighbours: resolution must be a power of two >= 8, got {R}")
        if Rc < 8 or Rc > 128 or Rc & (Rc - 1) or Rc > R:
            raise ValueError(f"NearestNeighbours: compare must be a power of two in [8, "
                             f"min(128, resolution = {R})], got {Rc}")
        if k < 1 or k > NN_MAX_K:
            raise ValueError(f"NearestNeighbours: k must be in [1, {NN_MAX_K}], got {k}")
        self.ops, self.R, self.Rc, self.k, self.D = ops, R, Rc, k, 3 * Rc * Rc
        self.q = self.qsq = self.best_d2 = self.best_idx = None

    def descriptors(self, images):
        """(int8 [B, D] rows, int32 [B] sums of squares) of fp32 NCHW or uint8 NHWC images."""
        R = self.R
        ok = images.dim() == 4 and (
            (images.dtype == torch.uint8 and tuple(images.shape[1:]) == (R, R, 3)) or
            (images.dtype != torch.uint8 and tuple(images.shape[1:]) == (3, R, R)))
        if not ok:
            raise ValueError(f"NearestNeighbours: expected fp32 [B, 3, {R}, {R}] or uint8 "
                             f"[B, {R}, {R}, 3], got {images.dtype} {tuple(images.shape)}")
        x = images.detach()
        x = (x if x.dtype == torch.uint8 else x.to(torch.float32)).contiguous()
        B = x.shape[0]
        desc = torch.empty(B, self.D, dtype=torch.int8, device=x.device)
        sq = torch.empty(B, dtype=torch.int32, device=x.device)
        if B:
            self.ops.nn_descriptors(x, self.Rc, desc, sq)
        return desc, sq

    def set_queries(self, images):
        """The query images; forgets what was fed."""
        if images.dim() != 4 or images.shape[0] < 1:
            raise ValueError("NearestNeighbours.set_queries: at least one image")
        self.set_query_descriptors(*self.descriptors(images))

    def set_query_descriptors(self, desc, sq):
        """The queries as prebuilt rows (descriptors()); forgets what was fed."""
        if desc.dim() != 2 or desc.shape[0] < 1 or desc.shape[1] != self.D or \
                desc.dtype != torch.int8 or sq.dtype != torch.int32 or \
                tuple(sq.shape) != (desc.shape[0],):
            raise ValueError(f"NearestNeighbours.set_query_descriptors: expected int8 [Q, "
                             f"{self.D}] rows and int32 [Q] sums")
        self.q, self.qsq = desc.contiguous(), sq.contiguous()
        Q, dev = self.q.shape[0], self.q.device
        self.best_d2 = torch.full((Q, self.k), NN_NONE, dtype=torch.int64, device=dev)
        self.best_idx = torch.full((Q, self.k), -1, dtype=torch.int64, device=dev)

    def feed(self, images, first_index):
        """Database images with the indices first_index, first_index + 1, .."""
        desc, sq = self.descriptors(images)
        self.feed_descriptors(desc, sq, first_index)

    def feed_descriptors(self, desc, sq, first_index):
        """A prebuilt block of database rows (descriptors())."""
        if self.q is None:
            raise RuntimeError("NearestNeighbours.feed: set_queries first")
        if desc.dim() != 2 or desc.shape[1] != self.D or desc.dtype != torch.int8 or \
                sq.dtype != torch.int32 or tuple(sq.shape) != (desc.shape[0],):
            raise ValueError(f"NearestNeighbours.feed_descriptors: expected int8 [N, {self.D}] "
                             f"rows and int32 [N] sums, got {desc.dtype} {tuple(desc.shape)} and "
                             f"{sq.dtype} {tuple(sq.shape)}")
        if int(first_index) < 0:
            raise ValueError("NearestNeighbours.feed_descriptors: first_index must be >= 0")
        if desc.shape[0] == 0:
            return
        self.ops.nn_search(self.q, self.qsq, desc.contiguous(), sq.contiguous(), int(first_index),
                           self.best_d2, self.best_idx)

    def result(self):
        """(idx, d2), int64 [Q, k], nearest first."""
        if self.q is None:
            raise RuntimeError("NearestNeighbours.result: set_queries first")
        return self.best_idx, self.best_d2

    def rms(self):
        """sqrt(d2 / D), float64 [Q, k] on the CPU: the RMS pixel difference on the 0..255 scale
        (inf in the slots beyond the database size).  Taken on the host, where the square root
        is correctly rounded: the figure is a function of d2 alone, whatever ran the search."""
        idx, d2 = (t.cpu() for t in self.result())
        r = (d2.double() / self.D).sqrt()
        return torch.where(idx < 0, torch.full_like(r, float("inf")), r)


# ---------------------------------------------------------------------------- power spectrum
SPECTRUM_FLOOR = 1e-12       # a bin mean below this counts as this in the dB ratio


def spectrum_bin_index(r2):
    """The radius bin of the squared radii r2 (non-negative integers): the one k with
    k^2 - k < r2 <= k^2 + k (0 for r2 = 0): round(sqrt(r2)), decided in integers (the float
    root only proposes floor(sqrt(r2)), which is then corrected)."""
    r2 = np.asarray(r2, dtype=np.int64)
    k = np.sqrt(r2.astype(np.float64)).astype(np.int64)
    k = np.where(k * k > r2, k - 1, k)
    k = np.where((k + 1) * (k + 1) <= r2, k + 1, k)
    return np.where(r2 > k * k + k, k + 1, k)


def spectrum_bins(R):
    """int64 [R, R]: the bin of every point of the DFT plane in numpy.fft order (index i is
    the signed frequency i for i < R/2, i - R from R/2 on)."""
    f = np.arange(R, dtype=np.int64)
    f = np.where(f < R // 2, f, f - R)
    return spectrum_bin_index(f[:, None] ** 2 + f[None, :] ** 2)


@functools.lru_cache(maxsize=None)
def _spectrum_bin_counts(R):
    return np.bincount(spectrum_bins(R).ravel())[:R // 2 + 1].astype(np.int64)


def spectrum_bin_counts(R):
    """int64 [R/2 + 1]: the number of points of the R x R plane in each bin 0 .. R/2 (a
    function of R alone: computed once per R)."""
    return _spectrum_bin_counts(int(R)).copy()


def spectrum_db(S_real, S_fake):
    """10 log10(S_fake / S_real) per bin of two profiles [K + 1], either side floored at 1e-12."""
    a, b = (np.maximum(np.asarray(s, np.float64), SPECTRUM_FLOOR) for s in (S_real, S_fake))
    if a.shape != b.shape or a.ndim != 1 or a.size < 5:
        raise ValueError("spectrum_db: two profiles of one length >= 5")
    return 10.0 * np.log10(b / a)


def spectrum_compare(S_real, S_fake):
    """(dB [K], spec_dist, spec_hf) of two profiles [K + 1]: dB[k - 1] = 10 log10(S_fake[k] /
    S_real[k]) for k = 1 .. K (bin 0, the brightness, is left out; either side floored at
    1e-12), spec_dist the mean of |dB|, spec_hf the signed mean of dB over the top quarter
    k = 3K/4 + 1 .. K: positive is too much fine detail or noise, negative too little."""
    db = spectrum_db(S_real, S_fake)[1:]
    K = db.size
    return db, float(np.abs(db).mean()), float(db[3 * K // 4:].mean())


class PowerSpectrum:
    """The azimuthally averaged power spectrum of a set of images (Durall et al. 2020, "Watch
    your Up-Convolution"; DESIGN.md "Validation: power spectrum"): per image |DFT2(luma)|^2 of
    the 8-bit image summed over integer radius bins 0 .. K = R/2 in the library
    (csrc/spectrum.hip through the op set's spectrum_profile), averaged here over the images
    and the bin populations in float64.

        m = PowerSpectrum(ops, 256)
        for batch in fakes: m.feed(batch)       # fp32 [B, 3, 256, 256] in [-1, 1]
        m.profile()                             # float64 [129]; spectrum_compare(real, fake)

    quantize=False takes the images as they are, on the 0..255 scale.  The per-image profiles
    stay on the device, (K + 1) floats each."""

    def __init__(self, ops, resolution, quantize=True):
        R = int(resolution)
        if R < 8 or R > 1024 or R & (R - 1):
            raise ValueError(f"PowerSpectrum: resolution must be a power of two in [8, 1024], got {R}")
        self.ops, self.R, self.K, self.quantize = ops, R, R // 2, bool(quantize)
        self.counts = spectrum_bin_counts(R)
        self.count = 0               # images fed
        self._prof = []              # fp32 [B, K + 1] per feed

    def feed(self, images):
        if images.dim() != 4 or tuple(images.shape[1:]) != (3, self.R, self.R):
            raise ValueError(f"PowerSpectrum.feed: expected [B, 3, {self.R}, {self.R}], got "
                             f"{tuple(images.shape)}")
        B = images.shape[0]
        if B == 0:
            return
        x = images.detach().to(torch.float32).contiguous()
        out = torch.empty(B, self.K + 1, dtype=torch.float32, device=x.device)
        self.ops.spectrum_profile(x, self.quantize, out)
        self._prof.append(out)
        self.count += B

    def per_image(self):
        """The profiles as the library wrote them, fp32 [count, K + 1], in feed order."""
        if not self._prof:
            raise RuntimeError("PowerSpectrum: no image fed")
        return torch.cat(self._prof)

    def profile(self):
        """S[k]: the mean over the images of prof[k] / count[k], float64 numpy [K + 1]."""
        total = self.per_image().double().sum(dim=0).cpu().numpy()
        return total / self.count / self.counts
