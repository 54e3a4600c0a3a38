"""float64 reference of the multi-scale structural similarity of pggan_amd/metrics.py, written
from its definition with scipy (a 2-D FFT convolution and an ndimage box filter: neither the
separable passes nor the aligned 2x2 mean of the kernel), and `CpuMsssimOps`, a numpy double of
the two msssim_* ops so the host logic of MultiScaleSSIM and ProgressiveGAN.validation runs
without a GPU.

Definition (two images a, b, fp32 NCHW [3,R,R] in [-1,1], R a power of two >= 16; constants of
Wang et al. 2003 as in the evaluation script released with the PGGAN paper):
  q(x)     = rint(clip(127.5 x + 127.5, 0, 255)), ties to even (scale 0, `quantize`)
  scales   s = 0..4 of side S = R >> s; window of T = min(11, S) taps per axis, sigma = 1.5 T / 11,
             g[i] ~ exp(-(i - (T - 1) / 2)^2 / (2 sigma^2)) normalised to sum 1, 2-D window g (x) g,
             "valid" filtering F: n = S - T + 1 positions per axis
  per channel: mu1 = F(a), mu2 = F(b), s11 = F(a a) - mu1^2, s22 = F(b b) - mu2^2,
             s12 = F(a b) - mu1 mu2, c1 = 2.55^2, c2 = 7.65^2, v1 = 2 s12 + c2, v2 = s11 + s22 + c2
  ssim_s   = mean over 3 n^2 of (2 mu1 mu2 + c1) v1 / ((mu1^2 + mu2^2 + c1) v2)
  cs_s     = mean over 3 n^2 of v1 / v2
  next     = the aligned 2x2 mean of the float images (not re-quantised)
  value    = prod_{s<4} max(cs_s, 0)^w_s * max(ssim_4, 0)^w_4, w = WEIGHTS
  metric   = mean over the pairs (0,1), (2,3), .. of a stream, in float64
"""
import numpy as np
import scipy.ndimage as ndi
import scipy.signal as sig
import torch

WEIGHTS = np.array([0.0448, 0.2856, 0.3001, 0.2363, 0.1333])
C1, C2 = (0.01 * 255) ** 2, (0.03 * 255) ** 2
SCALES = 5


def quantize(x):
    return np.rint(np.clip(np.asarray(x, np.float64) * 127.5 + 127.5, 0.0, 255.0))


def taps(S, centre_shift=0.0):
    """The 1-D window of a scale of side S, float64.  centre_shift moves the centre off
    (T - 1) / 2 (only the tests' perturbed references use it)."""
    T = min(11, S)
    sigma = 1.5 * T / 11
    d = np.arange(T, dtype=np.float64) - ((T - 1) / 2.0 + centre_shift)
    g = np.exp(-d ** 2 / (2 * sigma ** 2))
    return g / g.sum()


def window2d(S, centre_shift=0.0):
    g = taps(S, centre_shift)
    return np.outer(g, g)


def filt(x, w):
    """'valid' correlation of the last two axes of x with the 2-D window w."""
    x = np.asarray(x, np.float64)
    return sig.fftconvolve(x, w[::-1, ::-1].reshape((1,) * (x.ndim - 2) + w.shape), mode="valid")


def down(x):
    x = np.asarray(x, np.float64)
    k = np.ones((1,) * (x.ndim - 2) + (2, 2)) / 4
    return ndi.convolve(x, k, mode="reflect")[..., ::2, ::2]


def scale_stats(a, b, w, drop=0):
    """(ssim, cs) means of one scale; a, b [..,3,S,S] on the 0..255 scale, w the 2-D window.
    drop > 0 leaves the last `drop` rows and columns of positions out (only the tests'
    perturbed references use it)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    mu1, mu2 = filt(a, w), filt(b, w)
    s11, s22, s12 = filt(a * a, w) - mu1 ** 2, filt(b * b, w) - mu2 ** 2, filt(a * b, w) - mu1 * mu2
    v1, v2 = 2 * s12 + C2, s11 + s22 + C2
    cs = v1 / v2
    ssim = (2 * mu1 * mu2 + C1) * v1 / ((mu1 ** 2 + mu2 ** 2 + C1) * v2)
    if drop:
        cs, ssim = cs[..., :-drop, :-drop], ssim[..., :-drop, :-drop]
    ax = (-3, -2, -1)
    return ssim.mean(axis=ax), cs.mean(axis=ax)


def combine(ssim, cs):
    """ssim, cs [5, ..] -> pair values."""
    ssim, cs = np.asarray(ssim, np.float64), np.asarray(cs, np.float64)
    v = np.ones(ssim.shape[1:])
    for s in range(SCALES):
        m = ssim[s] if s == SCALES - 1 else cs[s]
        v = v * np.maximum(m, 0.0) ** WEIGHTS[s]
    return v


def pair_values(a, b, quant=True, centre_shift=0.0, drop=0):
    """a, b [P,3,R,R] -> (values [P], ssim [5,P], cs [5,P])."""
    a = quantize(a) if quant else np.asarray(a, np.float64)
    b = quantize(b) if quant else np.asarray(b, np.float64)
    ss, cc = [], []
    for s in range(SCALES):
        S = a.shape[-1]
        ssim, cs = scale_stats(a, b, window2d(S, centre_shift if S % 2 == 0 and S < 11 else 0.0),
                               drop if S - min(11, S) + 1 > drop else 0)
        ss.append(ssim)
        cc.append(cs)
        if s + 1 < SCALES:
            a, b = down(a), down(b)
    return combine(ss, cc), np.array(ss), np.array(cc)


def msssim_reference(images, quant=True):
    """The metric over a stream [2P,3,R,R]: mean of the pair values."""
    images = np.asarray(images)
    return float(pair_values(images[0::2], images[1::2], quant)[0].mean())


def make_pairs(R, seed, P=1):
    """The GPU tests' inputs, on the 8-bit grid, as fp32 images in [-1, 1]: a = a sinusoid
    pattern plus N(0, 25), b = a + N(0, 40) (pair values 0.73 .. 0.93 at R = 16 .. 256, every
    factor >= 0.44: no clip fires, no factor is near 0)."""
    g = np.random.default_rng(seed)
    y, x = np.meshgrid(np.linspace(0, 1, R), np.linspace(0, 1, R), indexing="ij")
    k = np.arange(3).reshape(1, 3, 1, 1)
    c = g.uniform(0, 6, (P, 1, 1, 1))
    a = 127.5 + 90 * np.sin(5 * x * (k + 1) + c) * np.cos(4 * y + k) + g.normal(0, 25, (P, 3, R, R))
    a = np.rint(np.clip(a, 0, 255))
    b = np.rint(np.clip(a + g.normal(0, 40, a.shape), 0, 255))
    to = lambda u: ((u - 127.5) / 127.5).astype(np.float32)
    return to(a), to(b)


def interleave(a, b):
    out = np.empty((2 * a.shape[0],) + a.shape[1:], a.dtype)
    out[0::2], out[1::2] = a, b
    return out


def _np(t):
    return t.detach().cpu().numpy().astype(np.float64)


class CpuMsssimOps:
    """The msssim_* methods of pggan_amd._lib.HipOps on CPU tensors: the closed forms
    (separable taps, aligned 2x2 mean) in float64, results rounded once into the fp32 outputs.
    A mix-in (tests combine it with cpu_ops.CpuOps)."""

    def msssim_scale(self, a, b, taps_, quantize_, sums, pool_a=None, pool_b=None):
        g = np.asarray(taps_, np.float64)
        T = len(g)
        x = [quantize(_np(t)) if quantize_ else _np(t) for t in (a, b)]

        def F(v):
            n = v.shape[-1] - T + 1
            h = sum(g[t] * v[..., :, t:t + n] for t in range(T))
            return sum(g[t] * h[..., t:t + n, :] for t in range(T))

        mu1, mu2 = F(x[0]), F(x[1])
        s11, s22, s12 = F(x[0] * x[0]) - mu1 ** 2, F(x[1] * x[1]) - mu2 ** 2, F(x[0] * x[1]) - mu1 * mu2
        v1, v2 = 2 * s12 + C2, s11 + s22 + C2
        cs = v1 / v2
        ssim = (2 * mu1 * mu2 + C1) / (mu1 ** 2 + mu2 ** 2 + C1) * cs
        out = np.stack([ssim.sum(axis=(1, 2, 3)), cs.sum(axis=(1, 2, 3))], axis=1)
        sums.copy_(torch.from_numpy(out))
        for v, p in zip(x, (pool_a, pool_b)):
            if p is not None:
                p.copy_(torch.from_numpy((v[..., 0::2, 0::2] + v[..., 0::2, 1::2] +
                                          v[..., 1::2, 0::2] + v[..., 1::2, 1::2]) / 4))

    def msssim_combine(self, sums, counts, out):
        s = _np(sums).reshape(SCALES, -1, 2) / np.asarray(counts, np.float64).reshape(SCALES, 1, 1)
        out.copy_(torch.from_numpy(combine(s[..., 0], s[..., 1])))
