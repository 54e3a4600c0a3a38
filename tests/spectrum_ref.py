"""float64 reference of the radial power spectrum of pggan_amd/metrics.py (PowerSpectrum),
written from its definition with numpy.fft.fft2 over the whole plane (neither the packed real
rows, the half plane nor the per-column runs of the kernel), and `CpuSpectrumOps`, a numpy
double of the spectrum_profile op so the host logic of PowerSpectrum and
ProgressiveGAN.validation runs without a GPU.

Definition (one image, fp32 NCHW [3,R,R], R a power of two, 8 <= R <= 1024):
  q       = rint(clip(127.5 x + 127.5, 0, 255)), ties to even (`quantize`), else x as it is
  y       = 0.299 (q_r - 127.5) + 0.587 (q_g - 127.5) + 0.114 (q_b - 127.5)
  F       = DFT2(y), unnormalised, no window; signed frequencies u, v in [-R/2, R/2)
  bin     k = round(sqrt(u^2 + v^2)): k^2 - k < u^2 + v^2 <= k^2 + k; bins k > K = R/2 dropped
  prof[k] = sum over the bin of |F|^2
  S[k]    = mean over the images of prof[k] / count[k]
"""
import numpy as np
import torch

LUMA = {"weights": (0.299, 0.587, 0.114), "mean": (1 / 3, 1 / 3, 1 / 3)}


def quantize(x):
    return np.rint(np.clip(np.asarray(x, np.float64) * 127.5 + 127.5, 0.0, 255.0))


def bins(R, binning="round"):
    """[R, R] bin of every point in numpy.fft order.  "round" is the definition (evaluated in
    float64: exact for these radii, which tests/test_spectrum_cpu.py checks against the integer
    rule); "floor" is a deliberately wrong variant for the tests."""
    f = np.fft.fftfreq(R, 1.0 / R)
    r = np.sqrt(f[:, None] ** 2 + f[None, :] ** 2)
    return np.floor(r + {"round": 0.5, "floor": 0.0}[binning]).astype(np.int64)


def profile64(images, quantize_=True, binning="round", luma="weights"):
    """images [n,3,R,R] -> prof float64 [n, R/2 + 1]."""
    x = quantize(images) if quantize_ else np.asarray(images, np.float64)
    w = np.asarray(LUMA[luma], np.float64).reshape(1, 3, 1, 1)
    y = ((x - 127.5) * w).sum(axis=1)
    p = np.abs(np.fft.fft2(y)) ** 2
    R = y.shape[-1]
    k = bins(R, binning).ravel()
    keep = k <= R // 2
    return np.stack([np.bincount(k[keep], weights=pi.ravel()[keep], minlength=R // 2 + 1) for pi in p])


def counts(R, binning="round"):
    k = bins(R, binning).ravel()
    return np.bincount(k[k <= R // 2], minlength=R // 2 + 1)


def set_profile(images, quantize_=True):
    """S[k] of a set of images."""
    return profile64(images, quantize_).mean(axis=0) / counts(images.shape[-1])


def make_images(R, seed, n):
    """[n,3,R,R] fp32 on the 8-bit grid, in [-1, 1]: 127.5 + 60 sin(2 pi (3 x + 2 y + 0.1 i))
    cos(3 pi y) + N(0, 25) per channel (x, y in [0, 1), i the image's index), rounded, clipped
    and mapped back.  The white noise gives every bin substantial power; under 0.1 % of the
    values clip."""
    g = np.random.default_rng(seed)
    y, x = np.meshgrid(np.arange(R) / R, np.arange(R) / R, indexing="ij")
    i = np.arange(n).reshape(n, 1, 1, 1)
    v = 127.5 + 60 * np.sin(2 * np.pi * (3 * x + 2 * y + 0.1 * i)) * np.cos(3 * np.pi * y) + \
        g.normal(0, 25, (n, 3, R, R))
    v = np.rint(np.clip(v, 0, 255))
    return ((v - 127.5) / 127.5).astype(np.float32)


def cosine_image(R, u0, v0, amp=40.0):
    """[1,3,R,R] fp32 on the 0..255 scale (for quantize=False): every channel 127.5 + amp
    cos(2 pi (u0 r + v0 c) / R), so y = amp cos(..): two spectral lines of amp R^2 / 2 each."""
    r, c = np.meshgrid(np.arange(R), np.arange(R), indexing="ij")
    y = 127.5 + amp * np.cos(2 * np.pi * (u0 * r + v0 * c) / R)
    return np.broadcast_to(y, (1, 3, R, R)).astype(np.float32).copy()


class CpuSpectrumOps:
    """spectrum_profile of pggan_amd._lib.HipOps on CPU tensors: the definition in float64,
    rounded once into the fp32 output.  A mix-in (tests combine it with cpu_ops.CpuOps)."""

    def spectrum_profile(self, x, quantize_, out):
        out.copy_(torch.from_numpy(profile64(x.detach().cpu().numpy(), bool(quantize_))))
