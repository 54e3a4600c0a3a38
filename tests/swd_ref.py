"""float64 reference of the sliced Wasserstein distance of pggan_amd/metrics.py, written from
its definition with numpy / scipy.ndimage, and `CpuSwdOps`, a numpy double of the five swd_*
ops so the host logic of SlicedWasserstein and ProgressiveGAN.validation runs without a GPU.

Definition (images fp32 NCHW [B,3,R,R] in [-1,1], R a power of two >= 16):
  q(x)     = rint(clip(127.5 x + 127.5, 0, 255)), ties to even (level 0, `quantize`)
  down(G)  = correlate with k (x) k, k = [1 4 6 4 1] / 16, mode='mirror', then [::2, ::2]
  up(G)    = zero-insert to double size (samples at even indices), correlate with 4 k (x) k
  L_l      = G_l - up(G_{l+1}); the last level (16 x 16) is G_last itself
  desc     = K 7x7x3 patches per image and level around given centres -> [N, 147]
  norm     = per channel (x - mean) / population std over the N * 49 values
  distance = mean over repeats of mean |sort(A d) - sort(B d)| over N and the directions
"""
import numpy as np
import scipy.ndimage as ndi
import torch

K1 = np.array([1.0, 4.0, 6.0, 4.0, 1.0]) / 16.0
U24 = 2.0 ** -24


def quantize(x):
    return np.rint(np.clip(np.asarray(x, np.float64) * 127.5 + 127.5, 0.0, 255.0))


def _filt(x, scale=1.0):
    """k (x) k over the last two axes, mirror boundary (no repeated edge sample)."""
    x = ndi.correlate1d(np.asarray(x, np.float64), K1, axis=-1, mode="mirror")
    return ndi.correlate1d(x, K1, axis=-2, mode="mirror") * scale


def pyr_down(x):
    return _filt(x)[..., ::2, ::2]


def pyr_up(c):
    c = np.asarray(c, np.float64)
    z = np.zeros(c.shape[:-2] + (2 * c.shape[-2], 2 * c.shape[-1]))
    z[..., ::2, ::2] = c
    return _filt(z, 4.0)


def up_1d_closed(c):
    """The closed form of pyr_up along one axis."""
    c = np.asarray(c, np.float64)
    n = len(c)
    e = np.concatenate([[c[1]], c, [c[n - 1]]])      # c[-1] := c[1], c[n] := c[n-1]
    out = np.empty(2 * n)
    out[0::2] = (e[0:n] + 6 * e[1:n + 1] + e[2:n + 2]) / 8
    out[1::2] = (e[1:n + 1] + e[2:n + 2]) / 2
    return out


def down_1d_closed(x):
    x = np.asarray(x, np.float64)
    n = len(x)
    m = lambda j: -j if j < 0 else 2 * (n - 1) - j if j > n - 1 else j
    return np.array([sum(K1[t] * x[m(2 * i + t - 2)] for t in range(5)) for i in range(n // 2)])


def gaussian_pyramid(x, quant=True):
    g = [quantize(x) if quant else np.asarray(x, np.float64)]
    while g[-1].shape[-1] > 16:
        g.append(pyr_down(g[-1]))
    return g


def laplacian_pyramid(x, quant=True):
    g = gaussian_pyramid(x, quant)
    return [g[l] - pyr_up(g[l + 1]) for l in range(len(g) - 1)] + [g[-1]]


def gather(img, pos, K):
    """img [B,3,S,S], pos [B*K,2] (y, x) -> [B*K,3,7,7]."""
    pos = np.asarray(pos).reshape(-1, 2)
    out = np.empty((len(pos), 3, 7, 7), img.dtype)
    for p, (y, x) in enumerate(pos):
        out[p] = img[p // K, :, y - 3:y + 4, x - 3:x + 4]
    return out


def normalize(d):
    d = np.asarray(d, np.float64).reshape(-1, 3, 49)
    mean = d.mean(axis=(0, 2), keepdims=True)
    std = np.sqrt(((d - mean) ** 2).mean(axis=(0, 2), keepdims=True))
    return ((d - mean) / std).reshape(-1, 147)


def sliced_distance(da, db, dirs):
    """da, db [N,147] raw descriptors, dirs [repeats,147,P] -> distance x 1e3."""
    a, b = normalize(da), normalize(db)
    vals = []
    for d in np.asarray(dirs, np.float64):
        pa, pb = np.sort(a @ d, axis=0), np.sort(b @ d, axis=0)
        vals.append(np.abs(pa - pb).mean())
    return float(np.mean(vals)) * 1e3


def swd_reference(real, fake, positions, dirs, K, quant=True):
    """real, fake [N,3,R,R]; positions[which][level] int [N*K,2]; dirs [repeats,147,P]."""
    lr, lf = laplacian_pyramid(real, quant), laplacian_pyramid(fake, quant)
    out = {}
    for l, (a, b) in enumerate(zip(lr, lf)):
        da = gather(a, positions["real"][l], K).reshape(-1, 147)
        db = gather(b, positions["fake"][l], K).reshape(-1, 147)
        out[a.shape[-1]] = sliced_distance(da, db, dirs)
    out["avg"] = float(np.mean([out[k] for k in out]))
    return out


def _np(t):
    return t.detach().cpu().numpy().astype(np.float64)


class CpuSwdOps:
    """The swd_* methods of pggan_amd._lib.HipOps on CPU tensors: float64 arithmetic, results
    rounded once into the fp32 outputs.  A mix-in (tests combine it with cpu_ops.CpuOps)."""

    def swd_pyr_down(self, x, y, quantize_):
        v = _np(x)
        y.copy_(torch.from_numpy(pyr_down(quantize(v) if quantize_ else v)))

    def swd_descriptors(self, fine, coarse, pos, desc, K, quantize_):
        v = _np(fine)
        v = quantize(v) if quantize_ else v
        if coarse is not None:
            v = v - pyr_up(_np(coarse))
        desc.copy_(torch.from_numpy(gather(v, pos.numpy(), K).reshape(-1, 147)))

    def swd_stats(self, desc, mean3, rstd3):
        d = _np(desc).reshape(-1, 3, 49)
        mean = d.mean(axis=(0, 2))
        var = ((d - mean[None, :, None]) ** 2).mean(axis=(0, 2))
        mean3.copy_(torch.from_numpy(mean))
        rstd3.copy_(torch.from_numpy(1.0 / np.sqrt(var)))

    def swd_project(self, desc, mean3, rstd3, dirs, proj):
        n = desc.shape[0]
        d = (_np(desc).reshape(-1, 3, 49) - _np(mean3)[None, :, None]) * _np(rstd3)[None, :, None]
        proj[:, :n].copy_(torch.from_numpy((d.reshape(n, 147) @ _np(dirs)).T.copy()))

    def swd_l1(self, a, b, n, out):
        out += float(np.abs(_np(a)[:, :n] - _np(b)[:, :n]).sum())
