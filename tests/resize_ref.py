"""numpy restatement of Pillow's 8-bit BILINEAR resize (libImaging/Resample.c), the arithmetic
pg_resize_bilinear_u8 reproduces: `Image.resize((S, S), Image.BILINEAR)` of an RGB image, as
torchvision's Resize((S, S)) on a PIL image runs it (lib/dataset.py:107).

Per axis, input size `in`, output size `out` (all float arithmetic in C doubles = Python floats):
  scale = in / out, fs = max(scale, 1.0), support = fs, ksize = (int)ceil(support) * 2 + 1
  per output xx: c = (xx + 0.5) * scale
                 xmin = max((int)(c - support + 0.5), 0)
                 xmax = min((int)(c + support + 0.5), in) - xmin
                 w[x] = max(0, 1 - |(x + xmin - c + 0.5) / fs|)         x < xmax
                 ww   = w[0] + w[1] + ..  (in that order);  w[x] /= ww  if ww != 0
                 k[x] = (int)(0.5 + w[x] * 2^22)
  out[xx] = clip8((2^21 + sum_x pixel[xmin + x] * k[x]) >> 22)
The horizontal pass runs first, into a uint8 image [Hin][S]; the vertical pass reads that.  A
pass whose input and output sizes are equal is skipped (ImagingResample: need_horizontal /
need_vertical), so a same-size resize is a copy.
"""
import math

import numpy as np

PRECISION_BITS = 32 - 8 - 2


def coeffs(in_size, out_size):
    """-> (k int32 [out][ksize], bounds int32 [out][2] = (xmin, count)); unused taps are 0."""
    scale = in_size / out_size
    fs = scale if scale > 1.0 else 1.0
    support = 1.0 * fs
    ksize = int(math.ceil(support)) * 2 + 1
    k = np.zeros((out_size, ksize), np.int32)
    bounds = np.zeros((out_size, 2), np.int32)
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = int(center - support + 0.5)
        if xmin < 0:
            xmin = 0
        xmax = int(center + support + 0.5)
        if xmax > in_size:
            xmax = in_size
        xmax -= xmin
        w = []
        ww = 0.0
        for x in range(xmax):
            v = (x + xmin - center + 0.5) / fs
            if v < 0.0:
                v = -v
            v = 1.0 - v if v < 1.0 else 0.0
            w.append(v)
            ww += v
        for x in range(xmax):
            v = w[x] / ww if ww != 0.0 else w[x]
            k[xx, x] = int(0.5 + v * (1 << PRECISION_BITS))
        bounds[xx] = (xmin, xmax)
    return k, bounds


def _pass(img, k, bounds):
    """One pass along axis 0 of img uint8 [in][...] -> uint8 [out][...]."""
    out = np.empty((k.shape[0],) + img.shape[1:], np.uint8)
    wide = img.astype(np.int64)
    for xx in range(k.shape[0]):
        x0, n = int(bounds[xx, 0]), int(bounds[xx, 1])
        acc = np.tensordot(k[xx, :n].astype(np.int64), wide[x0:x0 + n], axes=(0, 0))
        out[xx] = np.clip((acc + (1 << (PRECISION_BITS - 1))) >> PRECISION_BITS, 0, 255)
    return out


def resize_bilinear(img, S):
    """img uint8 [Hin][Win][3] -> uint8 [S][S][3]."""
    Hin, Win = img.shape[:2]
    if Win != S:
        img = _pass(img.transpose(1, 0, 2), *coeffs(Win, S)).transpose(1, 0, 2)
    if Hin != S:
        img = _pass(img, *coeffs(Hin, S))
    return np.ascontiguousarray(img)
