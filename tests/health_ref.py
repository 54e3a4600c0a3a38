"""Independent float64 numpy reference of the training-health ops (pg_tensor_stats,
pg_nonfinite_watch), written from the definitions in include/pggan_hip.h -- TEST
INFRASTRUCTURE ONLY.  Per segment {offset, count} of a flat fp32 buffer: sums of squares (added
with math.fsum: exactly rounded, so the reference carries no summation error of its own),
largest magnitudes and non-finite counts, over x[offset : offset + count] and nothing else; the
Adam update u = step_size m / (sqrt(v) / bc2_sqrt + eps) in float64 from the fp32 m, v and the
fp32 scalars, where both m and v are finite."""
import math

import numpy as np

COLS = ("sumsq_p", "sumsq_g", "sumsq_u", "maxabs_p", "maxabs_g", "maxabs_u",
        "bad_p", "bad_g", "bad_m", "bad_v")


def update(m, v, step_size, bc2_sqrt, eps):
    """|u| in float64, elementwise, 0 where m or v is not finite."""
    m64, v64 = np.asarray(m, np.float32).astype(np.float64), np.asarray(v, np.float32).astype(np.float64)
    ok = np.isfinite(m64) & np.isfinite(v64)
    m64, v64 = np.where(ok, m64, 0.0), np.where(ok, v64, 0.0)
    ss, bc, e = (np.float64(np.float32(x)) for x in (step_size, bc2_sqrt, eps))
    return np.abs((ss * m64) / (np.sqrt(v64) / bc + e))


def _sum_max(x64):
    """(sum of squares, largest magnitude) of the finite elements of a float64 array."""
    a = np.abs(x64[np.isfinite(x64)])
    return math.fsum((a * a).tolist()), float(a.max()) if a.size else 0.0


def tensor_stats(table, p, g, m, v, step_size=1.0, bc2_sqrt=1.0, eps=0.0):
    """float64 [nseg, 10] in the order of COLS; a buffer that is None gives zeros."""
    table = np.asarray(table, np.int64).reshape(-1, 2)
    out = np.zeros((len(table), len(COLS)), np.float64)
    for s, (off, cnt) in enumerate(table):
        sl = slice(int(off), int(off + cnt))
        for k, x in enumerate((p, g)):
            if x is not None:
                out[s, k], out[s, 3 + k] = _sum_max(np.asarray(x[sl], np.float32).astype(np.float64))
        for k, x in enumerate((p, g, m, v)):
            if x is not None:
                out[s, 6 + k] = int((~np.isfinite(np.asarray(x[sl], np.float32))).sum())
        if m is not None and v is not None:
            out[s, 2], out[s, 5] = _sum_max(update(m[sl], v[sl], step_size, bc2_sqrt, eps))
    return out


def nonfinite_watch(table, x, tag, first_bad):
    """first_bad after one launch: slots still 0 whose segment holds a non-finite element."""
    table = np.asarray(table, np.int64).reshape(-1, 2)
    out = np.array(first_bad, np.int32, copy=True)
    for s, (off, cnt) in enumerate(table):
        if out[s] == 0 and not np.isfinite(np.asarray(x[int(off):int(off + cnt)], np.float32)).all():
            out[s] = tag
    return out


def segment_case(C, pad_value=np.nan, seed=0):
    """The segment-size case of the op tests: segments of 1, 3, 15, 16, 17, 63, 64, 65, C - 1, C,
    C + 1 and 3 C + 5 floats at 16-float-aligned offsets; every padding float (between a
    segment's end and the next offset, and up to the end of the buffer) holds `pad_value`.
    Returns (table int64 [12, 2], n, fill) where fill(scale_lo, scale_hi, positive) draws a
    float32 buffer of n: N(0, 1) scaled per segment by factors spread geometrically from
    scale_lo to scale_hi."""
    sizes = [1, 3, 15, 16, 17, 63, 64, 65, C - 1, C, C + 1, 3 * C + 5]
    return layout(sizes, pad_value, seed)


def layout(sizes, pad_value=np.nan, seed=0):
    offs, off = [], 0
    for c in sizes:
        offs.append(off)
        off += (c + 15) // 16 * 16
    n = off
    table = np.array(list(zip(offs, sizes)), np.int64)
    rng = np.random.default_rng(seed)

    def fill(scale_lo=1e-30, scale_hi=1e25, positive=False):
        x = np.full(n, pad_value, np.float32)
        scales = np.geomspace(scale_lo, scale_hi, len(sizes))
        for (o, c), sc in zip(table, scales):
            r = rng.standard_normal(int(c))
            x[o:o + c] = ((np.abs(r) if positive else r) * sc).astype(np.float32)
        return x
    return table, n, fill
