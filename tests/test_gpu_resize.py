"""pg_resize_bilinear_u8 (pggan_amd/csrc/resize.hip) against PIL itself: the kernel's bytes equal
`Image.resize((S, S), Image.BILINEAR)` with == on

  1024x1024 -> 4    the longest sums (513 taps, split over 64 lanes)
  1024x1024 -> 512  the shortest downscale (5 taps, one lane per sum)
  64x64 -> 64       both passes skipped: a copy
  100x64 -> 64      vertical pass only, straight from the source
  64x100 -> 64      horizontal pass only, straight into the destination
  37x53 -> 8        odd sizes, unaligned source rows, non-integer scales
  12x20 -> 16       an upscale
  33x33 -> 32       a scale just above 1

(source Hin x Win) with random, all-255 and alternating 0 / 255 row contents in one call of
n = 3 whose destinations are non-contiguous and out of order in a larger buffer (the untouched
rows keep a sentinel), and on a call per shape for two source shapes into one batch, as the
loader groups them.  PIL references are computed once per shape.
"""
import functools

import numpy as np
import pytest
import torch
from PIL import Image

from pggan_amd import data as PD

pytestmark = pytest.mark.gpu

SHAPES = [(1024, 1024, 4), (1024, 1024, 512), (64, 64, 64), (100, 64, 64), (64, 100, 64),
          (37, 53, 8), (12, 20, 16), (33, 33, 32)]
SENTINEL = 0xA5


def pil_resize(img, S):
    return np.asarray(Image.fromarray(img).resize((S, S), Image.BILINEAR))


@functools.lru_cache(maxsize=None)
def _case(Hin, Win, S):
    """Three images of one shape (random, all-255, alternating 0 / 255 rows) and PIL's resize."""
    rng = np.random.default_rng(Hin * 7 + Win * 3 + S)
    imgs = np.empty((3, Hin, Win, 3), np.uint8)
    imgs[0] = rng.integers(0, 256, size=(Hin, Win, 3), dtype=np.uint8)
    imgs[1] = 255
    imgs[2] = 0
    imgs[2, 1::2] = 255
    return imgs, np.stack([pil_resize(im, S) for im in imgs])


def _pack(imgs):
    """Images of any shapes -> (flat uint8 buffer, 16-byte aligned byte offsets)."""
    offs, used = [], 0
    for im in imgs:
        offs.append(used)
        used = (used + im.size + 15) // 16 * 16
    buf = np.full(used, 0x5A, np.uint8)      # the gaps: never read into a result
    for im, o in zip(imgs, offs):
        buf[o:o + im.size] = im.reshape(-1)
    return buf, offs


def _resize(ops, buf, offs, Hin, Win, S, dst, rows, ws=None):
    so = torch.tensor(offs, dtype=torch.int64, device="cuda")
    do = torch.tensor([r * 3 * S * S for r in rows], dtype=torch.int64, device="cuda")
    return ops.resize_u8(buf, so, Hin, Win, S, PD.device_resize_coeffs(Win, S, "cuda"),
                         PD.device_resize_coeffs(Hin, S, "cuda"), dst, do, ws=ws)


@pytest.mark.parametrize("Hin,Win,S", SHAPES, ids=[f"{h}x{w}-{s}" for h, w, s in SHAPES])
def test_kernel_equals_pil(Hin, Win, S):
    from pggan_amd import _lib
    ops = _lib.HipOps(torch.bfloat16)
    imgs, ref = _case(Hin, Win, S)
    buf, offs = _pack(list(imgs))
    rows = [4, 0, 2]                         # scattered, out of order; rows 1, 3, 5 untouched
    dst = torch.full((6, S, S, 3), SENTINEL, dtype=torch.uint8, device="cuda")
    _resize(ops, torch.from_numpy(buf).cuda(), offs, Hin, Win, S, dst, rows)
    torch.cuda.synchronize()
    got = dst.cpu().numpy()
    for k, r in enumerate(rows):
        bad = got[r] != ref[k]
        assert not bad.any(), (k, int(bad.sum()), np.argwhere(bad)[:4].tolist())
    assert (got[[1, 3, 5]] == SENTINEL).all()


def test_two_source_shapes_into_one_batch():
    """The loader's grouping: one call per source shape, sharing the batch and the workspace."""
    from pggan_amd import _lib
    ops = _lib.HipOps(torch.bfloat16)
    S = 8
    (a, ra), (b, rb) = _case(37, 53, S), _case(64, 64, S)
    order = [a[0], b[0], a[2], b[1], b[2]]   # interleaved in the ragged buffer too
    buf, offs = _pack(order)
    dev = torch.from_numpy(buf).cuda()
    dst = torch.full((6, S, S, 3), SENTINEL, dtype=torch.uint8, device="cuda")
    ws = _resize(ops, dev, [offs[0], offs[2]], 37, 53, S, dst, [5, 1])
    _resize(ops, dev, [offs[1], offs[3], offs[4]], 64, 64, S, dst, [0, 4, 2], ws=ws)
    torch.cuda.synchronize()
    got = dst.cpu().numpy()
    for r, want in ((5, ra[0]), (1, ra[2]), (0, rb[0]), (4, rb[1]), (2, rb[2])):
        assert np.array_equal(got[r], want), r
    assert (got[3] == SENTINEL).all()


def test_bad_arguments_are_refused():
    from pggan_amd import _lib
    ops = _lib.HipOps(torch.bfloat16)
    buf = torch.zeros(64 * 64 * 3, dtype=torch.uint8, device="cuda")
    off = torch.zeros(1, dtype=torch.int64, device="cuda")
    dst = torch.zeros(1, 8, 8, 3, dtype=torch.uint8, device="cuda")
    with pytest.raises(RuntimeError):        # tables for an axis that changes size are required
        ops.resize_u8(buf, off, 64, 64, 8, None, PD.device_resize_coeffs(64, 8, "cuda"), dst, off)
    with pytest.raises(RuntimeError, match="LDS"):   # 8 rows of 4096 pixels: past the staging
        ops.resize_u8(buf, off, 8, 4096, 8, PD.device_resize_coeffs(4096, 8, "cuda"), None, dst, off)
