"""The GPU resize's arithmetic and the source cache's bookkeeping without a GPU.

* tests/resize_ref.py (the numpy restatement of Pillow's libImaging/Resample.c that
  pg_resize_bilinear_u8 computes) equals `Image.resize((S, S), Image.BILINEAR)` with == over
  long and short sums, odd sizes, non-integer scales, an upscale, skipped passes, and on an
  all-255 image (the weights sum to 2^22 +- ksize / 2: white must stay white).
* pggan_amd.data.resize_coeffs, the tables the kernel is given, equals the restatement's.
* HbmSourceCache: room reserved from the header's size, 16-byte aligned ragged offsets, the
  budget cut-off; a second loader at another size decodes nothing for the images it holds.
  The loader runs on the CPU against `CpuOps`, a double of the two ops it calls.
"""
import numpy as np
import pytest
import torch
from PIL import Image

import resize_ref as R
from pggan_amd import data as PD

# (Hin, Win, S)
CASES = [(1024, 1024, 4), (64, 64, 8), (37, 53, 8), (12, 20, 16), (100, 64, 64), (64, 100, 64),
         (128, 128, 32), (33, 33, 32), (256, 192, 128), (16, 16, 16)]


def pil_resize(img, S):
    return np.asarray(Image.fromarray(img).resize((S, S), Image.BILINEAR))


def _image(Hin, Win, S, seed):
    if (Hin, Win, S) == (64, 64, 8):       # alternating 0 / 255 rows
        img = np.zeros((Hin, Win, 3), np.uint8)
        img[1::2] = 255
        return img
    return np.random.default_rng(seed).integers(0, 256, size=(Hin, Win, 3), dtype=np.uint8)


@pytest.mark.parametrize("Hin,Win,S", CASES, ids=[f"{h}x{w}-{s}" for h, w, s in CASES])
def test_restatement_equals_pil(Hin, Win, S):
    img = _image(Hin, Win, S, seed=Hin + Win + S)
    assert np.array_equal(R.resize_bilinear(img, S), pil_resize(img, S))
    white = np.full((Hin, Win, 3), 255, np.uint8)
    got = R.resize_bilinear(white, S)
    assert np.array_equal(got, pil_resize(white, S)) and (got == 255).all()


def test_resize_coeffs_equal_the_restatement():
    for n_in, n_out in sorted({(a, s) for h, w, s in CASES for a in (h, w)} | {(1024, 512), (1024, 128)}):
        k, b = PD.resize_coeffs(n_in, n_out)
        rk, rb = R.coeffs(n_in, n_out)
        assert k.dtype == np.int32 and b.dtype == np.int32
        assert np.array_equal(k, rk) and np.array_equal(b, rb), (n_in, n_out)
        assert (k >= 0).all() and (b[:, 0] + b[:, 1] <= n_in).all() and (b[:, 1] <= k.shape[1]).all()
        # what keeps an int32 accumulator exact: 255 * sum(k) + 2^21 < 2^31
        assert abs(int(k.sum(1).max()) - (1 << 22)) <= k.shape[1] // 2 + 1
    assert PD.resize_coeffs(1024, 4) is PD.resize_coeffs(1024, 4)      # built once per (in, out)


class CpuOps:
    """The two ops BatchLoader calls, on CPU tensors: resize_u8 through the restatement,
    augment_u8 as the plain ToTensor + Normalize (no flip / jitter: these tests compare the
    bytes the resize delivers)."""

    def __init__(self):
        self.resize_calls = []

    def resize_u8(self, src, src_off, Hin, Win, S, tab_x, tab_y, dst, dst_off, ws=None):
        assert (tab_x is None) == (Win == S) and (tab_y is None) == (Hin == S)
        self.resize_calls.append((Hin, Win, S, src_off.numel()))
        flat = dst.view(-1)
        for so, do in zip(src_off.tolist(), dst_off.tolist()):
            assert so % 16 == 0
            img = src[so:so + 3 * Hin * Win].numpy().reshape(Hin, Win, 3)
            flat[do:do + 3 * S * S] = torch.from_numpy(R.resize_bilinear(img, S).reshape(-1))
        return ws

    def augment_u8(self, src, params, dst, ws=None):
        dst.copy_((src.permute(0, 3, 1, 2).float() / 255 - 0.5) / 0.5)
        return ws


SHAPES = [(64, 64), (48, 80), (37, 53), (64, 64), (48, 80), (20, 12)]


@pytest.fixture()
def pngs(tmp_path):
    rng = np.random.default_rng(3)
    for k, (h, w) in enumerate(SHAPES):
        Image.fromarray(rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)).save(tmp_path / f"i{k}.png")
    return str(tmp_path)


def test_source_cache_reserves_by_header_size(pngs):
    ds = PD.ImageFolderDataset([pngs], scale_index=1)
    paths = sorted(ds.paths)
    sc = PD.HbmSourceCache("cpu", budget_bytes=3 * (64 * 64 + 48 * 80 + 37 * 53) + 64)
    offs = []
    for p, (h, w) in zip(paths[:3], SHAPES):
        off, eh, ew, filled = sc.reserve(p)
        assert (eh, ew, filled) == (h, w, False)        # from the header: nothing decoded yet
        offs.append(off)
    # ragged and 16-byte aligned: 37 * 53 * 3 = 5883 bytes is no multiple of 16
    assert offs == [0, 12288, 12288 + 11520] and all(o % 16 == 0 for o in offs)
    assert sc.used == (offs[2] + 5883 + 15) // 16 * 16
    assert sc.reserve(paths[3]) is None                 # the budget is used: not cached
    assert sc.reserve(paths[0])[0] == 0                 # an existing entry is kept
    assert not sc.filled(paths[0])
    img = PD.load_src_u8(paths[2])
    sc.fill(paths[2], torch.from_numpy(img))
    assert sc.filled(paths[2])
    assert np.array_equal(sc.buf[offs[2]:offs[2] + 5883].numpy().reshape(37, 53, 3), img)
    with pytest.raises(RuntimeError):
        sc.fill(paths[1], torch.from_numpy(img))        # not the shape the header announced


def _expect(ds, idx):
    u8 = np.stack([ds.load(i) for i in idx])
    return (u8.transpose(0, 3, 1, 2).astype(np.float32) / 255 - 0.5) / 0.5


@pytest.mark.parametrize("budget,cached", [(1 << 20, 6), (3 * (64 * 64 + 48 * 80 + 37 * 53) + 64, None)],
                         ids=["all", "budget"])
def test_second_stage_decodes_nothing_for_cached_images(pngs, budget, cached):
    sc = PD.HbmSourceCache("cpu", budget_bytes=budget)
    batches = [[0, 1, 2], [3, 4, 5], [0, 1, 2]]
    ds = PD.ImageFolderDataset([pngs], scale_index=2)           # 16 x 16
    ops = CpuOps()
    ld = PD.BatchLoader(ds, "cpu", ops, workers=2, cache_bytes=0, source_cache=sc)
    for k, b in enumerate(batches):
        out = ld.next(b, prefetch=batches[(k + 1) % 3])
        assert np.array_equal(out.numpy(), _expect(ds, b))      # the host's PIL bytes
    n_src = len(sc.entries)
    assert n_src == (cached or n_src) and all(e[3] for e in sc.entries.values())
    if cached:
        assert ld.decoded == 6                                   # once each; batch 2 from HBM
    else:
        assert 0 < n_src < 6 and ld.decoded == 6 + sum(ds.paths[i] not in sc.entries for i in batches[2])
    ld.close()
    # one call per distinct source shape in a batch
    assert all(n >= 1 for *_, n in ops.resize_calls)
    ds2 = PD.ImageFolderDataset([pngs], scale_index=3)          # the next stage: 32 x 32
    ops2 = CpuOps()
    ld2 = PD.BatchLoader(ds2, "cpu", ops2, workers=2, cache_bytes=0, source_cache=sc)
    for b in batches[:2]:
        assert np.array_equal(ld2.next(b).numpy(), _expect(ds2, b))
    assert ld2.decoded == 6 - n_src                              # 0 when every image is cached
    assert sum(n for *_, n in ops2.resize_calls) == n_src
    ld2.close()


def test_loader_without_source_cache_never_resizes_on_the_device(pngs):
    ds = PD.ImageFolderDataset([pngs], scale_index=2)
    ops = CpuOps()
    ld = PD.BatchLoader(ds, "cpu", ops, workers=2, cache_bytes=0)
    assert np.array_equal(ld.next([0, 1, 2, 3]).numpy(), _expect(ds, [0, 1, 2, 3]))
    assert ld.decoded == 4 and not ops.resize_calls
    ld.close()
