"""The source-resolution HBM cache end to end on the GPU (pggan_amd.data.HbmSourceCache +
pg_resize_bilinear_u8): a loader that resizes on the GPU delivers, from the same generator seed,
byte for byte the batches of the loader that decodes and resizes on the host; a later stage's
loader sharing the cache decodes nothing; a budget that holds only part of the images changes
no byte; and through ProgressiveGAN (`hbm_source_cache_gb`) the loader of the stage after
change_scale decodes nothing while train_step consumes the batches of a model with the key
blank.  8 PNGs of 64x64 and 48x80.
"""
import numpy as np
import pytest
import torch
from PIL import Image

from gen_inputs import TINY_DEPTHS
from pggan_amd import data as PD
from test_model_api import make_args

pytestmark = pytest.mark.gpu

BATCHES = [[0, 1, 2, 3], [4, 5, 6, 7], [2, 3, 4, 5]]


@pytest.fixture()
def pngs(tmp_path):
    rng = np.random.default_rng(11)
    d = tmp_path / "imgs"
    d.mkdir()
    for k in range(8):
        h, w = (64, 64) if k % 2 == 0 else (48, 80)
        Image.fromarray(rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)).save(d / f"im{k}.png")
    return str(d)


def _run(pngs, scale_index, source_cache, seed=7, batches=BATCHES):
    from pggan_amd import _lib
    ds = PD.ImageFolderDataset([pngs], scale_index=scale_index)
    assert len(ds) == 8
    ld = PD.BatchLoader(ds, "cuda", _lib.HipOps(torch.bfloat16), seed=seed, workers=3,
                        cache_bytes=1 << 20, source_cache=source_cache)
    outs = [ld.next(b, prefetch=batches[(k + 1) % len(batches)]).cpu().numpy()
            for k, b in enumerate(batches)]
    decoded = ld.decoded
    ld.close()
    return outs, decoded


def _same(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


def test_loader_bytes_equal_the_host_path(pngs):
    # the host path: PIL decodes and resizes.  The stage's cache exists from the second batch
    # on, so batch 2 decodes images 2 and 3 a second time
    ref16, dec = _run(pngs, 2, None)
    assert dec == 10
    sc = PD.HbmSourceCache("cuda", 1 << 20)
    got16, dec = _run(pngs, 2, sc)
    assert _same(got16, ref16) and dec == 8
    assert len(sc.entries) == 8 and all(e[0] % 16 == 0 and e[3] for e in sc.entries.values())
    # the next stage, same cache: nothing is decoded, and the bytes are a cold loader's
    ref32, dec = _run(pngs, 3, None)
    assert dec == 10
    got32, dec = _run(pngs, 3, sc)
    assert _same(got32, ref32) and dec == 0


def test_budget_for_three_images(pngs):
    ref, _ = _run(pngs, 2, None)
    sc = PD.HbmSourceCache("cuda", 3 * 64 * 64 * 3)   # room for three of the eight
    got, dec = _run(pngs, 2, sc)
    assert _same(got, ref)
    # images 0, 1, 2 fit (whatever their shapes: three of the larger shape fill the budget
    # exactly); the host path's 10 decodes minus image 2's second one
    assert len(sc.entries) == 3 and dec == 9
    ref32, _ = _run(pngs, 3, None)
    got32, dec = _run(pngs, 3, sc)
    assert _same(got32, ref32) and dec == 6           # 3, 4..7 and 3 again: still the host path


def _model(tmp_path, pngs, source_gb):
    from pggan_amd import nets
    from pggan_amd.model import ProgressiveGAN
    nets.OPS_FACTORY = None
    ProgressiveGAN.ops_factory = None
    args = make_args(tmp_path, max_step_at_scale=[2, 4, 3, 3], alpha_jump_start=[-1, 0, 1, 1],
                     alpha_jump_interval=[0, 1, 1, 1], alpha_jump_Ntimes=[0, 2, 2, 2],
                     depths=list(TINY_DEPTHS), synthetic_data=False, dataset_root_list=[pngs],
                     hbm_source_cache_gb=source_gb)
    torch.manual_seed(5)
    m = ProgressiveGAN(args, 0)
    m.initialize_models()
    m.set_optimizers()
    m.set_dataset()
    m.set_data_iterator()
    m.set_loss_collector()
    m.scale_index = 0
    m.alpha_index = 0
    m.alpha_jump_value = 0
    m.next_scale_jump_step = args.max_step_at_scale[0]
    m.next_alpha_jump_step = args.alpha_jump_start[0]
    seen = []
    load = m.load_next_batch

    def recording_load():
        out = load()
        seen.append(out.cpu().numpy())
        return out

    m.load_next_batch = recording_load
    return m, seen


def test_progressive_gan_keeps_the_cache_across_a_stage_change(tmp_path, pngs):
    """6 training images (the 70 % split), B = 4: the reference's loader order reads images
    0..3 in every batch (the next four would pass the end, so it wraps).  Two steps at 4^2,
    change_scale, two steps at 8^2, whose loader fills every batch from the source cache."""
    runs = []
    for gb in (None, 0.001):
        m, seen = _model(tmp_path / str(gb), pngs, gb)
        decoded = []
        for step in range(4):
            if step == 2:
                m.change_scale(step)
            m.train_step()
            decoded.append(m._loader.decoded)
        m.flush()
        assert [b.shape[-1] for b in seen] == [4, 4, 8, 8]
        runs.append((seen, decoded, m))
        m._loader.close()
    (ref, dec_ref, m_off), (got, dec_on, m_on) = runs
    assert _same(got, ref)                             # the batches train_step consumed
    assert getattr(m_off, "_source_cache", None) is None
    assert dec_ref[0] == 4 and dec_ref[2] == 4         # the parent decodes again at 8^2
    assert dec_on[:2] == [4, 4] and dec_on[2:] == [0, 0]   # the new stage's loader: nothing
    assert len(m_on._source_cache.entries) == 4
