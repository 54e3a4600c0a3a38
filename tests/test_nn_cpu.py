"""The nearest-training-image search without a GPU: the integer reference (tests/nn_ref.py)
against hand cases, NearestNeighbours over the numpy op double, BatchLoader.raw_u8, the C ABI's
host-side argument checks, and ProgressiveGAN.validation with `nn_queries` on the CPU test
double.  Every comparison is integer equality."""
import ctypes
import os

import numpy as np
import pytest
import torch
from PIL import Image

import msssim_ref
import nn_ref as N
import swd_ref
from cpu_ops import CpuOps
from pggan_amd import _lib, nets
from pggan_amd import data as PD
from pggan_amd.metrics import NN_NONE, NearestNeighbours
from pggan_amd.model import ProgressiveGAN
from test_model_api import fresh_model, make_args
from test_swd_cpu import assert_unchanged, snapshot


class NnCpuOps(N.CpuNnOps, msssim_ref.CpuMsssimOps, swd_ref.CpuSwdOps, CpuOps):
    pass


def to_f32(u8):
    """uint8 NHWC -> the fp32 NCHW image in [-1, 1] on the 8-bit grid."""
    return ((np.moveaxis(u8.astype(np.float64), -1, -3) - 127.5) / 127.5).astype(np.float32)


# ------------------------------------------------------------------ the reference itself
def test_reference_hand_cases():
    assert NN_NONE == N.NONE_D2 == 2 ** 63 - 1
    img = N.smooth_images(2, 32, 0)
    for Rc in (8, 16, 32):
        rows, sq = N.descriptor(img, Rc)
        assert rows.dtype == np.int8 and rows.shape == (2, 3 * Rc * Rc)
        d2 = N.distances(rows, sq, rows, sq)
        assert d2[0, 0] == 0 and d2[1, 1] == 0 and d2[0, 1] == d2[1, 0] > 0, "an identical image"
        # the fp32 image on the 8-bit grid has the same descriptor
        rows_f, sq_f = N.descriptor(to_f32(img), Rc)
        assert np.array_equal(rows_f, rows) and np.array_equal(sq_f, sq)
    # all-0 against all-255 at Rc = 128: past int32
    black, white = np.zeros((1, 128, 128, 3), np.uint8), np.full((1, 128, 128, 3), 255, np.uint8)
    (b, bs), (w, ws) = N.descriptor(black, 128), N.descriptor(white, 128)
    assert bs[0] == 16384 * 49152 and ws[0] == 127 * 127 * 49152
    assert N.distances(b, bs, w, ws)[0, 0] == 65025 * 49152 > 2 ** 31
    # (y, x, c) order: one bright pixel of channel 1 at y = 2, x = 5
    one = np.zeros((8, 8, 3), np.uint8)
    one[2, 5, 1] = 200
    assert np.flatnonzero(N.descriptor(one, 8)[0] != -128).tolist() == [(2 * 8 + 5) * 3 + 1]


def test_reference_pooling_rounds_half_up():
    img = np.zeros((16, 16, 3), np.uint8)
    img[0, 0, 0] = 2          # block sum 2 of 4: 0.5 -> 1
    img[0, 2, 0] = 1          # 0.25 -> 0
    img[0, 4, 0] = 3          # 0.75 -> 1
    img[0:2, 6:8, 0] = (5, 5), (5, 7)      # 22 / 4 = 5.5 -> 6
    rows = N.descriptor(img, 8)[0].astype(np.int64).reshape(8, 8, 3) + 128
    assert rows[0, :4, 0].tolist() == [1, 0, 1, 6] and rows[..., 1:].max() == 0
    # fp32 quantisation: ties to even after the 127.5 x + 127.5
    x = np.array([-1.0, 1.0, 0.0, -2.0, 3.0, 1 / 127.5, float("nan")], np.float32)
    assert N.quantize(x[:6]).tolist() == [0, 255, 128, 0, 255, 128]


def test_reference_streamed_equals_brute_force():
    q, qsq, db, dbsq, known = N.make_case(6, 37, 8, 1)
    d2, idx = N.search(q, qsq, db, dbsq, 3)
    assert np.array_equal(idx[0::2, 0], known[0::2]) and (known[1::2] == -1).all()
    assert (d2[0::2, 0] <= 4 * 192).all() and (d2[0::2, 1] > 100 * 192).all(), "separated"
    assert (np.diff(d2, axis=1) >= 0).all()
    for sizes in ([37], [7, 30], [1] * 37, [36, 1]):
        sd2, sidx = N.streamed(q, qsq, db, dbsq, 3, sizes)
        assert np.array_equal(sd2, d2) and np.array_equal(sidx, idx)


# ------------------------------------------------------------------ NearestNeighbours over the double
def t8(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def run(q, qsq, db, dbsq, k, sizes, Rc=8):
    m = NearestNeighbours(NnCpuOps(), Rc, k, compare=Rc)
    m.set_query_descriptors(t8(q), t8(qsq))
    first = 0
    for n in sizes:
        m.feed_descriptors(t8(db[first:first + n]), t8(dbsq[first:first + n]), first)
        first += n
    idx, d2 = m.result()
    return d2.numpy(), idx.numpy(), m


def test_any_split_equals_one_feed():
    q, qsq, db, dbsq, _ = N.make_case(5, 130, 8, 2)
    ref = N.search(q, qsq, db, dbsq, 4)
    for sizes in ([130], [1, 129], [64, 66], [50, 0, 80], [13] * 10):
        d2, idx, m = run(q, qsq, db, dbsq, 4, sizes)
        assert np.array_equal(d2, ref[0]) and np.array_equal(idx, ref[1]), sizes
    assert np.array_equal(m.rms().numpy(), np.sqrt(ref[0] / 192.0))


def test_images_and_descriptors_agree():
    img = N.smooth_images(9, 32, 5)
    m = NearestNeighbours(NnCpuOps(), 32, 2, compare=16)
    m.set_queries(torch.from_numpy(to_f32(img[:3])))
    m.feed(torch.from_numpy(img[:4]), 0)                    # uint8 NHWC
    m.feed(torch.from_numpy(to_f32(img[4:])), 4)            # fp32 NCHW
    idx, d2 = m.result()
    rows, sq = N.descriptor(img, 16)
    ref = N.search(rows[:3], sq[:3], rows, sq, 2)
    assert np.array_equal(d2.numpy(), ref[0]) and np.array_equal(idx.numpy(), ref[1])
    assert idx[:, 0].tolist() == [0, 1, 2] and d2[:, 0].tolist() == [0, 0, 0]


def test_ties_go_to_the_lower_index():
    q, qsq, db, dbsq, _ = N.make_case(2, 40, 8, 3)
    db, dbsq = db.copy(), dbsq.copy()
    db[39], dbsq[39] = db[0], dbsq[0]           # the same row at index 0 and at N - 1
    q[0], qsq[0] = db[0], dbsq[0]
    for sizes in ([40], [1, 39], [39, 1], [20, 20]):
        d2, idx, _ = run(q, qsq, db, dbsq, 3, sizes)
        assert idx[0, :2].tolist() == [0, 39] and d2[0, :2].tolist() == [0, 0], sizes
        assert d2[0, 2] > 0
    ref = N.search(q, qsq, db, dbsq, 3)
    assert np.array_equal(d2, ref[0]) and np.array_equal(idx, ref[1])


def test_fewer_rows_than_k():
    q, qsq, db, dbsq, _ = N.make_case(3, 2, 8, 4)
    d2, idx, m = run(q, qsq, db, dbsq, 5, [1, 1])
    assert (idx[:, 2:] == -1).all() and (d2[:, 2:] == NN_NONE).all()
    assert (idx[:, :2] >= 0).all() and (d2[:, :2] < NN_NONE).all()
    assert torch.isinf(m.rms()[:, 2:]).all() and torch.isfinite(m.rms()[:, :2]).all()
    ref = N.search(q, qsq, db, dbsq, 5)
    assert np.array_equal(d2, ref[0]) and np.array_equal(idx, ref[1])


def test_bad_arguments_are_refused():
    ops = NnCpuOps()
    for R, Rc in ((32, 4), (32, 24), (32, 64), (256, 256), (24, 8), (4, 4)):
        with pytest.raises(ValueError, match="NearestNeighbours"):
            NearestNeighbours(ops, R, 3, compare=Rc)
    for k in (0, 17, -1):
        with pytest.raises(ValueError, match="k must be"):
            NearestNeighbours(ops, 64, k)
    m = NearestNeighbours(ops, 32, 3, compare=8)
    with pytest.raises(RuntimeError, match="set_queries"):
        m.feed(torch.zeros(1, 3, 32, 32), 0)
    with pytest.raises(RuntimeError, match="set_queries"):
        m.result()
    with pytest.raises(ValueError, match="expected"):
        m.set_queries(torch.zeros(2, 3, 16, 16))                    # not the resolution
    m.set_queries(torch.zeros(2, 3, 32, 32))
    with pytest.raises(ValueError, match="expected"):
        m.feed(torch.zeros(2, 32, 32, 3), 0)                        # NHWC must be uint8
    with pytest.raises(ValueError, match="expected"):
        m.feed(torch.zeros(2, 3, 32, 32, dtype=torch.uint8), 0)     # uint8 must be NHWC
    with pytest.raises(ValueError, match="feed_descriptors"):
        m.feed_descriptors(torch.zeros(2, 768, dtype=torch.int8), torch.zeros(2, dtype=torch.int32), 0)
    with pytest.raises(ValueError, match="feed_descriptors"):
        m.feed_descriptors(torch.zeros(2, 192, dtype=torch.int8), torch.zeros(3, dtype=torch.int32), 0)
    with pytest.raises(ValueError, match="first_index"):
        m.feed_descriptors(torch.zeros(2, 192, dtype=torch.int8), torch.zeros(2, dtype=torch.int32), -1)
    assert (m.result()[0] == -1).all(), "nothing was merged"


# ------------------------------------------------------------------ the C ABI on the host
def test_entry_points_reject_bad_arguments_on_the_host():
    """Refused before any HIP call: the pointers here are never dereferenced."""
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libpggan_hip.so not built")
    lib = _lib.load_library()
    buf = (ctypes.c_longlong * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    odd = ctypes.c_void_p(p.value + 4)
    assert lib.pg_nn_row_block() == 64
    assert lib.pg_nn_workspace_bytes(17, 130, 3) == 3 * 17 * 3 * 8, "3 row blocks"
    assert lib.pg_nn_workspace_bytes(1, 64, 16) == 16 * 8
    assert lib.pg_nn_workspace_bytes(1, 64, 17) == 0 and lib.pg_nn_workspace_bytes(1, 0, 1) == 0

    def search(Q=2, N=3, D=192, k=3, q=p, first=0, ws=p, wsb=1 << 20, best=p):
        return lib.pg_nn_search(Q, N, D, k, q, p, p, p, first, best, p, ws, wsb, None)

    calls = {
        "nn_search": [lambda: search(k=0), lambda: search(k=17), lambda: search(D=100),
                      lambda: search(D=0), lambda: search(D=49152 + 64), lambda: search(Q=0),
                      lambda: search(N=0), lambda: search(first=-1),
                      lambda: search(first=2 ** 31 - 2), lambda: search(q=odd),
                      lambda: search(ws=None), lambda: search(best=None),
                      lambda: search(wsb=2 * 3 * 8 - 1)],
        "nn_descriptors_f32": [lambda: lib.pg_nn_descriptors_f32(1, 32, 4, p, p, p, None),
                               lambda: lib.pg_nn_descriptors_f32(1, 32, 64, p, p, p, None),
                               lambda: lib.pg_nn_descriptors_f32(1, 256, 256, p, p, p, None),
                               lambda: lib.pg_nn_descriptors_f32(1, 48, 16, p, p, p, None),
                               lambda: lib.pg_nn_descriptors_f32(0, 32, 8, p, p, p, None),
                               lambda: lib.pg_nn_descriptors_f32(1, 32, 8, odd, p, p, None),
                               lambda: lib.pg_nn_descriptors_f32(1, 32, 8, p, None, p, None)],
        "nn_descriptors_u8": [lambda: lib.pg_nn_descriptors_u8(1, 32, 12, p, p, p, None),
                              lambda: lib.pg_nn_descriptors_u8(1, 8, 16, p, p, p, None),
                              lambda: lib.pg_nn_descriptors_u8(1, 32, 8, p, p, None, None)],
    }
    for name, fns in calls.items():
        for i, fn in enumerate(fns):
            assert fn() == -1, (name, i)
            assert name.encode() in lib.pg_last_error(), (name, i, lib.pg_last_error())
    assert not any(buf), "nothing was written"


# ------------------------------------------------------------------ BatchLoader.raw_u8
class LoaderOps:
    """augment_u8 that uses its parameters, so a batch shows what was drawn from the generator."""

    def augment_u8(self, src, params, dst, ws=None):
        dst.copy_(src.permute(0, 3, 1, 2).float() / 127.5 - 1 + params[:, 1].view(-1, 1, 1, 1))
        return ws


@pytest.fixture()
def pngs(tmp_path):
    rng = np.random.default_rng(8)
    for k in range(12):
        Image.fromarray(rng.integers(0, 256, size=(32, 32, 3), dtype=np.uint8)).save(
            tmp_path / f"i{k:02d}.png")
    return str(tmp_path)


@pytest.mark.parametrize("scale_index,cache_bytes", [(3, 0), (3, 1 << 20), (2, 1 << 20)])
def test_raw_u8_is_the_gather_alone(pngs, scale_index, cache_bytes):
    ds = PD.ImageFolderDataset([pngs], scale_index=scale_index)
    S = ds.size
    assert len(ds) == 12 and S == 4 * 2 ** scale_index
    batches = [[0, 1, 2, 3], [4, 5, 6, 7], [0, 1, 2, 3], [8, 9, 10, 11]]

    def loader():
        return PD.BatchLoader(ds, "cpu", LoaderOps(), seed=5, workers=2, cache_bytes=cache_bytes)

    plain, peeked = loader(), loader()
    expect = lambda idx: np.stack([PD.load_u8(ds.paths[i], S) for i in idx])
    assert np.array_equal(peeked.raw_u8(range(12)).numpy(), expect(range(12))), "before any next"
    for k, b in enumerate(batches):
        nxt = batches[(k + 1) % 4]
        a = plain.next(b, prefetch=nxt)
        for idx in ([11, 0, 5], b, nxt):         # uncached, just cached, being prefetched
            got = peeked.raw_u8(idx)
            assert got.dtype == torch.uint8 and tuple(got.shape) == (len(idx), S, S, 3)
            assert np.array_equal(got.numpy(), expect(idx))
        assert torch.equal(peeked.next(b, prefetch=nxt), a), f"batch {k}"
        assert peeked._calls == plain._calls and peeked.decoded == plain.decoded
        assert torch.equal(peeked.gen.get_state(), plain.gen.get_state())
        assert (peeked.cache is None) == (plain.cache is None)
        if plain.cache is not None:
            assert np.array_equal(np.asarray(peeked.cache.slot), np.asarray(plain.cache.slot))
    if cache_bytes:
        assert plain.cache is not None, "the cached path was exercised"
    plain.close()
    peeked.close()


# ------------------------------------------------------------------ ProgressiveGAN.validation
@pytest.fixture
def cpu_model(monkeypatch):
    monkeypatch.setattr(ProgressiveGAN, "ops_factory", staticmethod(NnCpuOps))
    monkeypatch.setattr(nets, "OPS_FACTORY", NnCpuOps)
    nets._ENGINES.clear()

    def make(tmp_path, stage=2, **over):
        torch.manual_seed(11)
        m = fresh_model(make_args(tmp_path, **dict(dict(swd_images=8, use_validation=True), **over)))
        m.set_validation()
        for _ in range(stage):
            m.change_scale(0)
        m.G.alpha = m.D.alpha = 0.5
        return m
    return make


def nn_figures(m, images, Rc, k):
    """(rms [Q, k], idx) of images against the model's synthetic batch, from the reference."""
    q, qsq = N.descriptor(images.numpy(), Rc)
    db, dbsq = N.descriptor(m.synthetic.numpy(), Rc)
    d2, idx = N.search(q, qsq, db, dbsq, k)
    return np.sqrt(d2 / (3.0 * Rc * Rc)), idx, d2


def test_validation_with_nn_queries(tmp_path, cpu_model):
    on = cpu_model(tmp_path / "on", nn_queries=5, msssim_pairs=2)
    off = cpu_model(tmp_path / "off", msssim_pairs=2)
    for m in (on, off):
        m.train_step()
    before = snapshot(on)
    out, old = on.validation(7), off.validation(7)
    assert_unchanged(on, before)
    assert list(old) == [16, "avg", "msssim", "msssim_real"], "the key blank: exactly the dict as before"
    assert list(out) == [16, "avg", "msssim", "msssim_real", "nn", "nn_real", "nn_min"]
    assert {k: out[k] for k in old} == old, "the SWD and MS-SSIM figures do not change"
    # the first 5 of the 8 fakes and of the 8 reals validation draws (batches of 4), at 16 x 16
    g = torch.Generator().manual_seed(0)
    fakes = torch.cat([on.sample(torch.randn(4, on.args.latent_dim, generator=g), ema=False)
                       for _ in range(2)])[:5]
    reals = torch.cat(list(on._validation.reals(16, 8, 4)))[:5]
    rf, rr = nn_figures(on, fakes, 16, 3)[0], nn_figures(on, reals, 16, 3)[0]
    assert out["nn"] == float(np.median(rf[:, 0])) and out["nn_min"] == float(rf[:, 0].min())
    assert out["nn_real"] == float(np.median(rr[:, 0]))
    assert 0 < out["nn_min"] <= out["nn"] < 255 and 0 < out["nn_real"] < 255
    assert on.validation(8) == out
    d_on, d_off = os.path.join(str(tmp_path), "on", "t"), os.path.join(str(tmp_path), "off", "t")
    rows = open(os.path.join(d_on, "nn.csv")).read().splitlines()
    assert [r.split(",")[:3] for r in rows] == [["7", "2", "16"], ["8", "2", "16"]]
    assert [float(v) for v in rows[0].split(",")[3:]] == [out["nn"], out["nn_min"], out["nn_real"]]
    assert sorted(os.listdir(d_off)) == ["msssim.csv", "swd.csv"], "the key blank: no new file"
    assert sorted(os.listdir(d_on)) == ["msssim.csv", "nn", "nn.csv", "swd.csv"]
    for f in ("swd.csv", "msssim.csv"):
        assert open(os.path.join(d_on, f)).read().splitlines()[0] == \
            open(os.path.join(d_off, f)).read().splitlines()[0]
    # the figure: 5 generated images in the top row, k = 3 rows of training images under them
    assert sorted(os.listdir(os.path.join(d_on, "nn"))) == ["e7.jpg", "e8.jpg"]
    assert Image.open(os.path.join(d_on, "nn", "e7.jpg")).size == (5 * 18 + 2, 4 * 20)
    # the public query: the same indices, and a training image finds itself
    idx, d2 = on.nearest_neighbours(fakes)
    ref = nn_figures(on, fakes, 16, 3)
    assert np.array_equal(idx.numpy(), ref[1]) and np.array_equal(d2.numpy(), ref[2])
    idx, d2 = on.nearest_neighbours(on.synthetic, k=1)
    assert idx[:, 0].tolist() == [0, 1, 2, 3] and d2[:, 0].tolist() == [0, 0, 0, 0]
    assert_unchanged(on, before)
    # the database is kept for the stage and dropped with it
    assert on._validation.nn_db[0] == (2, 16) and tuple(on._validation.nn_db[1].shape) == (4, 768)
    on.reset_solver()
    assert on._validation.nn_db is None
    # training goes on exactly as without it
    off.reset_solver()
    for m in (on, off):
        m.train_step()
    assert torch.equal(on.fpG.flat, off.fpG.flat) and torch.equal(on.fpD.flat, off.fpD.flat)


def test_validation_nn_settings_and_small_stages(tmp_path, cpu_model, capsys):
    m = cpu_model(tmp_path, stage=0, nn_queries=4, nn_k=6, nn_resolution=8, isMaster=True)
    assert m.validation(1) is None                                  # 4 x 4
    lines = [l for l in capsys.readouterr().out.splitlines() if l.startswith("step 1:")]
    assert len(lines) == 2 and "SWD is undefined" in lines[0]
    assert "nearest-neighbour search is undefined below 8x8" in lines[1]
    m.change_scale(0)
    m.G.alpha = m.D.alpha = 0.5
    out = m.validation(2)                                           # 8 x 8: the search alone
    assert list(out) == ["nn", "nn_real", "nn_min"]
    d = os.path.join(str(tmp_path), "t")
    assert sorted(os.listdir(d)) == ["nn", "nn.csv"]
    assert open(os.path.join(d, "nn.csv")).read().split(",")[:3] == ["2", "1", "8"]
    lines = [l for l in capsys.readouterr().out.splitlines() if l.startswith("step 2:")]
    assert len(lines) == 2 and "SWD is undefined" in lines[0]
    assert lines[1].startswith("step 2: nearest training image at 8x8")
    # k = 6 > the 4 synthetic images: the slots past them are empty
    idx, d2 = m.nearest_neighbours(m.synthetic[:2])
    assert tuple(idx.shape) == (2, 6) and (idx[:, 4:] == -1).all() and (d2[:, 4:] == NN_NONE).all()
    assert idx[:, 0].tolist() == [0, 1] and (idx[:, :4] >= 0).all()
    # without nn_queries 8 x 8 stays what it was
    plain = cpu_model(tmp_path / "p", stage=1)
    assert plain.validation(0) is None and not os.path.exists(os.path.join(str(tmp_path), "p", "t"))


def test_nn_config_errors(tmp_path, cpu_model):
    with pytest.raises(ValueError, match="nn_queries"):
        cpu_model(tmp_path, nn_queries=9)               # > swd_images = 8
    with pytest.raises(ValueError, match="nn_queries"):
        cpu_model(tmp_path, nn_queries=-1)
    for k in (0.5, 17, -2):
        with pytest.raises(ValueError, match="nn_k"):
            cpu_model(tmp_path, nn_queries=4, nn_k=k)
    for rc in (4, 48, 256):
        with pytest.raises(ValueError, match="nn_resolution"):
            cpu_model(tmp_path, nn_queries=4, nn_resolution=rc)
    off = cpu_model(tmp_path, nn_queries=4, use_validation=False)
    assert off.validation(0) is None
