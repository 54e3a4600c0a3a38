"""The nearest-training-image kernels (pggan_amd/csrc/nn.hip) and the search built on them, on
the GPU, against the integer reference of tests/nn_ref.py.  Squared L2 over 8-bit pixels is
exact in integers: every comparison is equality, there are no tolerances.

Inputs (nn_ref.make_case): a database of smooth random images; the even queries are database
rows plus noise in {-2 .. 2}, so their nearest neighbour is known and separated, the odd ones
are independent."""
import functools

import numpy as np
import pytest
import torch
from PIL import Image

import nn_ref as N
from gen_inputs import TINY_DEPTHS
from test_gpu_graph import build
from test_model_api import make_args

pytestmark = pytest.mark.gpu

NONE = N.NONE_D2


@pytest.fixture(scope="module")
def ops():
    from pggan_amd import _lib
    return _lib.HipOps(torch.float32)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def to_f32(u8):
    return ((np.moveaxis(u8.astype(np.float64), -1, -3) - 127.5) / 127.5).astype(np.float32)


# ------------------------------------------------------------------ descriptors
@functools.lru_cache(maxsize=None)
def desc_case(S, Rc):
    """Three uniform-noise images at side S (every rounding case of the pooling shows up), as
    uint8 NHWC and as fp32 NCHW with a few values pushed outside [-1, 1] (clipped to 0 / 255)."""
    g = np.random.default_rng(1000 * S + Rc)
    u8 = g.integers(0, 256, (3, S, S, 3), dtype=np.uint8)
    u8[0, 0, 0], u8[1, -1, -1], u8[2, S // 2, 1] = (0, 255, 0), (255, 0, 255), (255, 255, 0)
    f32 = to_f32(u8)
    f32[0, :, 0, 0], f32[1, :, -1, -1] = (-3.0, 1.5, -1.0), (2.0, -1.25, 1.0)
    return u8, f32, N.descriptor(u8, Rc)


@pytest.mark.parametrize("S,Rc", [(8, 8), (16, 8), (64, 16), (256, 128)])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("kind", ["f32", "u8"])
def test_descriptors(ops, S, Rc, B, kind):
    u8, f32, (rows, sq) = desc_case(S, Rc)
    x = dev(f32[:B] if kind == "f32" else u8[:B])
    D = 3 * Rc * Rc
    desc = torch.full((B + 1, D), 77, dtype=torch.int8, device="cuda")
    s = torch.full((B + 1,), -5, dtype=torch.int32, device="cuda")
    ops.nn_descriptors(x, Rc, desc[:B], s[:B])
    got, got_sq = desc.cpu().numpy(), s.cpu().numpy()
    assert (got[B] == 77).all() and got_sq[B] == -5, "the row past the last image is untouched"
    assert np.array_equal(got[:B], rows[:B])
    assert np.array_equal(got_sq[:B].astype(np.int64), sq[:B])


# ------------------------------------------------------------------ search
@functools.lru_cache(maxsize=None)
def search_case(N_, Rc):
    """17 queries against N_ rows at Rc, and the reference's 16 nearest; fewer queries or a
    smaller k are prefixes of it."""
    q, qsq, db, dbsq, known = N.make_case(17, N_, Rc, 31 * N_ + Rc)
    return q, qsq, db, dbsq, known, N.search(q, qsq, db, dbsq, 16)


def gpu_search(ops, q, qsq, db, dbsq, k, sizes=None):
    """One search on the GPU, the database fed in chunks of `sizes`: (d2, idx) as numpy, with a
    guard row behind the best lists."""
    Q = q.shape[0]
    best_d2 = torch.full((Q + 1, k), NONE, dtype=torch.int64, device="cuda")
    best_idx = torch.full((Q + 1, k), -1, dtype=torch.int64, device="cuda")
    best_d2[Q], best_idx[Q] = 123, 456
    qd, qs = dev(q), dev(qsq)
    first = 0
    for n in sizes or [db.shape[0]]:
        ops.nn_search(qd, qs, dev(db[first:first + n]), dev(dbsq[first:first + n]), first,
                      best_d2[:Q], best_idx[:Q])
        first += n
    d2, idx = best_d2.cpu().numpy(), best_idx.cpu().numpy()
    assert (d2[Q] == 123).all() and (idx[Q] == 456).all(), "the row past the last query is untouched"
    return d2[:Q], idx[:Q]


@pytest.mark.parametrize("N_", [1, 3, 37, 130, 1031])
@pytest.mark.parametrize("Q", [1, 5, 16, 17])
@pytest.mark.parametrize("k", [1, 3, 16])
def test_search_rc8(ops, Q, N_, k):
    q, qsq, db, dbsq, known, (ref_d2, ref_idx) = search_case(N_, 8)
    d2, idx = gpu_search(ops, q[:Q], qsq[:Q], db, dbsq, k)
    assert np.array_equal(d2, ref_d2[:Q, :k]) and np.array_equal(idx, ref_idx[:Q, :k])
    if N_ >= 37:
        assert np.array_equal(idx[0::2, 0], known[:Q][0::2]), "the planted neighbours"
    if N_ < k:
        assert (idx[:, N_:] == -1).all() and (d2[:, N_:] == NONE).all()


def test_search_d3072(ops):
    q, qsq, db, dbsq, known, (ref_d2, ref_idx) = search_case(130, 32)
    assert q.shape[1] == 3072
    for k in (3, 16):
        d2, idx = gpu_search(ops, q, qsq, db, dbsq, k)
        assert np.array_equal(d2, ref_d2[:, :k]) and np.array_equal(idx, ref_idx[:, :k])
    assert np.array_equal(idx[0::2, 0], known[0::2])


def test_search_d49152_is_64_bit(ops):
    """All-0, all-255 and a 0 / 255 checkerboard at Rc = 128: d^2 passes 2^31 (a 32-bit d^2
    fails) and |q . x| reaches 128^2 * 49152 (a 16- or 24-bit partial sum fails)."""
    y, x = np.meshgrid(np.arange(128), np.arange(128), indexing="ij")
    chk = np.repeat((((y + x) & 1) * 255).astype(np.uint8)[..., None], 3, axis=2)
    imgs = np.stack([np.zeros((128, 128, 3), np.uint8), np.full((128, 128, 3), 255, np.uint8), chk])
    db, dbsq = N.descriptor(imgs, 128)
    q, qsq = db[:2], dbsq[:2]
    ref_d2, ref_idx = N.search(q, qsq, db, dbsq, 3)
    assert ref_d2[0].tolist() == [0, 65025 * 24576, 65025 * 49152] and ref_idx[0].tolist() == [0, 2, 1]
    assert ref_d2[0, 2] > 2 ** 31
    d2, idx = gpu_search(ops, q, qsq.astype(np.int32), db, dbsq.astype(np.int32), 3)
    assert np.array_equal(d2, ref_d2) and np.array_equal(idx, ref_idx)


def test_streaming_and_repeatability(ops):
    q, qsq, db, dbsq, _, (ref_d2, ref_idx) = search_case(1031, 8)
    for k in (3, 16):
        runs = [gpu_search(ops, q, qsq, db, dbsq, k, sizes)
                for sizes in ([1031], [7, 512, 512], [1000, 31], [1031])]
        for d2, idx in runs:
            assert np.array_equal(d2, ref_d2[:, :k]) and np.array_equal(idx, ref_idx[:, :k])


def test_through_the_metric_class(ops):
    """NearestNeighbours end to end: images in, both layouts, split feeds."""
    from pggan_amd.metrics import NearestNeighbours
    img = N.smooth_images(70, 32, 9)
    rows, sq = N.descriptor(img, 16)
    ref_d2, ref_idx = N.search(rows[:5], sq[:5], rows, sq, 4)
    m = NearestNeighbours(ops, 32, 4, compare=16)
    m.set_queries(dev(to_f32(img[:5])))
    m.feed(dev(img[:33]), 0)
    m.feed(dev(to_f32(img[33:])), 33)
    idx, d2 = m.result()
    assert np.array_equal(d2.cpu().numpy(), ref_d2) and np.array_equal(idx.cpu().numpy(), ref_idx)
    assert idx[:, 0].tolist() == [0, 1, 2, 3, 4] and d2[:, 0].tolist() == [0] * 5
    assert np.array_equal(m.rms().cpu().numpy(), np.sqrt(ref_d2 / 768.0))


def test_duplicate_rows(ops):
    """The same row at index 0, either side of the kernel's row-block boundary and at N - 1:
    all at d^2 = 0, in index order, however the database is split."""
    RB = ops.nn_row_block
    assert RB >= 16
    N_ = 2 * RB + 9
    q, qsq, db, dbsq, _ = N.make_case(6, N_, 8, 77)
    db, dbsq, q, qsq = db.copy(), dbsq.copy(), q.copy(), qsq.copy()
    where = [0, RB - 1, RB, N_ - 1]
    db[where], dbsq[where] = db[5], dbsq[5]
    q[3], qsq[3] = db[5], dbsq[5]
    ref_d2, ref_idx = N.search(q, qsq, db, dbsq, 6)
    assert ref_idx[3].tolist()[:5] == [0, 5, RB - 1, RB, N_ - 1] and (ref_d2[3, :5] == 0).all()
    for sizes in ([N_], [RB, N_ - RB], [RB - 1, 2, N_ - RB - 1], [1, N_ - 2, 1]):
        for k in (2, 6):
            d2, idx = gpu_search(ops, q, qsq, db, dbsq, k, sizes)
            assert np.array_equal(d2, ref_d2[:, :k]) and np.array_equal(idx, ref_idx[:, :k]), (sizes, k)


# ------------------------------------------------------------------ bad arguments
def test_bad_arguments(ops):
    i8 = lambda *s: torch.full(s, 3, dtype=torch.int8, device="cuda")
    i32 = lambda *s: torch.full(s, 7, dtype=torch.int32, device="cuda")
    i64 = lambda *s: torch.full(s, 12345, dtype=torch.int64, device="cuda")
    q, qsq, db, dbsq = i8(2, 192), i32(2), i8(130, 192), i32(130)
    bd, bi = i64(2, 3), i64(2, 3)
    with pytest.raises(RuntimeError, match="nn_search"):
        ops.nn_search(q, qsq, db, dbsq, 0, i64(2, 0), i64(2, 0))              # k = 0
    bd17, bi17 = i64(2, 17), i64(2, 17)
    with pytest.raises(RuntimeError, match="nn_search"):
        ops.nn_search(q, qsq, db, dbsq, 0, bd17, bi17)                        # k = 17
    with pytest.raises(RuntimeError, match="nn_search"):
        ops.nn_search(i8(2, 100), qsq, i8(130, 100), dbsq, 0, bd, bi)         # D % 64 != 0
    with pytest.raises(RuntimeError, match="nn_search"):
        ops.nn_search(q.cpu(), qsq, db, dbsq, 0, bd, bi)                      # a CPU tensor
    small = torch.zeros(3 * 2 * 3 * 8 - 8, dtype=torch.uint8, device="cuda")
    with pytest.raises(RuntimeError, match="nn_search"):
        ops.nn_search(q, qsq, db, dbsq, 0, bd, bi, ws=small)                  # 3 row blocks need 144 B
    with pytest.raises(RuntimeError, match="nn_search"):
        ops.nn_search(q, qsq, db, dbsq, 2 ** 31 - 100, bd, bi)                # indices past 2^31
    desc, sq = i8(2, 192), i32(2)
    with pytest.raises(RuntimeError, match="nn_descriptors"):
        ops.nn_descriptors(torch.zeros(2, 3, 16, 16), 8, desc, sq)            # a CPU tensor
    with pytest.raises(RuntimeError, match="nn_descriptors"):
        ops.nn_descriptors(torch.zeros(2, 3, 16, 16, device="cuda"), 16, desc, sq)    # rows of 768
    with pytest.raises(RuntimeError, match="nn_descriptors"):
        ops.nn_descriptors(torch.zeros(2, 3, 24, 24, device="cuda"), 8, desc, sq)     # S no power of two
    with pytest.raises(RuntimeError, match="nn_descriptors"):
        ops.nn_descriptors(torch.zeros(2, 16, 16, 3, device="cuda"), 8, desc, sq)     # NHWC must be uint8
    torch.cuda.synchronize()
    for t in (bd, bi, bd17, bi17):
        assert (t == 12345).all(), "outputs are left unwritten"
    assert (desc == 3).all() and (sq == 7).all()
    assert (small == 0).all()


# ------------------------------------------------------------------ model level
def model(tmp_path, replay, nq):
    args = make_args(tmp_path, depths=list(TINY_DEPTHS), ema_decay=0.5, use_validation=True,
                     swd_images=8, valid_cycle=1, nn_queries=nq, batch_per_gpu=2)
    m = build(args, False, 2)
    m.use_replay = replay
    m.set_validation()
    m.G.alpha = m.D.alpha = 0.5
    return m


@pytest.mark.parametrize("replay", [False, True])
def test_validation_leaves_training_alone(tmp_path, replay):
    with_, without = model(tmp_path / "a", replay, 4), model(tmp_path / "b", replay, None)
    assert with_.synthetic.shape[0] == 2, "a database smaller than k = 3"
    for step in range(4):
        for m in (with_, without):
            m.train_step()
        out, old = with_.validation(step), without.validation(step)
        assert list(old) == [16, "avg"] and list(out) == [16, "avg", "nn", "nn_real", "nn_min"]
        assert {k: out[k] for k in old} == old
        assert all(np.isfinite(out[k]) and 0 <= out[k] <= 255 for k in ("nn", "nn_real", "nn_min"))
        assert out["nn_min"] <= out["nn"]
    idx, d2 = with_.nearest_neighbours(with_.synthetic)
    assert idx[:, 0].tolist() == [0, 1] and d2[:, 0].tolist() == [0, 0]
    assert (idx[:, :2] >= 0).all() and (idx[:, 2] == -1).all() and (d2[:, 2] == NONE).all(), \
        "index -1 only in the slot beyond the 2 images"
    torch.cuda.synchronize()
    if replay:
        assert with_.graph_replays == without.graph_replays > 0
    for net in ("fpG", "fpD"):
        for buf in ("flat", "m", "v"):
            assert torch.equal(getattr(getattr(with_, net), buf),
                               getattr(getattr(without, net), buf)), (net, buf)
    assert torch.equal(with_.fpG.ema, without.fpG.ema)


def test_training_images_find_themselves(tmp_path):
    root = tmp_path / "imgs"
    root.mkdir()
    for k, im in enumerate(N.smooth_images(20, 40, 12)):
        Image.fromarray(im).save(root / f"i{k:02d}.png")
    args = make_args(tmp_path, depths=list(TINY_DEPTHS), synthetic_data=False,
                     dataset_root_list=[str(root)], nn_resolution=16)
    m = build(args, False, 3)                       # 32 x 32, compared at 16 x 16
    n = len(m.train_dataset)
    assert n == 14
    raw = m._stage_loader().raw_u8(range(n))
    assert raw.dtype == torch.uint8 and tuple(raw.shape) == (n, 32, 32, 3)
    idx, d2 = m.nearest_neighbours(raw, k=1)
    assert idx[:, 0].tolist() == list(range(n)) and d2[:, 0].tolist() == [0] * n
    # the same images as the loader's fp32 layout, and three neighbours: the image first
    idx3, d23 = m.nearest_neighbours(raw.permute(0, 3, 1, 2).float() / 127.5 - 1)
    assert tuple(idx3.shape) == (n, 3) and torch.equal(idx3[:, 0], idx[:, 0])
    assert (d23[:, 0] == 0).all() and (d23[:, 1] > 0).all()
    rows, sq = N.descriptor(raw.cpu().numpy(), 16)
    ref_d2, ref_idx = N.search(rows, sq, rows, sq, 3)
    assert np.array_equal(idx3.cpu().numpy(), ref_idx) and np.array_equal(d23.cpu().numpy(), ref_d2)
    m._loader.close()
