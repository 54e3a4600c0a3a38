"""Integer reference of the nearest-training-image search of pggan_amd/metrics.py, in numpy
int64 from its definition, and `CpuNnOps`, a numpy double of the nn_* ops so the host logic of
NearestNeighbours and ProgressiveGAN.validation runs without a GPU.

Definition.  Descriptor of an S x S image at the comparison resolution Rc (powers of two,
8 <= Rc <= 128, Rc <= S), f = S / Rc:
  8-bit grid  a uint8 image as it is; an fp32 image x in [-1, 1] through
              q(x) = rint(clip(fl32(127.5 x + 127.5), 0, 255)), ties to even, the sum rounded
              once to fp32 (the library's fused multiply-add)
  box pool    (sum of the f x f block + f^2 / 2) // f^2 per channel
  row         the pooled image - 128 as int8 [Rc, Rc, 3] in (y, x, c) order, D = 3 Rc^2 values;
              sq = the sum of their squares
Distance      d^2 = sq_q + sq_x - 2 (q . x) in int64
Result        per query the k (1 <= k <= 16) smallest (d^2, index) pairs in lexicographic order
              (a tie goes to the lower index); slots beyond the database size hold
              (INT64_MAX, -1); how the database is split into chunks does not matter.
"""
import numpy as np
import torch

NONE_D2 = np.iinfo(np.int64).max
ROW_BLOCK = 64      # what the double answers for HipOps.nn_row_block (it has no blocks)


def quantize(x):
    """fp32 [-1, 1] -> 0..255, int64.  127.5 x + 127.5 is exact in float64 for every fp32 x of
    ordinary size, and its rounding to fp32 is what a fused multiply-add returns."""
    v = (np.asarray(x, np.float32).astype(np.float64) * 127.5 + 127.5).astype(np.float32)
    return np.rint(np.clip(v, np.float32(0), np.float32(255))).astype(np.int64)


def pixels(images):
    """uint8 NHWC [.., S, S, 3] or floating NCHW [.., 3, S, S] -> int64 [.., S, S, 3] in 0..255."""
    images = np.asarray(images)
    if images.dtype == np.uint8:
        assert images.shape[-1] == 3 and images.shape[-2] == images.shape[-3]
        return images.astype(np.int64)
    assert images.shape[-3] == 3 and images.shape[-1] == images.shape[-2]
    return np.moveaxis(quantize(images), -3, -1)


def descriptor(images, Rc):
    """(rows int8 [.., 3 Rc^2], sq int64 [..]) of a batch of images."""
    p = pixels(images)
    S = p.shape[-2]
    assert Rc >= 8 and Rc <= 128 and Rc & (Rc - 1) == 0 and S % Rc == 0 and S >= Rc
    f = S // Rc
    lead = p.shape[:-3]
    blocks = p.reshape(lead + (Rc, f, Rc, f, 3)).sum(axis=(-4, -2))
    pooled = (blocks + (f * f) // 2) // (f * f) - 128
    assert pooled.min() >= -128 and pooled.max() <= 127
    rows = pooled.reshape(lead + (3 * Rc * Rc,))
    return rows.astype(np.int8), (rows * rows).sum(axis=-1)


def distances(q, qsq, db, dbsq):
    """d^2 int64 [Q, N]."""
    dot = np.asarray(q, np.int64) @ np.asarray(db, np.int64).T
    return np.asarray(qsq, np.int64)[:, None] + np.asarray(dbsq, np.int64)[None, :] - 2 * dot


def select(d2, idx, k):
    """The k lexicographically smallest (d2, idx) pairs of each row: (d2 [Q, k], idx [Q, k]),
    padded with (INT64_MAX, -1)."""
    Q = d2.shape[0]
    out_d = np.full((Q, k), NONE_D2, np.int64)
    out_i = np.full((Q, k), -1, np.int64)
    for i in range(Q):
        live = idx[i] >= 0
        order = np.lexsort((idx[i][live], d2[i][live]))[:k]
        out_d[i, :len(order)] = d2[i][live][order]
        out_i[i, :len(order)] = idx[i][live][order]
    return out_d, out_i


def search(q, qsq, db, dbsq, k, first_index=0):
    """Brute force over the whole database: (d2 [Q, k], idx [Q, k])."""
    d2 = distances(q, qsq, db, dbsq)
    idx = np.broadcast_to(first_index + np.arange(d2.shape[1], dtype=np.int64), d2.shape)
    return select(d2, idx, k)


def merge(best_d2, best_idx, q, qsq, db, dbsq, first_index):
    """One chunk merged into running lists [Q, k]; returns the new lists."""
    k = best_d2.shape[1]
    d2 = distances(q, qsq, db, dbsq)
    idx = np.broadcast_to(first_index + np.arange(d2.shape[1], dtype=np.int64), d2.shape)
    return select(np.concatenate([best_d2, d2], axis=1), np.concatenate([best_idx, idx], axis=1), k)


def streamed(q, qsq, db, dbsq, k, sizes):
    """The same search with the database merged chunk by chunk (chunk sizes `sizes`)."""
    assert sum(sizes) == db.shape[0]
    best_d2 = np.full((q.shape[0], k), NONE_D2, np.int64)
    best_idx = np.full((q.shape[0], k), -1, np.int64)
    first = 0
    for n in sizes:
        best_d2, best_idx = merge(best_d2, best_idx, q, qsq, db[first:first + n],
                                  dbsq[first:first + n], first)
        first += n
    return best_d2, best_idx


# ------------------------------------------------------------------ the tests' inputs
def smooth_images(n, S, seed):
    """n smooth random uint8 images [n, S, S, 3]: 4 x 4 (at S = 8: 2 x 2) noise upsampled
    bilinearly, so neighbouring rows of a descriptor are correlated as in real images."""
    g = np.random.default_rng(seed)
    low = max(2, min(4, S // 4))
    z = torch.from_numpy(g.uniform(10, 245, (n, 3, low, low)))
    up = torch.nn.functional.interpolate(z, size=(S, S), mode="bilinear", align_corners=True)
    return np.rint(up.permute(0, 2, 3, 1).numpy()).astype(np.uint8)


def make_case(Q, N, Rc, seed):
    """A database of N smooth images at Rc x Rc and Q queries, as descriptor rows: the even
    queries are database rows (spread over the database) plus noise in {-2 .. 2} per value, so
    their nearest neighbour is known (d^2 <= 4 D against >= 100 D for other rows); the odd ones
    are independent smooth images.  Returns (q, qsq, db, dbsq, known) with known[i] the database
    index of query i or -1."""
    g = np.random.default_rng(seed + 1)
    db_img = smooth_images(N, Rc, seed)
    q_img = smooth_images(Q, Rc, seed + 7919)
    known = np.full(Q, -1, np.int64)
    for i in range(0, Q, 2):
        known[i] = (i // 2 * 7 + N // 2) % N
        noisy = db_img[known[i]].astype(np.int64) + g.integers(-2, 3, db_img[0].shape)
        q_img[i] = np.clip(noisy, 0, 255).astype(np.uint8)
    db, dbsq = descriptor(db_img, Rc)
    q, qsq = descriptor(q_img, Rc)
    return q, qsq.astype(np.int32), db, dbsq.astype(np.int32), known


# ------------------------------------------------------------------ the op double
class CpuNnOps:
    """The nn_* methods of pggan_amd._lib.HipOps on CPU tensors, through the reference above.
    A mix-in (tests combine it with cpu_ops.CpuOps)."""

    nn_row_block = ROW_BLOCK

    def nn_descriptors(self, images, Rc, desc, sq):
        rows, s = descriptor(images.detach().cpu().numpy(), int(Rc))
        assert tuple(desc.shape) == rows.shape and desc.dtype == torch.int8 and sq.dtype == torch.int32
        desc.copy_(torch.from_numpy(rows))
        sq.copy_(torch.from_numpy(s.astype(np.int32)))

    def nn_search(self, q, qsq, db, dbsq, first_index, best_d2, best_idx, ws=None):
        assert q.dtype == db.dtype == torch.int8 and qsq.dtype == dbsq.dtype == torch.int32
        assert best_d2.dtype == best_idx.dtype == torch.int64 and best_d2.shape == best_idx.shape
        d2, idx = merge(best_d2.numpy().copy(), best_idx.numpy().copy(), q.numpy(), qsq.numpy(),
                        db.numpy(), dbsq.numpy(), int(first_index))
        best_d2.copy_(torch.from_numpy(d2))
        best_idx.copy_(torch.from_numpy(idx))
