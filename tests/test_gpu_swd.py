"""The sliced Wasserstein kernels (pggan_amd/csrc/swd.hip) and the metric built on them, on the
GPU, against the float64 reference of tests/swd_ref.py.

Bounds (u = 2^-24).  A filter output is a weighted sum with dyadic weights summing to 1: in
any summation order its fp32 error is <= 25 u max|x|, so one filter application on given
fp32 inputs is held to level_bound = 32 u max|x| (the Laplacian value fine - up(coarse): one
filter plus one subtraction of operands <= max|x| each, the same bound).  A projection of a
normalised descriptor d on a unit direction is held to 160 u ||d||_2 (147 FMA roundings plus
the fused normalisation).  The sorted-L1 mean is 1-Lipschitz in the sup norm of the projections.

STATS_TOL and E2E_TOL are 4 x what was measured on an MI355X (each test prints its figures)."""
import numpy as np
import pytest
import torch

import swd_ref as R
from gen_inputs import TINY_DEPTHS
from test_gpu_graph import build
from test_model_api import make_args
from test_swd_cpu import images, reference_of

pytestmark = pytest.mark.gpu

U = R.U24
# 4 x the worst relative error of mean and rstd measured over the three sizes (8.7e-8, the
# rstd at n = 5), which is tighter than the 1e-5 that tells a one-pass E[x^2] - mean^2 in fp32
# apart (off by 5e-4 .. 1 on this input)
STATS_TOL = 3.5e-7
# 4 x the measured relative deviation of the end-to-end value from float64 (3.7e-8 at the
# worst level), under the cap of 1e-3 (the paper prints SWD x 1e3 to two decimals on values
# of 2-10).  The kernels are deterministic, so the measured figure repeats bit for bit.
E2E_TOL = 1.5e-7


@pytest.fixture(scope="module")
def ops():
    from pggan_amd import _lib
    return _lib.HipOps(torch.float32)


def level_bound(*arrays):
    return 32 * U * max(float(np.abs(a).max()) for a in arrays)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


# ------------------------------------------------------------------ pyr_down
@pytest.mark.parametrize("R_,B", [(32, 1), (32, 3), (64, 1), (64, 3), (256, 2)])
@pytest.mark.parametrize("quant", [False, True])
def test_pyr_down(ops, R_, B, quant):
    g = np.random.default_rng(R_ + B)
    if quant:     # on the u8 grid: 127.5 x + 127.5 is within 1e-5 of an integer, no tie can flip
        x = ((g.integers(0, 256, (B, 3, R_, R_)) - 127.5) / 127.5).astype(np.float32)
    else:
        x = g.normal(size=(B, 3, R_, R_)).astype(np.float32)
    y = torch.full((B, 3, R_ // 2, R_ // 2), float("nan"), device="cuda")
    ops.swd_pyr_down(dev(x), y, quant)
    src = R.quantize(x) if quant else x.astype(np.float64)
    if quant:
        assert np.abs(src - (x.astype(np.float64) * 127.5 + 127.5)).max() < 1e-4
    ref = R.pyr_down(src)
    err = np.abs(y.cpu().numpy().astype(np.float64) - ref)
    print(f"pyr_down R={R_} B={B} quant={quant}: max err {err.max():.3e} bound {level_bound(src):.3e}")
    assert err.max() <= level_bound(src)


# ------------------------------------------------------------------ descriptors
def corner_positions(S, B, K, g):
    pos = g.integers(3, S - 3, (B * K, 2)).astype(np.int32)
    pos[:4] = [(3, 3), (3, S - 4), (S - 4, 3), (S - 4, S - 4)]
    pos[K:K + 4] = pos[:4][::-1]            # and on another image
    return pos


@pytest.mark.parametrize("S", [16, 32, 64])
@pytest.mark.parametrize("quant", [False, True])
def test_descriptors(ops, S, quant):
    B, K = 3, 5
    g = np.random.default_rng(S)
    if quant:
        fine = ((g.integers(0, 256, (B, 3, S, S)) - 127.5) / 127.5).astype(np.float32)
    else:
        fine = g.normal(size=(B, 3, S, S)).astype(np.float32)
    pos = corner_positions(S, B, K, g)
    src = R.quantize(fine) if quant else fine.astype(np.float64)
    scale = 255.0 if quant else 1.0
    coarse = None if S == 16 else (g.normal(size=(B, 3, S // 2, S // 2)) * scale).astype(np.float32)
    desc = torch.full((B * K + 1, 147), float("nan"), device="cuda")
    ops.swd_descriptors(dev(fine), None if coarse is None else dev(coarse),
                        torch.from_numpy(pos).cuda(), desc[:B * K], K, quant)
    got = desc.cpu().numpy()
    assert np.isnan(got[B * K]).all(), "the row past the last patch is untouched"
    got = got[:B * K].reshape(-1, 3, 7, 7)
    if coarse is None:
        assert np.array_equal(got, R.gather(src, pos, K).astype(np.float32)), "bitwise the input"
        return
    up = R.pyr_up(coarse)
    ref = R.gather(src - up, pos, K)
    err = np.abs(got.astype(np.float64) - ref)
    bound = level_bound(src, coarse)
    print(f"descriptors S={S} quant={quant}: max err {err.max():.3e} bound {bound:.3e}")
    assert err.max() <= bound
    # a kernel that mirrored the right / bottom edge like the left / top one would be off by
    # far more than the bound at the last two rows and columns
    sym = up.copy()
    sym[..., -1] = up[..., -2]
    assert np.abs(R.gather(src - sym, pos, K) - ref).max() > 1e3 * bound


# ------------------------------------------------------------------ stats
@pytest.fixture(scope="module")
def big_desc():
    """70001 descriptors ~ N(0, 1) + 127 + channel (the 8-bit scale of the coarsest level);
    drawn once, every case takes its first n."""
    g = np.random.default_rng(70001)
    d = g.normal(size=(70001, 3, 49)) + (127.0 + np.arange(3))[None, :, None]
    return d.reshape(70001, 147).astype(np.float32)


@pytest.mark.parametrize("n", [5, 640, 70001])
def test_stats(ops, big_desc, n):
    d = big_desc[:n]
    mean3, rstd3 = torch.zeros(3, device="cuda"), torch.zeros(3, device="cuda")
    ops.swd_stats(dev(d), mean3, rstd3)
    d64 = d.astype(np.float64).reshape(n, 3, 49)
    mean, rstd = d64.mean(axis=(0, 2)), 1.0 / d64.std(axis=(0, 2))
    em = np.abs(mean3.cpu().numpy() - mean) / mean
    er = np.abs(rstd3.cpu().numpy() - rstd) / rstd
    # what a one-pass variance in fp32 would give on this input
    x32 = torch.from_numpy(d).view(n, 3, 49)
    naive = 1.0 / ((x32 * x32).mean(dim=(0, 2)) - x32.mean(dim=(0, 2)) ** 2).clamp_min(1e-12).sqrt()
    en = np.abs(naive.numpy().astype(np.float64) - rstd) / rstd
    print(f"stats n={n}: rel err mean {em.max():.3e} rstd {er.max():.3e} (one-pass fp32 {en.max():.3e})")
    assert em.max() <= STATS_TOL and er.max() <= STATS_TOL
    if n >= 640:
        assert en.max() > 2 * STATS_TOL, "the input must tell a one-pass variance apart"


# ------------------------------------------------------------------ project
@pytest.mark.parametrize("n", [5, 640, 5120])
@pytest.mark.parametrize("P", [3, 128])
def test_project(ops, big_desc, n, P):
    g = np.random.default_rng(n + P)
    d = big_desc[:n]
    mean3 = (127.0 + np.arange(3) + g.normal(size=3) * 0.1).astype(np.float32)
    rstd3 = (1.0 + g.uniform(-0.2, 0.2, 3)).astype(np.float32)
    dirs = g.normal(size=(147, P))
    dirs = (dirs / np.linalg.norm(dirs, axis=0)).astype(np.float32)
    stride = n + 11
    proj = torch.full((P, stride), -7.0, device="cuda")
    ops.swd_project(dev(d), dev(mean3), dev(rstd3), dev(dirs), proj)
    got = proj.cpu().numpy()
    assert (got[:, n:] == -7.0).all(), "padding beyond n is untouched"
    dn = (d.astype(np.float64).reshape(n, 3, 49) - mean3.astype(np.float64)[None, :, None]) * \
        rstd3.astype(np.float64)[None, :, None]
    dn = dn.reshape(n, 147)
    ref = (dn @ dirs.astype(np.float64)).T
    bound = 160 * U * np.linalg.norm(dn, axis=1)[None, :]
    err = np.abs(got[:, :n] - ref)
    print(f"project n={n} P={P}: worst err / bound {float((err / bound).max()):.3f}")
    assert (err <= bound).all()


# ------------------------------------------------------------------ l1
@pytest.mark.parametrize("stride", [70004, 70009])   # rows 16-B aligned (vector loads + tail) or not
def test_l1(ops, stride):
    P, n = 3, 70001
    g = np.random.default_rng(stride)
    a = np.sort(g.normal(size=(P, stride)).astype(np.float32), axis=1)
    b = np.sort((g.normal(size=(P, stride)) * 1.5 + 0.3).astype(np.float32), axis=1)
    ref = np.abs(a[:, :n].astype(np.float64) - b[:, :n].astype(np.float64)).sum()
    ta, tb = dev(a), dev(b)
    out1, out2 = torch.zeros(1, device="cuda"), torch.zeros(1, device="cuda")
    ops.swd_l1(ta, tb, n, out1)
    ops.swd_l1(ta, tb, n, out2)
    v1 = float(out1.item())
    print(f"l1 stride={stride}: rel err {abs(v1 - ref) / ref:.3e}")
    assert abs(v1 - ref) <= 1e-6 * ref
    assert torch.equal(out1, out2), "a repeated call is bitwise equal"
    ops.swd_l1(ta, tb, n, out2)
    assert abs(float(out2.item()) - 2 * ref) <= 1e-6 * 2 * ref, "accumulates into out"


# ------------------------------------------------------------------ end to end
def feed_all(ops, real, fake, **kw):
    from pggan_amd.metrics import SlicedWasserstein
    m = SlicedWasserstein(ops, real.shape[-1], real.shape[0], **kw)
    for w, x in (("real", real), ("fake", fake)):
        for part in torch.split(x.cuda(), [4, 8]):
            m.feed(w, part)
    return m, m.result()


def test_end_to_end(ops):
    kw = dict(per_image=128, dirs=128, repeats=2, seed=1)
    real, fake = images(12, 64, 11), images(12, 64, 12, "smooth")
    m, got = feed_all(ops, real, fake, **kw)
    ref = reference_of(m, real, fake)
    assert list(got) == [64, 32, 16, "avg"]
    for k in got:
        rel = abs(got[k] - ref[k]) / ref[k]
        print(f"end to end {k}: {got[k]:.6f} ref {ref[k]:.6f} rel {rel:.3e}")
    for k in got:
        assert ref[k] > 1.0 and abs(got[k] - ref[k]) <= E2E_TOL * ref[k], (k, got[k], ref[k])
    assert m.result() == got and feed_all(ops, real, fake, **kw)[1] == got, "bitwise repeatable"
    assert feed_all(ops, real, real.clone(), **kw)[1] == {64: 0.0, 32: 0.0, 16: 0.0, "avg": 0.0}


# ------------------------------------------------------------------ model level
def model(tmp_path, s, ema, replay=False, validate=True):
    args = make_args(tmp_path, depths=list(TINY_DEPTHS), ema_decay=ema, use_validation=validate,
                     swd_images=8, valid_cycle=1)
    m = build(args, False, s)
    m.use_replay = replay
    m.set_validation()
    m.G.alpha = m.D.alpha = 0.5
    return m


@pytest.mark.parametrize("ema", [None, 0.5])
@pytest.mark.parametrize("s", [2, 4])
def test_model_validation(tmp_path, s, ema):
    m = model(tmp_path, s, ema)
    m.train_step()
    out = m.validation(0)
    R_ = 4 * 2 ** s
    assert list(out) == [R_ >> l for l in range(s - 1)] + ["avg"]
    assert all(np.isfinite(v) and v > 0 for v in out.values()), out
    assert m.validation(1) == out


@pytest.mark.parametrize("replay", [False, True])
def test_validation_leaves_training_alone(tmp_path, replay):
    with_, without = model(tmp_path, 2, 0.5, replay), model(tmp_path, 2, 0.5, replay, validate=False)
    for step in range(4):
        for m in (with_, without):
            m.train_step()
        assert with_.validation(step) is not None and without.validation(step) is None
    torch.cuda.synchronize()
    if replay:
        assert with_.graph_replays == without.graph_replays > 0
    for net in ("fpG", "fpD"):
        for buf in ("flat", "m", "v"):
            assert torch.equal(getattr(getattr(with_, net), buf),
                               getattr(getattr(without, net), buf)), (net, buf)
    assert torch.equal(with_.fpG.ema, without.fpG.ema)


# ------------------------------------------------------------------ bad arguments
def test_bad_arguments(ops):
    z = lambda *s: torch.full(s, 3.0, device="cuda")
    y, pos = z(1, 3, 8, 8), torch.full((5, 2), 3, dtype=torch.int32, device="cuda")
    with pytest.raises(RuntimeError, match="swd_pyr_down"):
        ops.swd_pyr_down(z(1, 3, 16, 16), y, True)             # H < 32
    desc = z(5, 147)
    with pytest.raises(RuntimeError, match="swd_descriptors"):
        ops.swd_descriptors(z(1, 3, 8, 8), None, pos, desc, 5, False)    # S < 16
    m3, r3 = z(3), z(3)
    with pytest.raises(RuntimeError, match="swd_stats"):
        ops.swd_stats(torch.empty(0, 147, device="cuda"), m3, r3)        # n = 0
    proj = z(3, 4)
    with pytest.raises(RuntimeError, match="swd_project"):
        ops.swd_project(desc, m3, r3, z(147, 3), proj)                   # stride 4 < n = 5
    out = z(1)
    with pytest.raises(RuntimeError, match="swd_l1"):
        ops.swd_l1(z(3, 4), z(3, 4), 5, out)                             # n > stride
    with pytest.raises(RuntimeError, match="CPU tensor"):
        ops.swd_l1(torch.zeros(3, 4), z(3, 4), 4, out)
    torch.cuda.synchronize()
    for t in (y, desc, m3, r3, proj, out):
        assert bool((t == 3.0).all()), "outputs are left unwritten"
