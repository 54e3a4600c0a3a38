"""The MS-SSIM kernels (pggan_amd/csrc/msssim.hip) and the metric built on them, on the GPU,
against the float64 reference of tests/msssim_ref.py.

Inputs (msssim_ref.make_pairs): on the 8-bit grid, a = a sinusoid pattern + N(0, 25),
b = a + N(0, 40): pair values 0.73 .. 0.93, every factor >= 0.44, so no clip fires and nothing
is multiplied by a value near 0 (independent noise pairs have the value 0 and would hide every
error).

Bounds.  The pooled outputs are sums of four inputs times 1/4: held to 32 * 2^-24 * max|x| like
pyr_down (measured: exact on the 8-bit grid).  The tolerances are 4 x what was measured on an
MI355X (each test prints its figures), under the caps 2e-5 on a per-scale mean and 5e-5 on a
pair value (half a unit of the fourth decimal the paper prints):
  SCALE_TOL      a scale's two means, inputs on the 8-bit grid: measured 7.9e-8 at worst
                 (S = 8, P = 3), 1e-8 .. 6e-8 elsewhere
  SCALE_TOL_RAW  the same on fp32 normal inputs off the grid: measured 2.55e-6 at worst (S = 1,
                 where every variance is 0 and what is left is the rounding of x^2 ~ 1e4 over
                 c2 = 58.5), under 1e-6 from S = 16 on; off the grid x - 127.5 and the products
                 round, on the grid and on its 2x2 means (what the metric feeds) they are exact
  E2E_TOL        a pair value: measured 6.0e-8 at worst (R = 16), 2.8e-8 .. 4.3e-8 at 32 .. 256
A half-sample error in the centre of an even window, or one row and column of positions too
few, moves the reference by more than 100 x these bounds (asserted below)."""
import functools

import numpy as np
import pytest
import torch

import msssim_ref as M
from gen_inputs import TINY_DEPTHS
from test_gpu_graph import build
from test_model_api import make_args

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
SCALE_TOL, SCALE_TOL_RAW, E2E_TOL = 4 * 7.9e-8, 4 * 2.55e-6, 4 * 6.0e-8
assert max(SCALE_TOL, SCALE_TOL_RAW) <= 2e-5 and E2E_TOL <= 5e-5, "the caps"


@pytest.fixture(scope="module")
def ops():
    from pggan_amd import _lib
    return _lib.HipOps(torch.float32)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


# ------------------------------------------------------------------ one scale
@functools.lru_cache(maxsize=None)
def scale_case(S, quant):
    """Three pairs at side S and their float64 statistics; P = 1 takes the first."""
    if quant:
        a, b = M.make_pairs(S, 100 + S, 3)
        a64, b64 = M.quantize(a), M.quantize(b)
        assert np.abs(a64 - (a.astype(np.float64) * 127.5 + 127.5)).max() < 1e-4, "on the grid"
    else:
        g = np.random.default_rng(200 + S)
        a = (127.5 + 40 * g.normal(size=(3, 3, S, S))).astype(np.float32)
        b = (a + 20 * g.normal(size=a.shape)).astype(np.float32)
        a64, b64 = a.astype(np.float64), b.astype(np.float64)
    w = M.window2d(S)
    ssim, cs = M.scale_stats(a64, b64, w)
    n = S - w.shape[0] + 1
    off = M.scale_stats(a64, b64, w, drop=1) if n > 1 else None
    pool = (M.down(a64), M.down(b64)) if S % 2 == 0 else None
    return a, b, ssim, cs, off, pool, max(np.abs(a64).max(), np.abs(b64).max())


@pytest.mark.parametrize("S,T", [(16, 11), (8, 8), (4, 4), (2, 2), (1, 1), (32, 11), (64, 11),
                                 (96, 11), (256, 11)])
@pytest.mark.parametrize("P", [1, 3])
@pytest.mark.parametrize("quant", [True, False])
def test_msssim_scale(ops, S, T, P, quant):
    from pggan_amd.metrics import msssim_taps
    a, b, ssim, cs, off, pool, xmax = scale_case(S, quant)
    taps = msssim_taps(S)
    assert len(taps) == T
    x = dev(M.interleave(a[:P], b[:P]))              # the pairs interleaved: strided sides
    nan = float("nan")
    sums = torch.full((P + 1, 2), nan, device="cuda")
    pa = pb = None
    if pool is not None:
        pa, pb = (torch.full((P + 1, 3, S // 2, S // 2), nan, device="cuda") for _ in range(2))
    ops.msssim_scale(x[0::2], x[1::2], taps, quant, sums[:P],
                     None if pa is None else pa[:P], None if pb is None else pb[:P])
    got = sums.cpu().numpy().astype(np.float64)
    assert np.isnan(got[P]).all(), "the row past the last pair is untouched"
    n = S - T + 1
    e_ssim = np.abs(got[:P, 0] / (3 * n * n) - ssim[:P]).max()
    e_cs = np.abs(got[:P, 1] / (3 * n * n) - cs[:P]).max()
    print(f"msssim_scale S={S} T={T} P={P} quant={quant}: err ssim {e_ssim:.3e} cs {e_cs:.3e}")
    assert max(e_ssim, e_cs) <= (SCALE_TOL if quant else SCALE_TOL_RAW)
    if pool is not None:
        for t, ref in zip((pa, pb), pool):
            o = t.cpu().numpy().astype(np.float64)
            assert np.isnan(o[P]).all(), "the pooled image past the last pair is untouched"
            err = np.abs(o[:P] - ref[:P]).max()
            print(f"  pooled: max err {err:.3e} bound {32 * U * xmax:.3e}")
            assert err <= 32 * U * xmax
    if quant and P == 3 and S in (16, 32, 64):
        # positions 0 .. n - 2 only (an off-by-one in n) would be far outside the bound
        assert min(np.abs(off[0] - ssim).max(), np.abs(off[1] - cs).max()) > 100 * SCALE_TOL


# ------------------------------------------------------------------ end to end
@functools.lru_cache(maxsize=None)
def e2e_case(R):
    a, b = M.make_pairs(R, R, 3)
    return a, b, M.pair_values(a, b)[0]


def run_metric(ops, a, b, split):
    from pggan_amd.metrics import MultiScaleSSIM
    m = MultiScaleSSIM(ops, a.shape[-1], a.shape[0])
    for part in torch.split(dev(M.interleave(a, b)), split):
        m.feed(part)
    return m, m.values()


@pytest.mark.parametrize("R", [16, 32, 64, 256])
def test_end_to_end(ops, R):
    a, b, ref = e2e_case(R)
    assert ref.min() > 0.6 and ref.max() < 0.97
    m, got = run_metric(ops, a, b, [1, 3, 2])
    assert got.dtype == torch.float32 and got.shape == (3,)
    err = np.abs(got.cpu().numpy().astype(np.float64) - ref).max()
    print(f"end to end R={R}: values {got.tolist()} ref {ref.tolist()} worst err {err:.3e}")
    assert err <= E2E_TOL
    assert abs(m.result() - ref.mean()) <= E2E_TOL
    assert torch.equal(run_metric(ops, a, b, [1, 3, 2])[1], got), "two runs are bitwise equal"
    assert torch.equal(run_metric(ops, a, b, [6])[1], got), "however the stream is split"
    if R == 16:
        # a window centred half a sample off at the even sizes (8, 4, 2) is far outside the bound
        wrong = M.pair_values(a, b, centre_shift=0.5)[0]
        print(f"  centre off by half a sample: {np.abs(wrong - ref).max():.3e}")
        assert np.abs(wrong - ref).min() > 100 * E2E_TOL


@pytest.mark.parametrize("R", [16, 64])
def test_identical_and_negated_pairs(ops, R):
    a = e2e_case(R)[0]
    assert run_metric(ops, a, a.copy(), [6])[1].tolist() == [1.0, 1.0, 1.0]
    # b = 255 - a on the 8-bit grid: negative means are clipped to 0
    assert run_metric(ops, a, -a, [6])[1].tolist() == [0.0, 0.0, 0.0]


# ------------------------------------------------------------------ model level
def model(tmp_path, replay, pairs):
    args = make_args(tmp_path, depths=list(TINY_DEPTHS), ema_decay=0.5, use_validation=True,
                     swd_images=8, valid_cycle=1, msssim_pairs=pairs)
    m = build(args, False, 2)
    m.use_replay = replay
    m.set_validation()
    m.G.alpha = m.D.alpha = 0.5
    return m


@pytest.mark.parametrize("replay", [False, True])
def test_validation_leaves_training_alone(tmp_path, replay):
    with_, without = model(tmp_path / "a", replay, 3), model(tmp_path / "b", replay, None)
    for step in range(4):
        for m in (with_, without):
            m.train_step()
        out, old = with_.validation(step), without.validation(step)
        assert list(old) == [16, "avg"] and list(out) == [16, "avg", "msssim", "msssim_real"]
        assert {k: out[k] for k in old} == old
        assert 0.0 <= out["msssim_real"] <= 1.0 and 0.0 <= out["msssim"] <= 1.0
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
    x, sums, pa, pb = z(2, 3, 16, 16), z(1, 2), z(1, 3, 8, 8), z(1, 3, 8, 8)
    with pytest.raises(RuntimeError, match="msssim_scale"):
        ops.msssim_scale(x[0::2], x[1::2], [1 / 12] * 12, True, sums, pa, pb)      # T > 11
    with pytest.raises(RuntimeError, match="msssim_scale"):
        ops.msssim_scale(x[0::2, :, :8, :8], x[1::2, :, :8, :8], [0.25] * 4, True, sums)   # rows not contiguous
    y = z(2, 3, 15, 15)
    with pytest.raises(RuntimeError, match="msssim_scale"):
        ops.msssim_scale(y[0::2], y[1::2], [1 / 11] * 11, True, sums, z(1, 3, 7, 7), z(1, 3, 7, 7))
    with pytest.raises(RuntimeError, match="CPU tensor"):
        ops.msssim_scale(x[0::2].cpu(), x[1::2], [1 / 11] * 11, True, sums)
    out = z(1)
    with pytest.raises(RuntimeError, match="msssim_combine"):
        ops.msssim_combine(z(5, 1, 2), [108, 3, 3, 0, 3], out)
    torch.cuda.synchronize()
    for t in (sums, pa, pb, out):
        assert bool((t == 3.0).all()), "outputs are left unwritten"
