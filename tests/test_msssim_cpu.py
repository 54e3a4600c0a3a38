"""The MS-SSIM validation metric without a GPU: the float64 reference (tests/msssim_ref.py)
against the closed forms of its definition, MultiScaleSSIM's host logic over the numpy op
double, and ProgressiveGAN.validation with `msssim_pairs` on the CPU test double.

Bound of the double against the reference (DOUBLE_TOL): the double rounds each of a pair's sums
once into fp32 (relative 2^-24) and the pair value once more; the value is a product of means
raised to weights that sum to 1, so its relative error is at most 2 * 2^-24, on values <= 1."""
import ctypes
import os

import numpy as np
import pytest
import torch

import msssim_ref as M
import swd_ref
from cpu_ops import CpuOps
from pggan_amd import metrics, nets
from pggan_amd.metrics import MultiScaleSSIM
from pggan_amd.model import ProgressiveGAN
from test_model_api import fresh_model, make_args
from test_swd_cpu import assert_unchanged, snapshot

DOUBLE_TOL = 3 * 2.0 ** -24


class MsCpuOps(M.CpuMsssimOps, swd_ref.CpuSwdOps, CpuOps):
    pass


def stream(R, seed, P):
    a, b = M.make_pairs(R, seed, P)
    return torch.from_numpy(M.interleave(a, b))


# ------------------------------------------------------------------ the reference itself
@pytest.mark.parametrize("S,T", [(16, 11), (8, 8), (2, 2), (1, 1)])
def test_reference_window_matches_separable_taps(S, T):
    g = M.taps(S)
    assert len(g) == T and abs(g.sum() - 1) < 1e-15 and np.allclose(g, g[::-1], rtol=0, atol=1e-17)
    sigma = 1.5 * T / 11
    if T == 1:
        assert g.tolist() == [1.0]
    elif T == 2:
        assert g.tolist() == [0.5, 0.5], "half-integer positions: the two taps are equal"
    elif T == 8:      # positions -3.5 .. 3.5
        assert g[3] == g[4] and abs(g[2] / g[3] - np.exp(-(1.5 ** 2 - 0.5 ** 2) / (2 * sigma ** 2))) < 1e-15
    else:             # positions -5 .. 5, sigma 1.5
        assert sigma == 1.5 and abs(g[4] / g[5] - np.exp(-1 / 4.5)) < 1e-15 and g.argmax() == 5
    assert np.array_equal(metrics.msssim_taps(S), g.astype(np.float32)), "the host's taps"
    x = np.random.default_rng(S).normal(size=(2, 3, S, S)) * 50 + 100
    n = S - T + 1
    h = sum(g[t] * x[..., :, t:t + n] for t in range(T))
    sep = sum(g[t] * h[..., t:t + n, :] for t in range(T))
    got = M.filt(x, M.window2d(S))
    assert got.shape == (2, 3, n, n)
    assert np.abs(got - sep).max() <= 1e-12 * np.abs(x).max()


@pytest.mark.parametrize("S", [2, 4, 16])
def test_reference_down_is_the_aligned_mean(S):
    x = np.random.default_rng(S).normal(size=(2, 3, S, S))
    want = (x[..., 0::2, 0::2] + x[..., 0::2, 1::2] + x[..., 1::2, 0::2] + x[..., 1::2, 1::2]) / 4
    got = M.down(x)
    assert got.shape == want.shape and np.abs(got - want).max() <= 1e-15


def test_reference_one_by_one_scale_by_hand():
    """S = 1: one tap of weight 1, every variance 0, so cs = c2 / c2 = 1 and the ssim term is
    the luminance ratio alone."""
    a, b = np.array([10.0, 100.0, 250.0]), np.array([30.0, 90.0, 5.0])
    ssim, cs = M.scale_stats(a.reshape(3, 1, 1), b.reshape(3, 1, 1), M.window2d(1))
    want = np.mean((2 * a * b + M.C1) / (a * a + b * b + M.C1))
    assert cs == 1.0 and abs(ssim - want) < 1e-15
    # three channels by hand: (600 + c1) / (1000 + c1), (18000 + c1) / (18100 + c1), ..
    c1 = 6.5025
    hand = ((600 + c1) / (1000 + c1) + (18000 + c1) / (18100 + c1) + (2500 + c1) / (62525 + c1)) / 3
    assert abs(ssim - hand) < 1e-12


def test_reference_values_of_the_test_inputs():
    """What the GPU tests rely on: no clip fires and no factor is near 0 on these inputs."""
    for R in (16, 32, 64):
        a, b = M.make_pairs(R, R, 3)
        v, ssim, cs = M.pair_values(a, b)
        assert (v > 0.6).all() and (v < 0.97).all(), (R, v)
        assert cs[:4].min() >= 0.45 and ssim[4].min() >= 0.45, (R, cs, ssim)
    a, b = M.make_pairs(16, 1)
    assert M.pair_values(a, a)[0] == [1.0]
    assert M.pair_values(a, -a)[0] == [0.0], "b = 255 - a: a negative mean is clipped"
    g = np.random.default_rng(0)
    noise = g.uniform(-1, 1, (2, 3, 16, 16))
    assert M.pair_values(noise[:1], noise[1:])[0][0] < 0.05, "independent noise: near 0"


# ------------------------------------------------------------------ MultiScaleSSIM
@pytest.mark.parametrize("R", [16, 32])
def test_matches_reference(R):
    x = stream(R, 3, 3)
    m = MultiScaleSSIM(MsCpuOps(), R, 3)
    m.feed(x)
    ref = M.pair_values(x.numpy()[0::2], x.numpy()[1::2])[0]
    got = m.values()
    assert got.dtype == torch.float32 and got.shape == (3,)
    err = np.abs(got.numpy().astype(np.float64) - ref).max()
    print(f"R={R}: values {got.tolist()} worst err {err:.3e}")
    assert err <= DOUBLE_TOL
    res = m.result()
    assert isinstance(res, float) and res == float(got.double().mean())
    assert abs(res - M.msssim_reference(x.numpy())) <= DOUBLE_TOL
    assert m.sizes == [R >> s for s in range(5)]
    assert m.counts == [3 * (s - min(11, s) + 1) ** 2 for s in m.sizes]
    if R == 16:
        assert [len(t) for t in m.taps] == [11, 8, 4, 2, 1]


def test_split_equals_one_batch():
    x = stream(16, 5, 2)
    whole = MultiScaleSSIM(MsCpuOps(), 16, 2)
    whole.feed(x)
    parts = MultiScaleSSIM(MsCpuOps(), 16, 2)
    held = x[:1]
    parts.feed(held)
    held.add_(7.0)                # the held image is a copy: the caller may reuse its buffer
    parts.feed(x[1:])
    assert torch.equal(whole.values(), parts.values()) and whole.result() == parts.result()
    ones = MultiScaleSSIM(MsCpuOps(), 16, 2)
    x = stream(16, 5, 2)
    for i in range(4):
        ones.feed(x[i:i + 1])
    assert torch.equal(ones.values(), whole.values())


def test_argument_errors():
    ops = MsCpuOps()
    for bad in (8, 48):
        with pytest.raises(ValueError, match="resolution"):
            MultiScaleSSIM(ops, bad, 4)
    with pytest.raises(ValueError, match="n_pairs"):
        MultiScaleSSIM(ops, 16, 0)
    m = MultiScaleSSIM(ops, 16, 2)
    with pytest.raises(ValueError, match="expected"):
        m.feed(torch.zeros(2, 3, 32, 32))
    with pytest.raises(RuntimeError, match="0 of 4"):
        m.result()
    x = stream(16, 1, 3)
    m.feed(x[:3])
    with pytest.raises(RuntimeError, match="3 of 4"):
        m.result()
    with pytest.raises(RuntimeError, match="3 of 4"):
        m.values()
    with pytest.raises(ValueError, match="exceed"):
        m.feed(x[3:5])
    m.feed(x[3:4])
    assert 0.0 < m.result() < 1.0


def test_entry_points_reject_bad_arguments():
    """Both entry points refuse on the host, before any launch (the pointers here are never
    dereferenced on the device), naming themselves in the message."""
    from pggan_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libpggan_hip.so not built")
    lib = _lib.load_library()
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    cnt = (ctypes.c_longlong * 5)(108, 3, 3, 3, 3)
    big = 1 << 20

    def scale(S, T, taps=p, a=p, b=p, sums=p, pa=None, pb=None, ws=p, wsb=big, P=1):
        return lib.pg_msssim_scale(P, S, T, taps, a, b, 3 * S * S, 0, sums, pa, pb, ws, wsb, None)

    calls = {
        "msssim_scale": [lambda: scale(15, 11, pa=p, pb=p),          # odd S with pooled outputs
                         lambda: scale(8, 11),                       # T > S
                         lambda: scale(16, 12),                      # T > 11
                         lambda: scale(16, 0),                       # T < 1
                         lambda: scale(16, 11, taps=None),
                         lambda: scale(16, 11, a=None),
                         lambda: scale(16, 11, b=None),
                         lambda: scale(16, 11, sums=None),
                         lambda: scale(16, 11, ws=None),
                         lambda: scale(16, 11, pa=p),                # one pooled side only
                         lambda: scale(42, 11, pa=p, pb=p),          # n = 32: one tile, 10 columns unowned
                         lambda: scale(16, 11, wsb=4),               # workspace too small
                         lambda: scale(16, 11, P=0)],
        "msssim_combine": [lambda: lib.pg_msssim_combine(1, None, cnt, p, None),
                           lambda: lib.pg_msssim_combine(1, p, None, p, None),
                           lambda: lib.pg_msssim_combine(1, p, cnt, None, None),
                           lambda: lib.pg_msssim_combine(0, p, cnt, p, None)],
    }
    for name, fns in calls.items():
        for i, fn in enumerate(fns):
            assert fn() == -1, (name, i)
            assert name.encode() in lib.pg_last_error(), (name, i, lib.pg_last_error())
    assert lib.pg_msssim_workspace_bytes(3, 64, 11) == 3 * 3 * 4 * 2 * 4, "54 positions: 2 x 2 tiles"
    assert lib.pg_msssim_workspace_bytes(1, 16, 11) == 3 * 2 * 4


# ------------------------------------------------------------------ ProgressiveGAN.validation
@pytest.fixture
def cpu_model(monkeypatch):
    monkeypatch.setattr(ProgressiveGAN, "ops_factory", staticmethod(MsCpuOps))
    monkeypatch.setattr(nets, "OPS_FACTORY", MsCpuOps)
    nets._ENGINES.clear()

    def make(tmp_path, **over):
        torch.manual_seed(11)
        m = fresh_model(make_args(tmp_path, **dict(dict(swd_images=8, use_validation=True), **over)))
        m.set_validation()
        for _ in range(2):
            m.change_scale(0)
        m.G.alpha = m.D.alpha = 0.5
        return m
    return make


def test_validation_with_msssim_pairs(tmp_path, cpu_model):
    on, off = cpu_model(tmp_path / "on", msssim_pairs=3), cpu_model(tmp_path / "off")
    for m in (on, off):
        m.train_step()
    before = snapshot(on)
    out, old = on.validation(7), off.validation(7)
    assert_unchanged(on, before)
    assert list(old) == [16, "avg"], "the key blank: exactly the dict as before"
    assert list(out) == [16, "avg", "msssim", "msssim_real"]
    assert {k: out[k] for k in old} == old, "the SWD figures do not change"
    # the first 6 of the 8 fakes validation samples (batches of 4), paired up
    g = torch.Generator().manual_seed(0)
    fakes = torch.cat([on.sample(torch.randn(4, on.args.latent_dim, generator=g), ema=False)
                       for _ in range(2)])
    ref = M.msssim_reference(fakes[:6].numpy())
    reals = torch.cat(list(on._validation.reals(16, 8, 4)))
    ref_real = M.msssim_reference(reals[:6].numpy())
    print(f"msssim {out['msssim']} ref {ref}; reals {out['msssim_real']} ref {ref_real}")
    assert isinstance(out["msssim"], float) and isinstance(out["msssim_real"], float)
    assert abs(out["msssim"] - ref) <= DOUBLE_TOL and abs(out["msssim_real"] - ref_real) <= DOUBLE_TOL
    assert 0.0 <= out["msssim_real"] < out["msssim"] <= 1.0, "uniform noise is the most diverse"
    assert on.validation(8) == out
    d_on, d_off = os.path.join(str(tmp_path), "on", "t"), os.path.join(str(tmp_path), "off", "t")
    rows = open(os.path.join(d_on, "msssim.csv")).read().splitlines()
    assert [r.split(",")[:2] for r in rows] == [["7", "2"], ["8", "2"]]
    assert [float(v) for v in rows[0].split(",")[2:]] == [out["msssim"], out["msssim_real"]]
    assert sorted(os.listdir(d_off)) == ["swd.csv"], "the key blank: no new file"
    assert open(os.path.join(d_on, "swd.csv")).read().splitlines()[0] == \
        open(os.path.join(d_off, "swd.csv")).read().splitlines()[0]
    # training goes on exactly as without it
    for m in (on, off):
        m.train_step()
    assert torch.equal(on.fpG.flat, off.fpG.flat) and torch.equal(on.fpD.flat, off.fpD.flat)


def test_validation_prints_on_the_master(tmp_path, cpu_model, capsys):
    m = cpu_model(tmp_path, msssim_pairs=4, isMaster=True)
    out = m.validation(3)
    lines = [l for l in capsys.readouterr().out.splitlines() if l.startswith("step 3:")]
    assert len(lines) == 2 and lines[0].startswith("step 3: SWD x1e3")
    assert lines[1] == f"step 3: MS-SSIM {out['msssim']:.4f} (reals {out['msssim_real']:.4f})"


def test_too_many_pairs_raise(tmp_path, cpu_model):
    with pytest.raises(ValueError, match="msssim_pairs"):
        cpu_model(tmp_path, msssim_pairs=5)          # 10 > swd_images = 8
    off = cpu_model(tmp_path, msssim_pairs=3, use_validation=False)
    assert off.validation(0) is None
