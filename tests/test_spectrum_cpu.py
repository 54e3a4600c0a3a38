"""The power-spectrum validation metric without a GPU: the integer binning, the float64
reference (tests/spectrum_ref.py) and PowerSpectrum's host logic against closed forms,
spectrum_compare's figures, and ProgressiveGAN.validation with `spectrum_images` on the CPU
test doubles."""
import ctypes
import glob
import os

import numpy as np
import pytest
import torch

import spectrum_ref as S
from pggan_amd import metrics, nets
from pggan_amd.metrics import PowerSpectrum, spectrum_bin_counts, spectrum_compare
from pggan_amd.model import ProgressiveGAN
from test_model_api import fresh_model, make_args
from test_swd_cpu import assert_unchanged, snapshot
from test_validation_cpu import AllCpuOps


class SpecCpuOps(S.CpuSpectrumOps, AllCpuOps):
    pass


SIZES = [8, 16, 32, 64, 128, 256, 512, 1024]


# ------------------------------------------------------------------ binning
@pytest.mark.parametrize("R", SIZES)
def test_integer_binning_is_round_of_the_radius(R):
    f = np.arange(-R // 2, R // 2, dtype=np.int64)
    r2 = f[:, None] ** 2 + f[None, :] ** 2
    k = metrics.spectrum_bin_index(r2)
    assert np.array_equal(k, np.floor(np.sqrt(r2.astype(np.float64)) + 0.5).astype(np.int64))
    assert ((k * k - k < r2) | (r2 == 0)).all() and (r2 <= k * k + k).all(), "the rule itself"
    assert k[R // 2, R // 2] == 0
    cnt = spectrum_bin_counts(R)
    assert cnt.shape == (R // 2 + 1,) and cnt.dtype == np.int64
    assert cnt.sum() == (k <= R // 2).sum() and cnt[0] == 1 and cnt[1] == 8
    assert np.array_equal(cnt, S.counts(R)), "the reference's own count"
    assert np.array_equal(metrics.spectrum_bins(R), S.bins(R)), "and its plane, in numpy.fft order"


# ------------------------------------------------------------------ known answers
def profile_of(x, quantize, split=None):
    m = PowerSpectrum(SpecCpuOps(), x.shape[-1], quantize=quantize)
    for part in torch.split(torch.as_tensor(x), split or [len(x)]):
        m.feed(part)
    return m


@pytest.mark.parametrize("R", [8, 32, 256])
def test_constant_image(R):
    m = profile_of(np.zeros((2, 3, R, R), np.float32), True)      # q = 128 (the tie goes up to even)
    per = m.per_image().numpy().astype(np.float64)
    assert m.count == 2 and per.shape == (2, R // 2 + 1)
    want = (0.5 * R * R) ** 2
    assert np.allclose(per[:, 0], want, rtol=1e-6, atol=0) and (np.abs(per[:, 1:]) <= 1e-9 * want).all()
    prof = m.profile()
    assert prof.dtype == np.float64 and prof.shape == (R // 2 + 1,)
    assert abs(prof[0] - want) <= 1e-6 * want, "bin 0 holds one point"


@pytest.mark.parametrize("R", [32, 256])
def test_cosine_lands_in_bin_five(R):
    amp = 40.0
    a = profile_of(S.cosine_image(R, 3, 4, amp), False).per_image().numpy().astype(np.float64)[0]
    b = profile_of(S.cosine_image(R, 4, 3, amp), False).per_image().numpy().astype(np.float64)[0]
    want = 2 * (amp * R * R / 2) ** 2
    assert abs(a[5] - want) <= 1e-6 * want
    assert (np.abs(np.delete(a, 5)) <= 1e-9 * want).all(), "nothing off bin 5, bin 0 included"
    assert np.allclose(a, b, rtol=1e-9, atol=1e-9 * want), "the transposed pattern"


def test_reference_variants_differ():
    x = S.make_images(64, 64, 3)
    assert (np.abs(x) == 1.0).mean() < 1e-3, "under 0.1 % of the values clip"
    ref = S.profile64(x)
    assert ref.min() > 0
    rel = lambda other: (np.abs(other - ref) / ref).max()
    assert rel(S.profile64(x, binning="floor")) > 0.3
    assert rel(S.profile64(x, luma="mean")) > 0.5


# ------------------------------------------------------------------ compare
def test_compare():
    R = 64
    real = S.make_images(R, 1, 6)
    u8 = real.astype(np.float64) * 127.5 + 127.5
    g = np.random.default_rng(2)
    back = lambda v: ((np.rint(np.clip(v, 0, 255)) - 127.5) / 127.5).astype(np.float32)
    noisy = back(u8 + g.normal(0, 10, u8.shape))
    blur = back((u8 + np.roll(u8, 1, -1) + np.roll(u8, 1, -2) + np.roll(u8, (1, 1), (-2, -1))) / 4)
    s_real = profile_of(real, True).profile()
    assert np.allclose(s_real, S.set_profile(real), rtol=1e-6, atol=0)
    db, dist, hf = spectrum_compare(s_real, s_real)
    assert db.shape == (R // 2,) and not db.any() and dist == 0.0 and hf == 0.0
    db, dist, hf = spectrum_compare(s_real, profile_of(noisy, True).profile())
    assert hf > 0 and dist > 0 and isinstance(dist, float) and isinstance(hf, float)
    assert hf == db[3 * (R // 2) // 4:].mean() and dist == np.abs(db).mean()
    db, dist, hf = spectrum_compare(s_real, profile_of(blur, True).profile())
    assert hf < 0 and dist > 0
    # empty bins on either side: floored, never inf or nan
    zero = np.zeros_like(s_real)
    for a, b in ((zero, s_real), (s_real, zero), (zero, zero)):
        db, dist, hf = spectrum_compare(a, b)
        assert np.isfinite(db).all() and np.isfinite(dist) and np.isfinite(hf)
    assert spectrum_compare(zero, zero)[1] == 0.0


def test_feeding_in_pieces():
    x = S.make_images(16, 5, 6)
    whole, parts = profile_of(x, True, [6]), profile_of(x, True, [1, 3, 2])
    assert parts.count == whole.count == 6
    assert torch.equal(parts.per_image(), whole.per_image())
    assert np.array_equal(parts.profile(), whole.profile())
    parts.feed(torch.zeros(0, 3, 16, 16))
    assert parts.count == 6, "an empty batch is accepted"


def test_argument_errors():
    ops = SpecCpuOps()
    for bad in (4, 24, 2048):
        with pytest.raises(ValueError, match="resolution"):
            PowerSpectrum(ops, bad)
    m = PowerSpectrum(ops, 16)
    for shape in ((2, 3, 8, 8), (2, 1, 16, 16), (3, 16, 16)):
        with pytest.raises(ValueError, match="expected"):
            m.feed(torch.zeros(shape))
    with pytest.raises(RuntimeError, match="no image"):
        m.profile()


def test_entry_point_rejects_bad_arguments():
    """pg_spectrum_profile refuses on the host, before any launch (the pointers here are never
    dereferenced on the device), naming itself in the message."""
    from pggan_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libpggan_hip.so not built")
    lib = _lib.load_library()
    buf = (ctypes.c_float * 64)()
    base = (ctypes.addressof(buf) + 15) & ~15
    p, odd = ctypes.c_void_p(base), ctypes.c_void_p(base + 4)

    def call(B=1, R=128, x=p, prof=p, ws=p, wsb=1 << 30):
        return lib.pg_spectrum_profile(B, R, x, 1, prof, ws, wsb, None)

    for i, fn in enumerate([lambda: call(R=24), lambda: call(R=4), lambda: call(R=2048),
                            lambda: call(R=0), lambda: call(B=0), lambda: call(B=65536),
                            lambda: call(x=None), lambda: call(prof=None), lambda: call(ws=None),
                            lambda: call(x=odd), lambda: call(prof=odd), lambda: call(ws=odd),
                            lambda: call(wsb=lib.pg_spectrum_workspace_bytes(1, 128) - 1),
                            lambda: call(R=16, wsb=0)]):
        assert fn() == -1, i
        assert b"spectrum_profile" in lib.pg_last_error(), (i, lib.pg_last_error())
    size = lib.pg_spectrum_workspace_bytes
    assert size(1, 24) == size(0, 64) == size(1, 2048) == size(65536, 64) == 0
    assert size(1, 8) == size(500, 64) == 16, "the one-launch form needs no workspace"

    def want(n, R, lines):      # n images' half spectra [R/2+1][R] complex + their partials
        nk = R // 2 + 1
        return n * nk * R * 8 + (n * -(-nk // lines) * nk * 4 + 15) // 16 * 16

    assert size(1, 128) == want(1, 128, 8) and size(3, 1024) == want(3, 1024, 4)
    assert size(7, 1024) == size(64, 1024) == want(7, 1024, 4), "32 MB of half spectra at a time"


# ------------------------------------------------------------------ the validation part
@pytest.fixture
def cpu_model(monkeypatch):
    torch.set_num_threads(4)
    monkeypatch.setattr(ProgressiveGAN, "ops_factory", staticmethod(SpecCpuOps))
    monkeypatch.setattr(nets, "OPS_FACTORY", SpecCpuOps)
    nets._ENGINES.clear()

    def make(tmp_path, stage, **over):
        torch.manual_seed(11)
        m = fresh_model(make_args(tmp_path, swd_images=8, use_validation=True, isMaster=True, **over))
        m.set_validation()
        for _ in range(stage):
            m.change_scale(0)
        m.G.alpha = m.D.alpha = 0.5
        return m
    yield make
    nets._ENGINES.clear()


def validate(m, capsys):
    capsys.readouterr()
    before = snapshot(m)
    out = m.validation(5)
    assert_unchanged(m, before)
    return out, [l for l in capsys.readouterr().out.splitlines() if l.startswith("step 5:")]


def test_validation_with_spectrum_images(tmp_path, cpu_model, capsys):
    on = cpu_model(tmp_path / "on", 2, msssim_pairs=2, spectrum_images=4)
    off = cpu_model(tmp_path / "off", 2, msssim_pairs=2)
    out, lines = validate(on, capsys)
    old, old_lines = validate(off, capsys)
    assert list(old) == [16, "avg", "msssim", "msssim_real"]
    assert list(out) == list(old) + ["spec_dist", "spec_hf"]
    assert {k: out[k] for k in old} == old
    assert isinstance(out["spec_dist"], float) and out["spec_dist"] >= 0 and np.isfinite(out["spec_hf"])
    assert lines[:-1] == old_lines
    assert lines[-1] == (f"step 5: power spectrum, dB fake/real: mean |.| {out['spec_dist']:.3f}, "
                         f"top quarter {out['spec_hf']:+.3f}")
    d_on, d_off = (os.path.join(str(tmp_path), n, "t") for n in ("on", "off"))
    csvs = lambda d: {os.path.basename(p): open(p, "rb").read() for p in glob.glob(d + "/*.csv")}
    assert sorted(csvs(d_off)) == ["msssim.csv", "swd.csv"] and not os.path.exists(d_off + "/spectrum")
    assert sorted(csvs(d_on)) == ["msssim.csv", "spectrum.csv", "swd.csv"]
    for f, data in csvs(d_off).items():
        assert csvs(d_on)[f] == data, f
    row = open(d_on + "/spectrum.csv").read().splitlines()
    assert len(row) == 1 and row[0].split(",")[:2] == ["5", "2"]
    assert [float(v) for v in row[0].split(",")[2:]] == [out["spec_dist"], out["spec_hf"]]
    table = [l.split(",") for l in open(d_on + "/spectrum/e5.csv").read().splitlines()]
    assert len(table) == 9 and [int(r[0]) for r in table] == list(range(9))
    s_real, s_fake = (np.array([float(r[c]) for r in table]) for c in (1, 2))
    _, dist, hf = spectrum_compare(s_real, s_fake)
    assert (dist, hf) == (out["spec_dist"], out["spec_hf"]), "the table's floats read back exactly"
    assert [float(r[3]) for r in table][1:] == spectrum_compare(s_real, s_fake)[0].tolist()
    # the figures are those of the reference over the images the run streamed
    reals = torch.cat(list(on._validation.reals(16, 4, 4))).numpy()
    fakes = torch.cat([x.float() for x in on._validation.fakes(4, 4)]).numpy()
    assert np.allclose(s_real, S.set_profile(reals), rtol=1e-6, atol=0)
    assert np.allclose(s_fake, S.set_profile(fakes), rtol=1e-6, atol=0)
    # a second validation of the same step replaces the table and appends to the history
    on.validation(5)
    assert len(open(d_on + "/spectrum/e5.csv").read().splitlines()) == 9
    assert len(open(d_on + "/spectrum.csv").read().splitlines()) == 2


@pytest.mark.parametrize("stage", [0, 1], ids=["4x4", "8x8"])
def test_undefined_below_16(tmp_path, cpu_model, capsys, stage):
    m = cpu_model(tmp_path, stage, spectrum_images=4)
    out, lines = validate(m, capsys)
    R = 4 * 2 ** stage
    assert out is None
    assert lines == [f"step 5: SWD is undefined below 16x16 (stage is {R}x{R})",
                     f"step 5: the power spectrum is undefined below 16x16 (stage is {R}x{R})"]
    assert not glob.glob(os.path.join(str(tmp_path), "t", "spectrum*"))


def test_settings(tmp_path, cpu_model):
    with pytest.raises(ValueError, match="spectrum_images"):
        cpu_model(tmp_path, 0, spectrum_images=9)          # > swd_images = 8
    with pytest.raises(ValueError, match="spectrum_images"):
        cpu_model(tmp_path, 0, spectrum_images=-1)
    assert cpu_model(tmp_path, 0, spectrum_images=8)._validation.settings.spectrum_images == 8
    assert cpu_model(tmp_path, 0)._validation.settings.spectrum_images is None
