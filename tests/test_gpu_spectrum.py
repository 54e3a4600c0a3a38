"""The power-spectrum kernels (pggan_amd/csrc/spectrum.hip) and the metric built on them, on
the GPU, against the float64 reference of tests/spectrum_ref.py.

Inputs (spectrum_ref.make_images): on the 8-bit grid, a sinusoid pattern + N(0, 25) per channel,
so every radius bin holds substantial power and a relative bound per bin means something; the
`quantize=False` cases take the same images on the 0..255 scale plus N(0, 1), off the grid.

Bound: |got[k] - ref[k]| <= TOL * ref[k] in every bin, TOL = 4 x the worst relative error
measured on an MI355X (each test prints its figures), under the cap 1e-4 (0.0004 dB, below the
third decimal the metric prints):
  MEASURED  2.86e-6 at worst (R = 32, B = 3, off the grid; 2.17e-6 on it), 1.7e-6 at R = 256,
            5.6e-7 at R = 1024, 1.5e-7 .. 1.1e-6 elsewhere; the worst bin is bin 0, a single
            point whose power is what the shift by 127.5 leaves of the mean
The end-to-end figures came out within 9e-7 dB of the float64 ones (bound 2e-4 dB).  The wrong variants of the reference (floor instead of round in the binning, the channel mean
instead of the luma weights) are more than 100 x TOL away (asserted below)."""
import functools
import math

import numpy as np
import pytest
import torch

import spectrum_ref as S
from gen_inputs import TINY_DEPTHS
from test_gpu_graph import build
from test_model_api import make_args

pytestmark = pytest.mark.gpu

MEASURED = 2.86e-6
TOL = 4 * MEASURED
assert TOL <= 1e-4, "the cap"
DB_TOL = 10 * math.log10(1 + 2 * TOL) * 2


@pytest.fixture(scope="module")
def ops():
    from pggan_amd import _lib
    return _lib.HipOps(torch.float32)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def run_op(ops, x, quant):
    """prof [B, K + 1] as float64 numpy; the row past the last image must stay untouched."""
    B, K = x.shape[0], x.shape[-1] // 2
    out = torch.full((B + 1, K + 1), float("nan"), device="cuda")
    ops.spectrum_profile(x, quant, out[:B])
    got = out.cpu().numpy()
    assert np.isnan(got[B]).all(), "the row past the last image is untouched"
    return got[:B]


# ------------------------------------------------------------------ the op, per bin
@functools.lru_cache(maxsize=None)
def case(R, quant):
    """Three images at side R (one at 1024) and their float64 profiles."""
    x = S.make_images(R, 300 + R, 1 if R == 1024 else 3)
    if not quant:
        g = np.random.default_rng(400 + R)
        x = (x.astype(np.float64) * 127.5 + 127.5 + g.normal(0, 1, x.shape)).astype(np.float32)
    return x, S.profile64(x, quant)


@pytest.mark.parametrize("quant", [True, False])
@pytest.mark.parametrize("R,B", [(R, B) for R in (8, 16, 32, 64, 128, 256) for B in (1, 3)] +
                         [(1024, 1)])
def test_profile(ops, R, B, quant):
    x, ref = case(R, quant)
    got = run_op(ops, dev(x[:B]), quant).astype(np.float64)
    assert ref.min() > 0
    err = (np.abs(got - ref[:B]) / ref[:B]).max()
    print(f"spectrum_profile R={R} B={B} quant={quant}: worst relative error {err:.3e}")
    assert err <= TOL
    if B == 3 or R == 1024:
        for kw in (dict(binning="floor"), dict(luma="mean")):
            wrong = S.profile64(x, quant, **kw)
            assert (np.abs(wrong - ref) / ref).max() > 100 * TOL, kw


# ------------------------------------------------------------------ known answers
@pytest.mark.parametrize("R", [32, 256])
def test_known_answers(ops, R):
    got = run_op(ops, torch.zeros(2, 3, R, R, device="cuda"), True).astype(np.float64)
    want = (0.5 * R * R) ** 2                       # q = 128, y = 0.5
    print(f"constant R={R}: bin 0 {got[:, 0].tolist()} want {want}, largest other {np.abs(got[:, 1:]).max():.3e}")
    assert (np.abs(got[:, 0] - want) <= TOL * want).all()
    assert (np.abs(got[:, 1:]) <= 1e-9 * want).all()
    amp = 40.0
    want = 2 * (amp * R * R / 2) ** 2
    a = run_op(ops, dev(S.cosine_image(R, 3, 4, amp)), False).astype(np.float64)[0]
    b = run_op(ops, dev(S.cosine_image(R, 4, 3, amp)), False).astype(np.float64)[0]
    for p in (a, b):
        print(f"cosine R={R}: bin 5 {p[5]:.9e} want {want:.9e}, largest other {np.abs(np.delete(p, 5)).max():.3e}")
        assert abs(p[5] - want) <= TOL * want
        assert (np.abs(np.delete(p, 5)) <= 1e-9 * want).all()


# ------------------------------------------------------------------ repeatability
def per_image(ops, x, split):
    from pggan_amd.metrics import PowerSpectrum
    m = PowerSpectrum(ops, x.shape[-1])
    for part in torch.split(x, split):
        m.feed(part)
    return m


@pytest.mark.parametrize("R", [16, 64, 128, 256])
def test_repeatable_and_independent_of_the_batch(ops, R):
    x = dev(S.make_images(R, 500 + R, 6))
    whole = per_image(ops, x, [6])
    got = whole.per_image()
    assert whole.count == 6 and got.dtype == torch.float32 and got.shape == (6, R // 2 + 1)
    assert torch.equal(per_image(ops, x, [6]).per_image(), got), "two runs are bitwise equal"
    assert torch.equal(per_image(ops, x, [1, 3, 2]).per_image(), got), "however the stream is split"
    alone = torch.empty(1, R // 2 + 1, device="cuda")
    last = torch.empty(3, R // 2 + 1, device="cuda")
    ops.spectrum_profile(x[2:3], True, alone)
    ops.spectrum_profile(x[0:3], True, last)
    assert torch.equal(alone[0], last[2]) and torch.equal(alone[0], got[2])


# ------------------------------------------------------------------ end to end
@pytest.mark.parametrize("R", [64, 256])
def test_end_to_end(ops, R):
    from pggan_amd.metrics import spectrum_compare
    real = S.make_images(R, 600 + R, 6)
    g = np.random.default_rng(700 + R)
    u8 = np.rint(np.clip(real.astype(np.float64) * 127.5 + 127.5 + g.normal(0, 10, real.shape), 0, 255))
    fake = ((u8 - 127.5) / 127.5).astype(np.float32)
    db, dist, hf = spectrum_compare(per_image(ops, dev(real), [1, 3, 2]).profile(),
                                    per_image(ops, dev(fake), [6]).profile())
    rdb, rdist, rhf = spectrum_compare(S.set_profile(real), S.set_profile(fake))
    print(f"end to end R={R}: spec_dist {dist:.6f} (ref {rdist:.6f}) spec_hf {hf:+.6f} (ref {rhf:+.6f}) "
          f"worst bin {np.abs(db - rdb).max():.3e} dB, bound {DB_TOL:.3e}")
    assert rhf > 0.1, "the added noise shows in the top quarter"
    assert abs(dist - rdist) <= DB_TOL and abs(hf - rhf) <= DB_TOL


# ------------------------------------------------------------------ model level
def model(tmp_path, replay, n):
    args = make_args(tmp_path, depths=list(TINY_DEPTHS), ema_decay=0.5, use_validation=True,
                     swd_images=8, valid_cycle=1, spectrum_images=n)
    m = build(args, False, 2)
    m.use_replay = replay
    m.set_validation()
    m.G.alpha = m.D.alpha = 0.5
    return m


@pytest.mark.parametrize("replay", [False, True])
def test_validation_leaves_training_alone(tmp_path, replay):
    with_, without = model(tmp_path / "a", replay, 4), model(tmp_path / "b", replay, None)
    for step in range(4):
        for m in (with_, without):
            m.train_step()
        out, old = with_.validation(step), without.validation(step)
        assert list(old) == [16, "avg"] and list(out) == [16, "avg", "spec_dist", "spec_hf"]
        assert {k: out[k] for k in old} == old
        assert out["spec_dist"] >= 0 and math.isfinite(out["spec_dist"]) and math.isfinite(out["spec_hf"])
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
    outs = []

    def refused(x, out, match="spectrum_profile"):
        outs.append(out)
        with pytest.raises(RuntimeError, match=match):
            ops.spectrum_profile(x, True, out)

    refused(z(1, 3, 24, 24), z(1, 13))                       # not a power of two
    refused(z(1, 3, 2048, 2048), z(1, 1025))                 # too large
    refused(z(2, 3, 32, 32)[:, :, :16, :16], z(2, 9))        # rows not contiguous
    refused(z(2, 3, 16, 16).cpu(), z(2, 9), "CPU tensor")
    refused(z(2, 3, 16, 16), z(2, 8))                        # out of the wrong length
    refused(z(2, 3, 16, 16), z(3, 9))
    torch.cuda.synchronize()
    for t in outs:
        assert bool((t == 3.0).all()), "outputs are left unwritten"
