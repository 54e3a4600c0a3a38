"""The sliced Wasserstein validation metric without a GPU: the float64 reference
(tests/swd_ref.py) against the closed forms of its two filters, SlicedWasserstein's host logic
over the numpy op double, and ProgressiveGAN.validation on the CPU test double.

End-to-end bound (swd_bound): the sorted-L1 mean is 1-Lipschitz in the sup norm of each set's
projections, so |swd - ref| <= eps_A + eps_B with eps the largest projection error of a set.
A projection of a unit direction errs by at most ||delta d||_2 + 160 * 2^-24 * ||d||_2 (d the
normalised descriptor); delta d comes from the descriptor error -- a level-l pyramid value is
held to 32 (l + 1) 2^-24 * 255, the Laplacian adds one more filter -- times 1 / std, over 147
entries.  All of it is evaluated on the reference's own float64 descriptors."""
import os

import numpy as np
import pytest
import torch

import swd_ref as R
from cpu_ops import CpuOps
from pggan_amd import metrics, nets
from pggan_amd.metrics import SlicedWasserstein
from pggan_amd.model import ProgressiveGAN
from test_model_api import fresh_model, make_args


class SwdCpuOps(R.CpuSwdOps, CpuOps):
    pass


def images(n, res, seed, kind="noise"):
    """Two visibly different image distributions on the u8 grid's interior (fp32 [-1, 1])."""
    g = np.random.default_rng(seed)
    x = g.uniform(-1, 1, (n, 3, res, res))
    if kind == "smooth":
        x = 0.6 * R._filt(x) * 3 + 0.2 * g.uniform(-1, 1, (n, 3, 1, 1))
    return torch.from_numpy(np.clip(x, -1, 1).astype(np.float32))


def positions_of(m):
    return {w: [metrics.draw_positions(m.seed, l, 0, m.n_images, s, m.K).numpy()
                for l, s in enumerate(m.sizes)] for w in metrics.SETS}


def reference_of(m, real, fake):
    dirs = metrics.draw_directions(m.seed, m.repeats, m.P).numpy()
    return R.swd_reference(real.numpy(), fake.numpy(), positions_of(m), dirs, m.K, m.quantize)


def swd_bound(m, real, fake):
    """The bound of the module docstring per level, x 1e3 like the values."""
    pos, out = positions_of(m), {}
    laps = {"real": R.laplacian_pyramid(real.numpy(), m.quantize),
            "fake": R.laplacian_pyramid(fake.numpy(), m.quantize)}
    for l, s in enumerate(m.sizes):
        eps = 0.0
        for w in metrics.SETS:
            d = R.gather(laps[w][l], pos[w][l], m.K).reshape(-1, 3, 49)
            rstd = 1.0 / d.std(axis=(0, 2)).min()
            dmax = np.linalg.norm(R.normalize(d), axis=1).max()
            e_desc = 32 * (l + 2) * R.U24 * 255.0
            eps += np.sqrt(147.0) * e_desc * rstd + 160 * R.U24 * dmax
        out[s] = 1e3 * eps
    return out


def run(ops, real, fake, split=None, **kw):
    m = SlicedWasserstein(ops, real.shape[-1], real.shape[0], **kw)
    for w, x in (("real", real), ("fake", fake)):
        for part in (torch.split(x, split) if split else (x,)):
            m.feed(w, part)
    return m, m.result()


# ------------------------------------------------------------------ the reference itself
@pytest.mark.parametrize("n", [8, 16])
def test_reference_filters_match_closed_forms(n):
    g = np.random.default_rng(n)
    c, x = g.normal(size=n), g.normal(size=2 * n)
    up = R.pyr_up(np.outer(c, np.ones(n)))[:, 0]           # constant along x: the 1-D filter
    assert np.abs(up - R.up_1d_closed(c)).max() <= 1e-15 * np.abs(c).max() * 8
    # the two edges differ: out[2n-1] = c[n-1], out[2n-2] = (c[n-2] + 7 c[n-1]) / 8,
    # out[0] = (6 c[0] + 2 c[1]) / 8
    assert abs(up[-1] - c[-1]) <= 1e-15 and abs(up[-2] - (c[-2] + 7 * c[-1]) / 8) <= 1e-15
    assert abs(up[0] - (6 * c[0] + 2 * c[1]) / 8) <= 1e-15
    dn = R.pyr_down(np.outer(x, np.ones(2 * n)))[:, 0]
    assert dn.shape == (n,) and np.abs(dn - R.down_1d_closed(x)).max() <= 1e-15 * 8
    # and along the other axis
    assert np.abs(R.pyr_up(np.outer(np.ones(n), c))[0] - R.up_1d_closed(c)).max() <= 1e-14
    assert np.abs(R.pyr_down(np.outer(np.ones(2 * n), x))[0] - R.down_1d_closed(x)).max() <= 1e-14


def test_quantize_is_ties_to_even():
    x = (np.array([0.5, 1.5, 2.5, 254.5, -3.0, 300.0]) - 127.5) / 127.5
    assert R.quantize(x).tolist() == [0.0, 2.0, 2.0, 254.0, 0.0, 255.0]


# ------------------------------------------------------------------ SlicedWasserstein
KW = dict(per_image=16, dirs=8, repeats=2, seed=3)


def test_matches_reference_end_to_end():
    real, fake = images(8, 32, 1), images(8, 32, 2, "smooth")
    m, got = run(SwdCpuOps(), real, fake, **KW)
    ref, bound = reference_of(m, real, fake), swd_bound(m, real, fake)
    assert list(got) == [32, 16, "avg"] and all(isinstance(v, float) for v in got.values())
    for k in (32, 16):
        print(k, got[k], ref[k], bound[k])
        assert ref[k] > 10 * bound[k], "the two sets must differ by far more than the bound"
        assert abs(got[k] - ref[k]) <= bound[k], (k, got[k], ref[k], bound[k])
    assert abs(got["avg"] - ref["avg"]) <= max(bound.values())
    assert m.result() == got, "result() twice"


def test_batch_split_and_seed():
    real, fake = images(4, 32, 5), images(4, 32, 6, "smooth")
    _, whole = run(SwdCpuOps(), real, fake, **KW)
    _, parts = run(SwdCpuOps(), real, fake, split=[1, 3], **KW)
    assert whole == parts, "a 1 + 3 split equals one batch of 4"
    assert run(SwdCpuOps(), real, fake, **KW)[1] == whole, "same seed, same feeds"
    other = run(SwdCpuOps(), real, fake, **dict(KW, seed=4))[1]
    assert other != whole and abs(other[32] - whole[32]) < 0.5 * whole[32]
    # positions are keyed by (seed, level, image index), not by the call that drew them
    a = metrics.draw_positions(3, 1, 0, 4, 16, 16)
    b = torch.cat([metrics.draw_positions(3, 1, i, 1, 16, 16) for i in range(4)])
    assert torch.equal(a, b) and int(a.min()) >= 3 and int(a.max()) <= 12
    assert not torch.equal(a, metrics.draw_positions(3, 0, 0, 4, 16, 16))
    assert not torch.equal(a[:16], a[16:32])
    d = metrics.draw_directions(3, 2, 8)
    assert d.shape == (2, 147, 8) and d.dtype == torch.float32
    assert float((d.double().square().sum(1) - 1).abs().max()) < 1e-6


def test_identical_sets_give_zero():
    x = images(4, 32, 7)
    assert run(SwdCpuOps(), x, x.clone(), split=[3, 1], **KW)[1] == {32: 0.0, 16: 0.0, "avg": 0.0}


def test_argument_errors(monkeypatch):
    ops = SwdCpuOps()
    for bad in (8, 48):
        with pytest.raises(ValueError, match="resolution"):
            SlicedWasserstein(ops, bad, 4)
    m = SlicedWasserstein(ops, 16, 4, **KW)
    with pytest.raises(ValueError, match="expected"):
        m.feed("real", torch.zeros(2, 3, 32, 32))
    with pytest.raises(ValueError, match="which"):
        m.feed("both", torch.zeros(2, 3, 16, 16))
    with pytest.raises(RuntimeError, match="0 of 4"):
        m.result()
    m.feed("real", images(3, 16, 1))
    with pytest.raises(ValueError, match="exceed"):
        m.feed("real", images(2, 16, 2))
    m.feed("real", images(1, 16, 2))
    with pytest.raises(RuntimeError, match="fake"):
        m.result()
    m.feed("fake", images(3, 16, 3))
    monkeypatch.setattr(metrics, "draw_positions",
                        lambda *a: torch.tensor([[3, 13]] * 16, dtype=torch.int32))
    with pytest.raises(ValueError, match="centres"):
        m.feed("fake", images(1, 16, 4))
    monkeypatch.undo()
    m.feed("fake", images(1, 16, 4))
    assert set(m.result()) == {16, "avg"}


def test_entry_points_reject_bad_arguments():
    """The five entry points refuse null pointers and bad shapes on the host, before any
    launch (the pointers here are never dereferenced), naming themselves in the message."""
    import ctypes
    from pggan_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libpggan_hip.so not built")
    lib = _lib.load_library()
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    calls = {
        "swd_pyr_down": [lambda: lib.pg_swd_pyr_down(1, 32, 32, None, 1, p, None),
                         lambda: lib.pg_swd_pyr_down(1, 16, 16, p, 1, p, None),
                         lambda: lib.pg_swd_pyr_down(1, 48, 48, p, 1, p, None),
                         lambda: lib.pg_swd_pyr_down(1, 64, 32, p, 1, p, None),
                         lambda: lib.pg_swd_pyr_down(0, 32, 32, p, 1, p, None)],
        "swd_descriptors": [lambda: lib.pg_swd_descriptors(1, 16, p, None, 4, None, 0, p, None),
                            lambda: lib.pg_swd_descriptors(1, 8, p, None, 4, p, 0, p, None),
                            lambda: lib.pg_swd_descriptors(1, 16, p, None, 0, p, 0, p, None)],
        "swd_stats": [lambda: lib.pg_swd_stats(4, p, p, p, None, None),
                      lambda: lib.pg_swd_stats(0, p, p, p, p, None)],
        "swd_project": [lambda: lib.pg_swd_project(4, p, p, p, 2, None, p, 4, None),
                        lambda: lib.pg_swd_project(4, p, p, p, 2, p, p, 3, None),
                        lambda: lib.pg_swd_project(4, p, p, p, 0, p, p, 4, None)],
        "swd_l1": [lambda: lib.pg_swd_l1(2, 4, p, p, 4, None, p, None),
                   lambda: lib.pg_swd_l1(2, 4, p, p, 3, p, p, None),
                   lambda: lib.pg_swd_l1(70000, 4, p, p, 4, p, p, None)],
    }
    for name, fns in calls.items():
        for i, fn in enumerate(fns):
            assert fn() == -1, (name, i)
            assert name.encode() in lib.pg_last_error(), (name, i, lib.pg_last_error())


# ------------------------------------------------------------------ ProgressiveGAN.validation
@pytest.fixture
def cpu_model(monkeypatch):
    monkeypatch.setattr(ProgressiveGAN, "ops_factory", staticmethod(SwdCpuOps))
    monkeypatch.setattr(nets, "OPS_FACTORY", SwdCpuOps)
    nets._ENGINES.clear()

    def make(tmp_path, stage, **over):
        torch.manual_seed(11)
        m = fresh_model(make_args(tmp_path, swd_images=8, **over))
        m.set_validation()
        for _ in range(stage):
            m.change_scale(0)
        m.G.alpha = m.D.alpha = 0.5
        return m
    return make


def snapshot(m):
    return dict(rng_step=m._rng_step, rng=torch.get_rng_state().clone(), pos=m._pos,
                flat=[fp.flat.clone() for fp in (m.fpG, m.fpD)],
                mom=[t.clone() for fp in (m.fpG, m.fpD) for t in (fp.m, fp.v)])


def assert_unchanged(m, s):
    assert m._rng_step == s["rng_step"] and m._pos == s["pos"]
    assert torch.equal(torch.get_rng_state(), s["rng"])
    for a, b in zip(s["flat"], (m.fpG.flat, m.fpD.flat)):
        assert torch.equal(a, b)
    for a, b in zip(s["mom"], [t for fp in (m.fpG, m.fpD) for t in (fp.m, fp.v)]):
        assert torch.equal(a, b)


@pytest.mark.parametrize("ema", [None, 0.5])
def test_validation_on_the_cpu_double(tmp_path, cpu_model, ema):
    m = cpu_model(tmp_path, 1, use_validation=True, ema_decay=ema)
    assert m.valid_cycle == m.args.ckpt_cycle
    m.train_step()
    assert m.validation(0) is None, "8x8: undefined"
    m.change_scale(0)
    m.G.alpha = m.D.alpha = 0.5
    m.train_step()
    before = snapshot(m)
    out = m.validation(7)
    assert_unchanged(m, before)
    assert set(out) == {16, "avg"} and out[16] == out["avg"] and np.isfinite(out[16]) and out[16] > 0
    assert m.validation(8) == out, "private generators: the same answer again"
    rows = open(os.path.join(str(tmp_path), "t", "swd.csv")).read().splitlines()
    assert [r.split(",")[:2] for r in rows] == [["7", "2"], ["8", "2"]]
    assert [float(v) for v in rows[0].split(",")[2:]] == [out[16], out["avg"]]
    # training goes on exactly as without the validation
    twin = cpu_model(tmp_path, 1, ema_decay=ema)
    twin.train_step()
    twin.change_scale(0)
    twin.G.alpha = twin.D.alpha = 0.5
    twin.train_step()
    for mm in (m, twin):
        mm.train_step()
    m.train_step()
    twin.validation(0)
    twin.train_step()
    assert torch.equal(m.fpG.flat, twin.fpG.flat) and torch.equal(m.fpD.flat, twin.fpD.flat)


def test_validation_off_is_a_no_op(tmp_path, cpu_model):
    m = cpu_model(tmp_path, 2)
    assert m.args.use_validation is False
    before = snapshot(m)
    assert m.validation(0) is None and m.validation() is None
    assert_unchanged(m, before)
    assert not os.path.exists(os.path.join(str(tmp_path), "t", "swd.csv"))
    never_set = fresh_model(make_args(tmp_path))          # set_validation never called
    assert never_set.validation(0) is None


def test_held_out_split(tmp_path, cpu_model):
    from PIL import Image
    from pggan_amd.data import image_paths
    root = tmp_path / "imgs"
    root.mkdir()
    g = np.random.default_rng(0)
    for i in range(10):
        Image.fromarray(g.integers(0, 256, (20, 20, 3), dtype=np.uint8)).save(root / f"{i:02d}.png")
    m = cpu_model(tmp_path, 2, use_validation=True, synthetic_data=False,
                  dataset_root_list=[str(root)], valid_cycle=5, swd_seed=2)
    assert m.valid_cycle == 5
    paths = image_paths([str(root)])
    perm = np.random.default_rng(0).permutation(10)
    assert m.train_dataset.paths == [paths[i] for i in perm[:7]], "the training list as before"
    assert len(m.valid_paths) == 3 and not set(m.valid_paths) & set(m.train_dataset.paths)
    assert sorted(m.valid_paths + m.train_dataset.paths) == sorted(paths)
    # the 3 held-out images, decoded at 16x16 and wrapped around to 8 reals
    reals = torch.cat(list(m._validation.reals(16, 8, 4)))
    assert reals.shape == (8, 3, 16, 16) and torch.equal(reals[0], reals[3])
    u8 = torch.round(reals * 127.5 + 127.5)
    assert float((u8 - (reals * 127.5 + 127.5)).abs().max()) < 1e-4 and 0 <= u8.min() and u8.max() <= 255
    out = m.validation(1)
    assert set(out) == {16, "avg"} and out[16] > 0
    # valid_dataset_root takes precedence
    m.args.valid_dataset_root = str(root)
    assert len(torch.cat(list(m._validation.reals(16, 10, 4))).unique(dim=0)) == 10
