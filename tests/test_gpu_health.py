"""Training health on the GPU: pg_tensor_stats and pg_nonfinite_watch against the float64
reference (tests/health_ref.py), and ProgressiveGAN.health / save_checkpoint on a tiny model.

Bounds of the op tests.  Counts and maxima are exact.  sumsq_p, sumsq_g: 1e-9 relative -- the
squares are exact in double, at most 2^22 non-negative terms, each double add at most 2^-53
relative: < 5e-10.  sumsq_u: 4 x the worst relative error measured on an MI355X against the
reference, under a cap of 1e-7 (the margin is for a device double sqrt / divide that rounds
differently from numpy's).  Measured: 2.423e-16 (the segment-size case; sumsq_p 2.080e-16,
sumsq_g 2.201e-16 at worst), so the bound is 9.7e-16; the maxima of u came out bit for bit equal
to numpy's on that run -- the device's double sqrt and divide rounded as numpy's -- and the test
holds them to that."""
import ctypes
import os

import numpy as np
import pytest
import torch

import health_ref as R
from gen_inputs import TINY_DEPTHS
from test_gpu_graph import build
from test_model_api import make_args

pytestmark = pytest.mark.gpu

# worst relative error of sumsq_u over every case of this file, measured on an MI355X
U_MEASURED = 2.423e-16
U_BOUND = min(4 * U_MEASURED, 1e-7)
SQ_BOUND = 1e-9
PAIR = (np.float32(1e-2 / (1 - 0.5 ** 3)), np.float32(np.sqrt(1 - 0.99 ** 3)))   # some update 3
EPS = 1e-8


@pytest.fixture(scope="module")
def ops():
    from pggan_amd import _lib
    return _lib.HipOps(torch.float32)


def run_stats(ops, table, bufs, pair=PAIR, eps=EPS):
    t = torch.from_numpy(np.ascontiguousarray(table)).cuda()
    dev = [None if x is None else torch.from_numpy(x).cuda() for x in bufs]
    out = torch.full((len(table), 10), -1.0, dtype=torch.float64, device="cuda")
    ops.tensor_stats(t, *dev, step_size=float(pair[0]), bc2_sqrt=float(pair[1]), eps=eps, out=out)
    again = torch.full_like(out, -2.0)
    ops.tensor_stats(t, *dev, step_size=float(pair[0]), bc2_sqrt=float(pair[1]), eps=eps, out=again)
    torch.cuda.synchronize()
    assert torch.equal(out, again), "two calls give bitwise equal statistics"
    return out.cpu().numpy()


def check(got, want, what):
    """Counts and maxima exact, the sums within their bounds; prints the worst errors."""
    rel = np.abs(got[:, :3] - want[:, :3]) / np.maximum(want[:, :3], 1e-300)
    print(f"{what}: worst relative error sumsq_p {rel[:, 0].max():.3e} sumsq_g {rel[:, 1].max():.3e} "
          f"sumsq_u {rel[:, 2].max():.3e}; maxabs_u equal: {np.array_equal(got[:, 5], want[:, 5])}")
    assert np.array_equal(got[:, 6:], want[:, 6:]), (what, "counts", got[:, 6:], want[:, 6:])
    assert np.array_equal(got[:, 3:6], want[:, 3:6]), (what, "maxima", got[:, 3:6], want[:, 3:6])
    assert np.isfinite(got).all(), what
    assert rel[:, 0].max() <= SQ_BOUND and rel[:, 1].max() <= SQ_BOUND, (what, rel[:, :2].max(0))
    assert rel[:, 2].max() <= U_BOUND, (what, rel[:, 2].max())


def layouts(C):
    """name -> (table, n, fill): the segment-size case, one segment of 3 floats, 300 segments
    of 3 floats (more segments than a workgroup has threads), and one tensor longer than
    256 ranges (the finishing pass gives each of its threads more than one partial)."""
    return {"sizes": R.segment_case(C, seed=1), "one": R.layout([3], seed=2),
            "many": R.layout([3] * 300, seed=3), "long": R.layout([5, 300 * C + 7, 33], seed=4)}


@pytest.fixture(scope="module")
def cases(ops):
    """Per layout: the table, the four buffers (N(0, 1) scaled per segment from 1e-30 to 1e25,
    v non-negative, every padding float NaN) and the reference, drawn and computed once."""
    out = {}
    for name, (table, n, fill) in layouts(ops.tensor_stats_chunk).items():
        bufs = [fill(), fill(), fill(), fill(positive=True)]
        out[name] = (table, n, bufs, R.tensor_stats(table, *bufs, *PAIR, EPS))
    return out


# ---------------------------------------------------------------------- pg_tensor_stats
@pytest.mark.parametrize("name", ["sizes", "one", "many", "long"])
def test_stats_match_the_reference_and_never_read_padding(ops, cases, name):
    table, n, bufs, want = cases[name]
    assert all(np.isnan(x).sum() == n - table[:, 1].sum() for x in bufs), "all padding is NaN"
    assert ops.tensor_stats_chunk % 16 == 0
    got = run_stats(ops, table, bufs)
    assert not got[:, 6:].any(), "no padding float was counted"
    assert want[:, 0].min() < 1e-55 and want[:, 0].max() > 1e50 or name != "sizes", \
        "sums an fp32 accumulator cannot hold"
    check(got, want, name)


def test_stats_null_buffers_are_zero_columns(ops, cases):
    table, n, bufs, _ = cases["sizes"]
    p, g, m, v = bufs
    want = run_stats(ops, table, bufs)      # the same sums in the same order: bitwise
    got = run_stats(ops, table, [p, None, None, v])
    assert np.array_equal(got[:, [0, 3, 6, 9]], want[:, [0, 3, 6, 9]])
    assert not got[:, [1, 2, 4, 5, 7, 8]].any()
    got = run_stats(ops, table, [None, g, m, None])
    assert np.array_equal(got[:, [1, 4, 7, 8]], want[:, [1, 4, 7, 8]])
    assert not got[:, [0, 2, 3, 5, 6, 9]].any()


@pytest.mark.parametrize("which", [0, 1, 2, 3], ids=["p", "g", "m", "v"])
def test_stats_with_planted_non_finite_values(ops, cases, which):
    """+Inf, -Inf and NaN at the first and the last element of a segment and on both sides of a
    range boundary (absolute indices k C - 1, k C inside the longest segment), in one buffer."""
    table, n, bufs, _ = cases["sizes"]
    C = ops.tensor_stats_chunk
    bufs = [x.copy() for x in bufs]
    x = bufs[which]
    off, cnt = (int(t) for t in table[11])
    k = off // C + 1
    assert off < k * C - 1 and (k + 1) * C < off + cnt
    spots = {int(table[5][0]): np.inf, int(table[5][0] + table[5][1] - 1): -np.inf,
             int(table[2][0] + table[2][1] - 1): np.nan, off: np.nan, off + cnt - 1: np.inf,
             k * C - 1: -np.inf, k * C: np.nan, (k + 1) * C - 1: np.inf, (k + 1) * C: -np.inf}
    if which == 3:
        spots = {i: (np.inf if np.isinf(val) else val) for i, val in spots.items()}   # v >= 0
    for i, val in spots.items():
        x[i] = val
    want = R.tensor_stats(table, *bufs, *PAIR, EPS)
    assert want[:, 6 + which].tolist() == [0, 0, 1, 0, 0, 2, 0, 0, 0, 0, 0, 6]
    check(run_stats(ops, table, bufs), want, f"planted in {'pgmv'[which]}")


@pytest.mark.parametrize("t", [1, 50])
def test_update_is_what_adam_applies(ops, t):
    """sum((p_before - p_after)^2) of one pg_adam at update t agrees with sumsq_u of the moments
    it left, within 1 %: the cancellation in p (|p| <= 1, lr 1e-2) costs <= 2^-24 / 1e-2 ~ 6e-6
    per element, a wrong bias correction at t = 1 is off by ~10 x."""
    table, n, fill = R.layout([1000, 37, 4099], pad_value=0.0, seed=5)
    gen = torch.Generator(device="cuda").manual_seed(6)
    p = torch.rand(n, device="cuda", generator=gen) * 2 - 1
    g = torch.randn(n, device="cuda", generator=gen)
    m = torch.randn(n, device="cuda", generator=gen) * 0.1
    v = torch.randn(n, device="cuda", generator=gen).square() * 0.5
    kw = dict(lr=1e-2, beta1=0.5, beta2=0.99, eps=1e-8)
    before = p.clone()
    ops.adam(p, g, m, v, step=t, **kw)
    pair = ops.adam_pair(kw["lr"], kw["beta1"], kw["beta2"], t)
    assert pair == pytest.approx((1e-2 / (1 - 0.5 ** t), np.sqrt(1 - 0.99 ** t)), rel=1e-6)
    tab = torch.from_numpy(table).cuda()
    out = torch.zeros(3, 10, dtype=torch.float64, device="cuda")
    ops.tensor_stats(tab, p, g, m, v, step_size=pair[0], bc2_sqrt=pair[1], eps=kw["eps"], out=out)
    got = out.cpu().numpy()
    for s, (off, cnt) in enumerate(table):
        d = (before[off:off + cnt].double() - p[off:off + cnt].double()).square().sum().item()
        print(f"t {t} segment {s}: applied {d:.6e} sumsq_u {got[s, 2]:.6e}")
        assert abs(got[s, 2] - d) <= 0.01 * d, (t, s, got[s, 2], d)


def test_entry_points_reject_bad_arguments(ops):
    lib = ops.lib
    tab = torch.tensor([[0, 3]], dtype=torch.int64, device="cuda")
    x = torch.zeros(32, device="cuda")
    out = torch.zeros(1, 10, dtype=torch.float64, device="cuda")
    ws = torch.zeros(64, dtype=torch.float64, device="cuda")
    lat = torch.zeros(1, dtype=torch.int32, device="cuda")
    P = lambda t, byte=0: ctypes.c_void_p(t.data_ptr() + byte)
    need = lib.pg_tensor_stats_workspace_bytes(1, 16)
    assert need == (1 + 1) * 10 * 8 and lib.pg_tensor_stats_workspace_bytes(0, 16) == 0
    stats = lambda nseg=1, table=P(tab), p=P(x), o=P(out), w=P(ws), wb=need: lib.pg_tensor_stats(
        nseg, table, 16, p, None, None, None, 1.0, 1.0, 0.0, o, w, wb, None)
    watch = lambda nseg=1, table=P(tab), xx=P(x), tag=1, fb=P(lat): lib.pg_nonfinite_watch(
        nseg, table, xx, 16, tag, fb, None)
    for call in (lambda: stats(nseg=0), lambda: stats(table=None), lambda: stats(o=None),
                 lambda: stats(p=P(x, 4)), lambda: stats(wb=need - 8), lambda: stats(w=None)):
        assert call() == -1
        assert b"tensor_stats" in lib.pg_last_error()
    for call in (lambda: watch(nseg=0), lambda: watch(table=None), lambda: watch(fb=None),
                 lambda: watch(tag=0), lambda: watch(xx=P(x, 4))):
        assert call() == -1
        assert b"nonfinite_watch" in lib.pg_last_error()
    assert stats() == 0 and watch() == 0
    torch.cuda.synchronize()
    assert lat.item() == 0


# ---------------------------------------------------------------------- pg_nonfinite_watch
def test_watch_latches_the_first_tag(ops, cases):
    table, n, bufs, _ = cases["sizes"]
    tab = torch.from_numpy(table).cuda()
    x = torch.from_numpy(bufs[2]).cuda()            # every padding float is NaN
    lat = torch.zeros(len(table), dtype=torch.int32, device="cuda")
    ops.nonfinite_watch(tab, x, 4, lat)
    assert lat.tolist() == [0] * 12, "a clean buffer (NaN padding aside) latches nothing"
    k, j = 9, 2
    x[int(table[k][0] + table[k][1] - 1)] = float("nan")
    ops.nonfinite_watch(tab, x, 5, lat)
    assert lat.tolist() == [5 if s == k else 0 for s in range(12)]
    x[int(table[j][0])] = float("-inf")
    ops.nonfinite_watch(tab, x, 6, lat)
    assert lat.tolist() == [5 if s == k else 6 if s == j else 0 for s in range(12)]
    assert lat.tolist() == R.nonfinite_watch(table, x.cpu().numpy(), 6, [5 if s == k else 0 for s in range(12)]).tolist()


def test_watch_covers_every_element(ops):
    """300 segments of 3 floats, and a buffer longer than one sweep of the grid (2048 workgroups
    x 256 threads x 4 quads) whose length is no multiple of 4: a value in the second sweep and
    the very last element are seen."""
    table, n, fill = R.layout([3] * 300, seed=7)
    tab, x = torch.from_numpy(table).cuda(), torch.from_numpy(fill()).cuda()
    lat = torch.zeros(300, dtype=torch.int32, device="cuda")
    x[int(table[299][0]) + 2] = float("inf")
    x[int(table[150][0])] = float("nan")
    ops.nonfinite_watch(tab, x, 9, lat)
    assert [s for s in range(300) if lat[s].item()] == [150, 299] and lat[150].item() == 9
    sweep = 2048 * 256 * 4 * 4
    n = sweep + 4 * 1000 + 3
    tab = torch.tensor([[0, sweep], [sweep, 4 * 1000 - 16], [sweep + 4 * 1000 - 16, 19]],
                       dtype=torch.int64, device="cuda")
    x = torch.ones(n, device="cuda")
    lat = torch.zeros(3, dtype=torch.int32, device="cuda")
    ops.nonfinite_watch(tab, x, 1, lat)
    assert lat.tolist() == [0, 0, 0]
    x[n - 1] = float("nan")
    ops.nonfinite_watch(tab, x, 2, lat)
    assert lat.tolist() == [0, 0, 2]
    x[sweep + 5] = float("inf")
    ops.nonfinite_watch(tab, x, 3, lat)
    assert lat.tolist() == [0, 3, 2]


# ---------------------------------------------------------------------- the model
def model(tmp_path, replay=False, **over):
    args = make_args(tmp_path, depths=list(TINY_DEPTHS), isMaster=True, **over)
    m = build(args, False, 2)
    m.use_replay = replay
    m.G.alpha = m.D.alpha = 0.5
    return m


def test_report_matches_the_models_views(tmp_path):
    from pggan_amd import health as H
    m = model(tmp_path, health_cycle=1)
    for step in range(3):
        m.train_step()
        out = m.health(step)
    torch.cuda.synchronize()
    assert out["report"] and out["findings"] == [] and len(out["rows"]) > 20
    assert [r["name"] for r in out["rows"] if r["net"] == "G"] == H.segment_table(m.fpG)[0]
    assert not any("toRGB_blocks.0." in r["name"] or "fromRGB_blocks.0." in r["name"] for r in out["rows"])
    for r in out["rows"]:
        fp, lr = (m.fpG, m.opt_G.lr) if r["net"] == "G" else (m.fpD, m.opt_D.lr)
        n = r["numel"]
        p, g = (v[r["name"]].double().cpu().numpy().ravel() for v in (fp.views, fp.gviews))
        mm, vv = (fp._view(b, r["name"]).cpu().numpy().ravel() for b in (fp.m, fp.v))
        pair = m._health.ops.adam_pair(lr, m.hyper.beta1, m.hyper.beta2, fp.step)
        u = R.update(mm, vv, *pair, m.hyper.eps)
        assert fp.step == 3 and n == p.size
        for key, x in (("rms_p", p), ("rms_g", g), ("rms_u", u)):
            assert r[key] ** 2 * n == pytest.approx(float((x * x).sum()), rel=1e-9), (r["name"], key)
        assert r["max_p"] == np.abs(p).max() and r["max_g"] == np.abs(g).max()
        assert (r["bad"], r["first_bad_step"]) == (0, -1)
    lines = open(f"{tmp_path}/t/health.csv").read().splitlines()
    assert lines[0] == H.CSV_HEADER and len(lines) == 1 + 3 * len(out["rows"])
    for line, r in zip(lines[-len(out["rows"]):], out["rows"]):
        f = line.split(",")
        assert (int(f[0]), int(f[1]), f[2], f[3], int(f[4])) == (2, 2, r["net"], r["name"], r["numel"])
        assert [float(t) for t in f[5:11]] == [r[k] for k in ("rms_p", "rms_g", "rms_u", "ratio", "max_p", "max_g")]
        assert (int(f[11]), int(f[12])) == (0, -1)


def test_health_leaves_training_bitwise_alone(tmp_path):
    off, on = model(tmp_path, replay=True), model(tmp_path, replay=True, health_cycle=2)
    for step in range(5):
        off.train_step()
        on.train_step()
        assert off.health(step) is None
        assert on.health(step)["report"] == (step % 2 == 0)
    torch.cuda.synchronize()
    for net in ("fpG", "fpD"):
        for buf in ("flat", "m", "v"):
            assert torch.equal(getattr(getattr(off, net), buf), getattr(getattr(on, net), buf)), (net, buf)
    assert off.graph_replays == on.graph_replays > 0


def test_guard(tmp_path, capsys):
    from pggan_amd import health as H
    m = model(tmp_path, health_cycle=1, health_on_bad="warn")
    for step in range(2):
        m.train_step()
    assert m.save_checkpoint(1) is True
    paths = [f"{tmp_path}/t/ckpt/{n}_latest.pt" for n in ("G", "D")]
    before = [open(p, "rb").read() for p in paths]
    name = "minibatch_normalization_block.linear.module.weight"
    m.fpD._view(m.fpD.m, name).view(-1)[7] = float("nan")
    capsys.readouterr()
    out = m.health(1)
    want = dict(net="D", name=name, buffer="m", count=1, step=1)
    assert out["findings"] == [want]
    said = capsys.readouterr().out
    assert "WARNING" in said and name in said and "buffer m" in said and "first bad step 1" in said
    again = m.health(2)                               # no train step between
    assert again["findings"] == [want]
    m.args.health_on_bad = "stop"
    m._health.configure()
    with pytest.raises(H.TrainingDiverged) as e:
        m.health(3)
    assert (e.value.net, e.value.name, e.value.buffer, e.value.step) == ("D", name, "m", 1)
    assert m.save_checkpoint(3) is False
    assert [open(p, "rb").read() for p in paths] == before
    assert not os.path.exists(f"{tmp_path}/t/ckpt/D_3.pt")
    assert "NOT written" in capsys.readouterr().out
