"""Training health (pggan_amd.health, config `health_cycle`) on the CPU test double
(tests/cpu_ops_health.py): the segment table built from FlatParams, the config checks, that
nothing runs when the key is blank, the tag-to-step arithmetic (also with a generator update
that is one behind), health.csv, the checkpoint guard, and the double itself against the
numpy reference (tests/health_ref.py)."""
import os

import numpy as np
import pytest
import torch

import health_ref as R
from cpu_ops_health import CHUNK, CpuOpsHealth, RecordingHealthOps
from gen_inputs import TINY_DEPTHS
from pggan_amd import engine as E
from pggan_amd import health as H
from pggan_amd import nets
from pggan_amd.model import ProgressiveGAN
from test_model_api import fresh_model, make_args

HEALTH_OPS = ("tensor_stats", "nonfinite_watch", "adam_pair")


@pytest.fixture(autouse=True)
def _cpu_ops(monkeypatch):
    monkeypatch.setattr(ProgressiveGAN, "ops_factory", staticmethod(CpuOpsHealth))
    monkeypatch.setattr(nets, "OPS_FACTORY", CpuOpsHealth)
    nets._ENGINES.clear()


def model(tmp_path, **over):
    m = fresh_model(make_args(tmp_path, isMaster=True, **over))
    m.change_scale(0)
    m.G.alpha = m.D.alpha = 0.5
    return m


# ---------------------------------------------------------------------- the segment table
@pytest.mark.parametrize("s", [0, 2, 3])
def test_segment_table_from_flat_params(s):
    for which, shapes in (("G", E.g_param_shapes(TINY_DEPTHS, s)), ("D", E.d_param_shapes(TINY_DEPTHS, s))):
        dead = E.dead_params(which, s)
        fp = E.FlatParams(shapes, dead, "cpu")
        names, offs, counts = H.segment_table(fp)
        assert len(dead) == 2 * max(0, s - 1) and not set(names) & dead
        assert sorted(names) == sorted(n for n, _ in shapes if n not in dead)
        shp = dict(shapes)
        assert counts == [int(np.prod(shp[n])) for n in names], "true element counts"
        assert offs == [fp.offsets[n] for n in names]
        assert all(o % 16 == 0 for o in offs) and offs == sorted(offs), "flat order, 64-byte starts"
        assert any(c % 16 for c in counts), "some tensor has padding behind it"
        spans = [fp.spans[n][1] - fp.spans[n][0] for n in names]
        assert counts != spans and all(c <= sp for c, sp in zip(counts, spans))
        assert offs[-1] + counts[-1] <= fp.n_live <= fp.numel
        net = H._Net(which, fp, "cpu")
        assert net.table.dtype == torch.int64 and net.table.tolist() == [list(x) for x in zip(offs, counts)]


# ---------------------------------------------------------------------- settings
@pytest.mark.parametrize("key,value", [("health_cycle", 0), ("health_cycle", -3), ("health_cycle", "often"),
                                       ("health_cycle", 2.5), ("health_cycle", True),
                                       ("health_on_bad", "ignore"), ("health_on_bad", 1)])
def test_settings_are_checked_once(tmp_path, key, value):
    over = {"health_cycle": 5, key: value}
    with pytest.raises(ValueError, match=key):
        ProgressiveGAN(make_args(tmp_path, **over), "cpu")


def test_settings_defaults(tmp_path):
    s = ProgressiveGAN(make_args(tmp_path, health_cycle=7), "cpu")._health.settings
    assert (s.cycle, s.on_bad) == (7, "stop")
    s = ProgressiveGAN(make_args(tmp_path, health_cycle="3", health_on_bad="warn"), "cpu")._health.settings
    assert (s.cycle, s.on_bad) == (3, "warn")
    # health_on_bad alone configures nothing
    assert ProgressiveGAN(make_args(tmp_path, health_on_bad="warn"), "cpu")._health.settings is None


def test_off_launches_nothing(tmp_path, monkeypatch):
    monkeypatch.setattr(ProgressiveGAN, "ops_factory", staticmethod(RecordingHealthOps))
    RecordingHealthOps.calls.clear()
    m = model(tmp_path)
    assert m._health.settings is None
    for step in range(2):
        m.train_step()
        assert m.health(step) is None
    assert m.save_checkpoint(1) is None          # as before: no guard, no result
    assert os.path.exists(f"{tmp_path}/t/ckpt/G_latest.pt")
    assert "adam" in RecordingHealthOps.calls
    assert not set(RecordingHealthOps.calls) & set(HEALTH_OPS)
    assert not os.path.exists(f"{tmp_path}/t/health.csv")
    # and on: the probe every step, the statistics on the cycle
    RecordingHealthOps.calls.clear()
    m = model(tmp_path, health_cycle=2)
    m.train_step()
    m.health(1)
    assert RecordingHealthOps.calls.count("nonfinite_watch") == 3        # m of G, m of D, loss
    assert "tensor_stats" not in RecordingHealthOps.calls
    m.health(2)
    assert RecordingHealthOps.calls.count("tensor_stats") == 2


# ---------------------------------------------------------------------- tags and steps
def test_tag_to_step_arithmetic():
    class FP:
        step = 0
    fp = FP()
    net = H._Net.__new__(H._Net)
    net.fp, net.seen = fp, {}
    # in step: update k is applied during global step k - 1 and first seen by that step's call
    for step in range(5):
        fp.step = step + 1
        net.see(step)
    assert [net.step_of(t, 4) for t in (1, 3, 5)] == [0, 2, 4]
    # the same answer from the counts alone (nothing seen, e.g. after a report)
    net.seen = {}
    assert [net.step_of(t, 4) for t in (1, 3, 5)] == [0, 2, 4]
    # one behind: the call of step s sees count s; update k is first seen at step k
    net.seen = {}
    for step in range(1, 6):
        fp.step = step
        net.see(step)
    assert [net.step_of(t, 5) for t in (1, 3, 5)] == [1, 3, 5]
    net.seen = {}
    assert [net.step_of(t, 5) for t in (1, 3, 5)] == [1, 3, 5]
    # calls without a train step between them do not move a count's step
    net.see(6)
    net.see(7)
    assert net.step_of(5, 7) == 6


class _Handle:
    def wait(self):
        pass


@pytest.mark.parametrize("deferred", [False, True])
def test_first_bad_step_in_a_run(tmp_path, deferred):
    """A NaN written into one element of a D tensor's first moment after step 5; the report
    of step 8 (health_cycle 4, warn) names that tensor with step 5.  The NaN reaches D's
    parameter in step 6's Adam_D, all of G's gradients in the same step and the rest of D in
    step 7: G's moments are first seen bad at step 6, or at step 7 when the generator update
    is deferred (a gradient hook that returns an object with .wait()) and so one behind."""
    m = model(tmp_path, health_cycle=4, health_on_bad="warn")
    if deferred:
        m._grad_hook = lambda net, g: _Handle()
    name = "decision_layer.module.weight"
    for step in range(9):
        m.train_step()
        assert m.fpD.step == step + 1 and m.fpG.step == (step if deferred else step + 1)
        if step == 5:
            m.fpD._view(m.fpD.m, name).view(-1)[0] = float("nan")
        out = m.health(step)
        assert out["report"] == (step % 4 == 0)
        if step < 8:
            assert not out.get("findings")
    first = {(f["net"], f["name"], f["buffer"]): f["step"] for f in out["findings"]}
    f0 = out["findings"][0]
    assert (f0["net"], f0["name"], f0["buffer"], f0["step"]) == ("D", name, "m", 5)
    g_steps = {v for (net, _, buf), v in first.items() if net == "G" and buf == "m"}
    assert g_steps == {7 if deferred else 6}
    d_steps = {v for (net, n, buf), v in first.items() if net == "D" and buf == "m" and n != name}
    assert d_steps == {7}
    assert first[("loss", "loss", "loss")] == 6
    rows = {(r["net"], r["name"]): r for r in out["rows"]}
    assert rows[("D", name)]["first_bad_step"] == 5 and rows[("D", name)]["bad"] >= 1
    assert m.fpG.step == 9, "the report flushed the deferred update"


def test_stop_raises_with_the_fields(tmp_path):
    m = model(tmp_path, health_cycle=1)
    m.train_step()
    assert m.health(0)["findings"] == []
    m.train_step()
    name = "first_block.block.0.module.bias"
    m.fpG._view(m.fpG.m, name).view(-1)[-1] = float("inf")
    with pytest.raises(H.TrainingDiverged, match=name) as e:
        m.health(1)
    assert (e.value.net, e.value.name, e.value.buffer, e.value.step) == ("G", name, "m", 1)
    assert "G" in str(e.value) and "buffer m" in str(e.value) and "step 1" in str(e.value)
    # a new stage starts with clean latches
    m.fpG.m.zero_()
    m.change_scale(1)
    m.train_step()
    assert m.health(2)["findings"] == []


# ---------------------------------------------------------------------- files
def test_csv_header_and_rows(tmp_path, capsys):
    m = model(tmp_path, health_cycle=2)
    for step in range(3):
        m.train_step()
        out = m.health(step)
    lines = open(f"{tmp_path}/t/health.csv").read().splitlines()
    assert lines[0] == H.CSV_HEADER == \
        "step,scale,net,name,numel,rms_p,rms_g,rms_u,ratio,max_p,max_g,bad,first_bad_step"
    names = [("G", n) for n in H.segment_table(m.fpG)[0]] + [("D", n) for n in H.segment_table(m.fpD)[0]]
    assert len(lines) == 1 + 2 * len(names), "one header, two reports (steps 0 and 2)"
    last = [l.split(",") for l in lines[1 + len(names):]]
    assert [(f[2], f[3]) for f in last] == names
    for f, r in zip(last, out["rows"]):
        assert (int(f[0]), int(f[1]), int(f[4])) == (2, m.scale_index, r["numel"])
        for k, key in zip(range(5, 11), ("rms_p", "rms_g", "rms_u", "ratio", "max_p", "max_g")):
            assert float(f[k]) == r[key], "floats are written with repr: they read back exactly"
        assert (int(f[11]), int(f[12])) == (0, -1)
    # the rows against the model's own views
    for r in out["rows"]:
        fp = m.fpG if r["net"] == "G" else m.fpD
        p, g = fp.views[r["name"]].double(), fp.gviews[r["name"]].double()
        assert r["rms_p"] == pytest.approx(float(p.square().mean().sqrt()), rel=1e-12)
        assert r["rms_g"] == pytest.approx(float(g.square().mean().sqrt()), rel=1e-12)
        assert r["max_p"] == float(p.abs().max()) and r["max_g"] == float(g.abs().max())
        assert r["ratio"] == (r["rms_u"] / r["rms_p"] if r["rms_p"] else 0.0)
    text = capsys.readouterr().out
    assert text.count("health grad rms G") == 2 and out["worst"][1] in text


# ---------------------------------------------------------------------- checkpoints
@pytest.mark.parametrize("buffer", ["flat", "m", "v", "ema"])
def test_checkpoint_guard(tmp_path, buffer, capsys):
    m = model(tmp_path, health_cycle=1000, ema_decay=0.5)
    for _ in range(2):
        m.train_step()
    assert m.save_checkpoint(1) is True
    paths = [f"{tmp_path}/t/ckpt/{n}_latest.pt" for n in ("G", "D", "G_ema")]
    before = [open(p, "rb").read() for p in paths]
    name = "latent_format_layer.module.weight"
    m.fpG._view(getattr(m.fpG, buffer), name).view(-1)[3] = float("nan")
    assert m.save_checkpoint(2) is False
    assert [open(p, "rb").read() for p in paths] == before
    assert not os.path.exists(f"{tmp_path}/t/ckpt/G_2.pt")
    said = capsys.readouterr().out
    assert "NOT written" in said and name in said
    assert f"buffer {'p' if buffer == 'flat' else buffer}" in said


# ---------------------------------------------------------------------- the double itself
def test_cpu_double_matches_the_reference():
    ops = CpuOpsHealth()
    table, n, fill = R.segment_case(CHUNK)
    p, g, m, v = fill(), fill(), fill(), fill(positive=True)
    for x, where in ((p, 0), (g, 16 + 2), (m, table[9][0] + CHUNK - 1), (v, table[11][0])):
        x[where] = np.inf
    pair = ops.adam_pair(1e-2, 0.5, 0.99, 3)
    want = R.tensor_stats(table, p, g, m, v, *pair, 1e-8)
    out = torch.zeros(len(table), 10, dtype=torch.float64)
    t = torch.from_numpy(table)
    ops.tensor_stats(t, *(torch.from_numpy(x) for x in (p, g, m, v)), step_size=pair[0],
                     bc2_sqrt=pair[1], eps=1e-8, out=out)
    got = out.numpy()
    assert np.array_equal(got[:, 3:], want[:, 3:]), "maxima and counts are exact"
    assert want[:, 6:].sum() == 4 and np.isfinite(got).all()
    np.testing.assert_allclose(got[:, :3], want[:, :3], rtol=1e-12)
    latch = torch.zeros(len(table), dtype=torch.int32)
    ops.nonfinite_watch(t, torch.from_numpy(m), 5, latch)
    assert latch.tolist() == R.nonfinite_watch(table, m, 5, np.zeros(len(table))).tolist()
    assert latch.tolist() == [0] * 9 + [5, 0, 0]
