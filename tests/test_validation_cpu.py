"""All the parts of ProgressiveGAN.validation in one run (SWD, MS-SSIM, nearest training
images, latent recovery) against each part alone, on the CPU test doubles: the parts read the
same stream of images and must not disturb each other, so the full run's dict, csv rows and
printed lines are exactly the union of the single-part runs'."""
import glob
import os

import pytest
import torch

import msssim_ref
import nn_ref
import swd_ref
from cpu_ops_recover import CpuOpsRecover
from pggan_amd import nets
from pggan_amd.model import ProgressiveGAN
from test_model_api import fresh_model, make_args
from test_swd_cpu import assert_unchanged, snapshot


class AllCpuOps(nn_ref.CpuNnOps, msssim_ref.CpuMsssimOps, swd_ref.CpuSwdOps, CpuOpsRecover):
    pass


PARTS = dict(ms=dict(msssim_pairs=2), nn=dict(nn_queries=5), rec=dict(recover_images=3))
TAIL = ["avg", "msssim", "msssim_real", "nn", "nn_real", "nn_min", "rec_train", "rec_real", "rec_fake"]


@pytest.fixture
def cpu_model(monkeypatch):
    torch.set_num_threads(4)
    monkeypatch.setattr(ProgressiveGAN, "ops_factory", staticmethod(AllCpuOps))
    monkeypatch.setattr(nets, "OPS_FACTORY", AllCpuOps)
    nets._ENGINES.clear()

    def make(tmp_path, stage, **over):
        torch.manual_seed(11)
        m = fresh_model(make_args(tmp_path, swd_images=8, use_validation=True, isMaster=True,
                                  recover_steps=3, **over))
        m.set_validation()
        for _ in range(stage):
            m.change_scale(0)
        m.G.alpha = m.D.alpha = 0.5
        return m
    yield make
    nets._ENGINES.clear()


def validate(m, capsys):
    """(dict, the run's `step 5:` lines) of one validation that leaves the model as it was."""
    capsys.readouterr()
    before = snapshot(m)
    out = m.validation(5)
    assert_unchanged(m, before)
    return out, [l for l in capsys.readouterr().out.splitlines() if l.startswith("step 5:")]


def csvs(d):
    return {os.path.basename(p): open(p, "rb").read() for p in glob.glob(os.path.join(d, "*.csv"))}


@pytest.mark.parametrize("stage", [0, 1, 2], ids=["4x4", "8x8", "16x16"])
def test_all_parts_at_once_equal_each_part_alone(tmp_path, cpu_model, capsys, stage):
    runs = {"full": {k: v for part in PARTS.values() for k, v in part.items()}, "none": {}, **PARTS}
    out, lines, files = {}, {}, {}
    for name, keys in runs.items():
        m = cpu_model(tmp_path / name, stage, **keys)
        out[name], lines[name] = validate(m, capsys)
        files[name] = csvs(os.path.join(str(tmp_path), name, "t"))
    singles = [n for n in runs if n != "full"]
    # the dict: the union of the single-part dicts, float for float, in the documented order
    union = {}
    for n in singles:
        union.update(out[n] or {})
    assert out["full"] == union and list(out["full"]) == list(union)
    sizes = [16] if stage == 2 else []
    have = sizes + [k for k in TAIL if k in out["full"]]
    assert list(out["full"]) == have
    assert set(have) == set(sizes + {0: TAIL[6:], 1: TAIL[3:], 2: TAIL}[stage])
    assert out["none"] is None if stage < 2 else list(out["none"]) == [16, "avg"]
    # the csv files: each byte for byte the one its part wrote alone
    want = {}
    for n in singles:
        for f, data in files[n].items():
            assert files["full"].get(f) == data, (n, f)
            want[f] = data
    assert files["full"] == want
    assert sorted(want) == {0: ["recover.csv"], 1: ["nn.csv", "recover.csv"],
                            2: ["msssim.csv", "nn.csv", "recover.csv", "swd.csv"]}[stage]
    # the printed lines: the single runs' lines, each once, in the order of the parts
    merged = []
    for n in singles:
        merged += [l for l in lines[n] if l not in merged]
    assert lines["full"] == merged and len(merged) == {0: 3, 1: 3, 2: 4}[stage]
    # the figures, wherever their part ran
    for n, fig, ran in (("full", "nn", stage >= 1), ("nn", "nn", stage >= 1),
                        ("full", "recover", True), ("rec", "recover", True)):
        assert os.path.exists(os.path.join(str(tmp_path), n, "t", fig, "e5.jpg")) == ran, (n, fig)
