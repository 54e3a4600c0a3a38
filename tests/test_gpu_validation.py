"""All the parts of ProgressiveGAN.validation in one run against each part alone, on the HIP
library (the CPU doubles' version is test_validation_cpu.py): SWD, MS-SSIM and the
nearest-neighbour search are bit-repeatable and latent recovery is a function of its inputs, so
the full run's dict and csv rows are exactly the union of the single-part runs'."""
import os

import pytest
import torch

from gen_inputs import TINY_DEPTHS
from test_gpu_graph import build
from test_gpu_recover import use_hip
from test_model_api import make_args
from test_validation_cpu import PARTS, TAIL, csvs

pytestmark = pytest.mark.gpu


def model(tmp_path, stage, **over):
    args = make_args(tmp_path, depths=list(TINY_DEPTHS), use_validation=True, swd_images=8,
                     valid_cycle=1, recover_steps=5, isMaster=True, **over)
    m = build(args, False, stage)
    m.set_validation()
    m.G.alpha = m.D.alpha = 0.5
    return m


@pytest.mark.parametrize("stage", [1, 2], ids=["8x8", "16x16"])
def test_all_parts_at_once_equal_each_part_alone(tmp_path, stage):
    use_hip()
    runs = {"full": {k: v for part in PARTS.values() for k, v in part.items()}, "none": {}, **PARTS}
    out, files = {}, {}
    for name, keys in runs.items():
        m = model(tmp_path / name, stage, **keys)
        m.train_step()
        m.flush()
        before = [t.clone() for fp in (m.fpG, m.fpD) for t in (fp.flat, fp.m, fp.v)]
        out[name] = m.validation(5)
        after = [t for fp in (m.fpG, m.fpD) for t in (fp.flat, fp.m, fp.v)]
        assert all(torch.equal(a, b) for a, b in zip(before, after)), name
        files[name] = csvs(os.path.join(str(tmp_path), name, "t"))
    singles = [n for n in runs if n != "full"]
    union = {}
    for n in singles:
        union.update(out[n] or {})
    print(f"stage {stage}: full {out['full']}\nunion {union}")
    assert out["full"] == union and list(out["full"]) == list(union)
    assert list(out["full"]) == ([16] + TAIL if stage == 2 else TAIL[3:])
    want = {}
    for n in singles:
        for f, data in files[n].items():
            assert files["full"].get(f) == data, (n, f)
            want[f] = data
    assert files["full"] == want
    assert sorted(want) == (["msssim.csv", "nn.csv", "recover.csv", "swd.csv"] if stage == 2
                            else ["nn.csv", "recover.csv"])
