"""Checkpoint interoperability with the reference.

Everywhere, against a checkpoint the reference's own save_checkpoint wrote, stored under
tests/golden/ref_ckpt (tests/golden/make_golden.py ref_ckpt: one training step at stage 1,
narrow depths): pggan_amd's load_checkpoint restores exactly what the files hold, and what
pggan_amd's save_checkpoint then writes has the reference file's layout, entry for entry,
with the same values.

With the reference itself, only in the build container, where it is importable (SURVEY
§8(c) recipe, tests/golden/make_golden.import_reference); skipped elsewhere:

* reference -> pggan_amd: the reference's own ProgressiveGAN trains one step at stage 1
  and writes {save_root}/{run_id}/ckpt/{G,D}_{step,latest}.pt with its own
  save_checkpoint (pggan/model.py:50-67, lib/checkpoint.py:22-34); pggan_amd's
  load_checkpoint restores bit-identical parameters, Adam moments / step counts and the
  schedule scalars.
* pggan_amd -> reference: pggan_amd's save_checkpoint output is read back by the
  reference's own load_checkpoint (pggan/model.py:70-101) into a fresh reference model:
  bit-identical parameters and optimizer state.  (The reference hard-codes
  map_location='cuda' and .cuda() calls; on this CPU container they are redirected to
  the CPU for the duration of the call.)
"""
import os

import numpy as np
import pytest
import torch

from cpu_ops import CpuOps
from pggan_amd import nets
from pggan_amd.model import ProgressiveGAN
from test_model_api import make_args

REF = "/root/reference"
needs_reference = pytest.mark.skipif(
    not os.path.isdir(os.path.join(REF, "pggan")),
    reason="the reference is importable only in the build container")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(autouse=True)
def _cpu_ops(monkeypatch):
    monkeypatch.setattr(ProgressiveGAN, "ops_factory", staticmethod(CpuOps))
    monkeypatch.setattr(nets, "OPS_FACTORY", CpuOps)


def _stored(name):
    """One file of the reference-written checkpoint under tests/golden/ref_ckpt."""
    return torch.load(os.path.join(GOLDEN, "ref_ckpt", "ckpt", f"{name}_latest.pt"),
                      map_location="cpu", weights_only=True)


def _resume_from_stored(tmp_path):
    ref = {n: _stored(n) for n in "GD"}
    args = make_args(tmp_path, save_root=GOLDEN, ckpt_id="ref_ckpt", ckpt_step=None,
                     depths=list(ref["G"]["args"]["depths"]),
                     latent_dim=ref["G"]["args"]["latent_dim"])
    ma = ProgressiveGAN(args, "cpu")
    ma.initialize_models()
    ma.set_optimizers()
    ma.set_dataset()
    ma.set_data_iterator()
    ma.set_loss_collector()
    ma.load_checkpoint()
    return ma, ref


def _same_optimizer_state(a, b):
    assert set(a["state"]) == set(b["state"])
    for i in a["state"]:
        assert set(a["state"][i]) == set(b["state"][i]) == {"step", "exp_avg", "exp_avg_sq"}
        assert float(a["state"][i]["step"]) == float(b["state"][i]["step"]) == 1.0
        for k in ("exp_avg", "exp_avg_sq"):
            x, y = a["state"][i][k], b["state"][i][k]
            assert x.dtype == y.dtype and torch.equal(x, y), (i, k)
    assert len(a["param_groups"]) == len(b["param_groups"]) == 1
    ga, gb = a["param_groups"][0], b["param_groups"][0]
    assert ga["params"] == gb["params"] and set(a["state"]) <= set(ga["params"])
    for k in ("lr", "betas", "eps", "weight_decay", "amsgrad"):
        assert np.allclose(ga[k], gb[k], rtol=1e-12, atol=0), k


def test_stored_reference_checkpoint_resumes_exactly(tmp_path):
    ma, ref = _resume_from_stored(tmp_path)
    assert (ma.scale_index, ma.global_step, ma.alpha_index, ma.alpha_jump_value,
            ma.next_alpha_jump_step, ma.next_scale_jump_step) == (1, 7, 1, 0.5, 9, 12)
    assert ma.G.alpha == 0.5 and ma.D.alpha == 0.5
    for n, net, opt in (("G", ma.G, ma.opt_G), ("D", ma.D, ma.opt_D)):
        sd = net.state_dict()
        assert list(sd) == list(ref[n]["model"])
        for k, v in ref[n]["model"].items():
            assert torch.equal(sd[k].cpu(), v), (n, k)
        assert len(ref[n]["optimizer"]["state"]) > 0
        _same_optimizer_state(opt.state_dict(), ref[n]["optimizer"])


def test_saved_checkpoint_has_the_stored_reference_layout(tmp_path):
    ma, ref = _resume_from_stored(tmp_path)
    ma.args.save_root, ma.args.run_id = str(tmp_path), "ours"
    ma.save_checkpoint(11)
    assert sorted(os.listdir(tmp_path / "ours" / "ckpt")) == ["D_11.pt", "D_latest.pt", "G_11.pt",
                                                                "G_latest.pt"]
    for n in "GD":
        for f in (f"{n}_11.pt", f"{n}_latest.pt"):
            ours = torch.load(tmp_path / "ours" / "ckpt" / f, map_location="cpu", weights_only=True)
            assert list(ours) == list(ref[n])          # every entry the reference's loader reads
            for k in ("alpha_G", "alpha_D", "alpha_index", "alpha_jump_value",
                      "next_alpha_jump_step", "scale_index", "next_scale_jump_step"):
                assert type(ours[k]) is type(ref[n][k]) and ours[k] == ref[n][k], k
            assert ours["global_step"] == 11
            assert set(ref[n]["args"]) <= set(ours["args"])
            assert list(ours["model"]) == list(ref[n]["model"])
            for k, v in ref[n]["model"].items():
                w = ours["model"][k]
                assert w.dtype == v.dtype and w.shape == v.shape and torch.equal(w, v), (n, k)
            _same_optimizer_state(ours["optimizer"], ref[n]["optimizer"])


@needs_reference
def test_checkpoints_interoperate_with_the_reference(tmp_path, monkeypatch):
    from make_golden import import_reference, ref_model, run_ref_checkpoint
    R = import_reference()
    import lib.checkpoint as ref_ckpt
    # ---- reference trains one step at stage 1 and saves
    mr = run_ref_checkpoint(R, tmp_path, "ref")
    assert sorted(os.listdir(tmp_path / "ref" / "ckpt")) == ["D_7.pt", "D_latest.pt", "G_7.pt",
                                                               "G_latest.pt"]
    # ---- pggan_amd resumes from it
    args = make_args(tmp_path, ckpt_id="ref", ckpt_step=None)
    ma = ProgressiveGAN(args, "cpu")
    ma.initialize_models()
    ma.set_optimizers()
    ma.set_dataset()
    ma.set_data_iterator()
    ma.set_loss_collector()
    ma.load_checkpoint()
    assert (ma.scale_index, ma.global_step, ma.alpha_index, ma.alpha_jump_value,
            ma.next_alpha_jump_step, ma.next_scale_jump_step) == (1, 7, 1, 0.5, 9, 12)
    assert ma.G.alpha == 0.5 and ma.D.alpha == 0.5
    for a, b in ((mr.G, ma.G), (mr.D, ma.D)):
        sa, sb = a.state_dict(), b.state_dict()
        assert list(sa) == list(sb)
        for k in sa:
            assert torch.equal(sa[k], sb[k]), k
    for opt_r, opt_a in ((mr.opt_G, ma.opt_G), (mr.opt_D, ma.opt_D)):
        ra, aa = opt_r.state_dict()["state"], opt_a.state_dict()["state"]
        assert set(ra) == set(aa)
        for i in ra:
            assert float(ra[i]["step"]) == float(aa[i]["step"])
            for k in ("exp_avg", "exp_avg_sq"):
                assert torch.equal(ra[i][k], aa[i][k]), (i, k)
    # ---- pggan_amd saves, the reference's own load_checkpoint reads it back
    ma.args.run_id = "ours"
    ma.save_checkpoint(11)
    mb = ref_model(R, tmp_path, "reader", 0, ckpt_id="ours")
    mb.reset_solver = mb.set_optimizers          # its dataset half needs torchvision
    real_load = torch.load
    monkeypatch.setattr(ref_ckpt.torch, "load",
                        lambda p, map_location=None, **k: real_load(p, map_location="cpu", **k))
    mb.load_checkpoint()
    assert mb.scale_index == 1 and mb.global_step == 11
    for a, b in ((ma.G, mb.G), (ma.D, mb.D)):
        sa, sb = a.state_dict(), b.state_dict()
        assert list(sa) == list(sb)
        for k in sa:
            assert torch.equal(sa[k].cpu(), sb[k]), k
    for opt_a, opt_b in ((ma.opt_G, mb.opt_G), (ma.opt_D, mb.opt_D)):
        sa, sb = opt_a.state_dict()["state"], opt_b.state_dict()["state"]
        assert set(sa) == set(sb)
        for i in sa:
            for k in ("exp_avg", "exp_avg_sq"):
                assert torch.equal(sa[i][k].cpu(), sb[i][k]), (i, k)
    assert np.isclose(mb.opt_D.param_groups[0]["lr"], ma.opt_D.lr)
