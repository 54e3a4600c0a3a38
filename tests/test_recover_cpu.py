"""Latent recovery on the CPU double (tests/cpu_ops_recover.py): the generator's
input-gradient pass and its tail to the latent against the oracle's autograd, dL/dz through
the autograd modules, the training step's unchanged launch sequence, and that the loop
recovers latents.  The HIP kernels themselves are in test_gpu_recover.py, which reuses the
helpers here."""
import json
import os

import pytest
import torch

import kink_parity as K
import recover_ref as RR
from cpu_ops_recover import CpuOpsRecover, RecordingOps
from gen_inputs import TINY_DEPTHS, make_inputs, make_params
from golden_utils import GOLDEN
from oracle import pggan_oracle as O
from pggan_amd import engine as E
from pggan_amd import nets
from pggan_amd import recover as R

DZ_CASES = [(0, 1.0, 3), (1, 0.5, 3), (2, 0.5, 4), (2, 1.0, 4)]     # (s, alpha, B)


def g_params(s, seed=81, device="cpu"):
    sh = E.g_param_shapes(TINY_DEPTHS, s)
    return {k: torch.from_numpy(v).to(device) for k, v in make_params(sh, seed).items()}


def make_generator(s, alpha, device="cpu", dtype=torch.float32, seed=81):
    G = nets.Generator(512, TINY_DEPTHS[0]).to(device)
    for i in range(1, s + 1):
        G.add_block(TINY_DEPTHS[i])
    G.alpha = alpha
    G.compute_dtype = dtype
    G.load_state_dict(g_params(s, seed))
    return G


def dz_parity(ops, s, alpha, B, device="cpu", **engine_options):
    """Relative L2 of dL/dz from g_input_grad + the PixelNorm tail against the oracle's
    autograd (float64, this forward's leaky-ReLU regions injected), L the multi-scale loss
    against fixed random targets; also the engine (for its predicates)."""
    P = g_params(s, device=device)
    st = make_inputs(B, 4 * 2 ** s, seed=83)[0]
    z, tgt = torch.from_numpy(st["z1"]).to(device), torch.from_numpy(st["real"])
    levels = min(3, s + 2)
    eng = E.StepEngine(ops, TINY_DEPTHS, s, B, device, forward_only="Gtrain", **engine_options)
    eng.hyper = E.Hyper()
    eng.pack("G", P)
    img = eng.g_forward(P, z, alpha)
    kinks = O.Kinks(K.g_masks(eng))
    # the loss gradient at OUR image, in float64: both sides backpropagate the same dL/dimg
    gimg = RR.recon_loss_grad(img.detach().cpu(), tgt, levels)[2]
    gzn = eng.g_input_grad(P, gimg.float().to(device).contiguous(), alpha)
    ours = torch.empty_like(gzn)
    ops.pixnorm_lrelu_bwd(eng.g["z"], gzn, ours, 512, 1.0, mask=False)
    _, ref = RR.dz({k: v.cpu() for k, v in P.items()}, z.cpu(), s, alpha, lambda im: gimg, kinks)
    assert kinks.worst() <= K.FLIP_BOUND[ops.tdtype], kinks.worst()
    return K.rel_l2(ours.cpu(), ref), eng


@pytest.mark.parametrize("s,alpha,B", DZ_CASES)
def test_dz_matches_the_oracle(s, alpha, B):
    torch.set_num_threads(4)
    err, _ = dz_parity(CpuOpsRecover(), s, alpha, B)
    print(f"dz rel L2 {err:.2e}")
    assert err <= 1e-4, err


def test_dz_without_fused_epilogues():
    """The unfused generator path (separate PixelNorm kernels) through the same switch."""
    torch.set_num_threads(4)
    err, _ = dz_parity(CpuOpsRecover(fused=False), 2, 0.5, 4)
    assert err <= 1e-4, err


def autograd_dz(device="cpu", dtype=torch.float32, s=2, alpha=0.5, B=4):
    """z.requires_grad_(); G(z).square().mean().backward(): (rel L2 of z.grad against the
    oracle, parameter grads with z requiring grad, the same without)."""
    G = make_generator(s, alpha, device, dtype)
    z0 = torch.from_numpy(make_inputs(B, 4 * 2 ** s, seed=83)[0]["z1"]).to(device)
    z = z0.clone().requires_grad_()
    img = G(z)
    kinks = O.Kinks(K.g_masks(nets._ENGINES["Gtrain"][1]))
    img.square().mean().backward()
    g_with = {k: p.grad.clone() for k, p in G.named_parameters() if p.grad is not None}
    assert z.grad is not None and z.grad.shape == z.shape
    n = img.numel()
    _, ref = RR.dz(g_params(s), z0.cpu(), s, alpha,
                   lambda im: 2.0 * img.detach().cpu().double() / n, kinks)
    for p in G.parameters():
        p.grad = None
    G(z0).square().mean().backward()
    g_without = {k: p.grad.clone() for k, p in G.named_parameters() if p.grad is not None}
    # only z requires grad: the input-gradient pass, no parameter gradient
    G.requires_grad_(False)
    for p in G.parameters():
        p.grad = None
    z2 = z0.clone().requires_grad_()
    G(z2).square().mean().backward()
    assert all(p.grad is None for p in G.parameters())
    assert torch.equal(z2.grad, z.grad)
    return K.rel_l2(z.grad.cpu(), ref), g_with, g_without


def test_autograd_returns_dz(monkeypatch):
    torch.set_num_threads(4)
    monkeypatch.setattr(nets, "OPS_FACTORY", RecordingOps)
    nets._ENGINES.clear()
    err, g_with, g_without = autograd_dz()
    assert err <= 1e-4, err
    assert g_with.keys() == g_without.keys() and len(g_with) > 8
    for k in g_with:
        assert torch.equal(g_with[k], g_without[k]), k
    # the third backward (only z requires grad) launched no weight gradient
    calls = [c[0] for c in nets._ENGINES["Gtrain"][1].ops.calls]
    last_fwd = len(calls) - 1 - calls[::-1].index("rgb_out")
    tail = calls[last_fwd:]
    assert "linear_dgrad" in tail
    assert not {"conv_wgrad", "linear_wgrad", "bias_grad"} & set(tail), tail
    nets._ENGINES.clear()


# ---- the training step's launches are the ones before the switch existed --------------------
STEP_CASES = [("s2_b4_a05", 2, 4, 0.5), ("s2_b4_a1", 2, 4, 1.0), ("s1_b3_a05", 1, 3, 0.5)]


def step_calls(s, B, alpha):
    """(name, tensor shapes) of every op call of one training step on the CPU double."""
    gsh, dsh = E.g_param_shapes(TINY_DEPTHS, s), E.d_param_shapes(TINY_DEPTHS, s)
    PG = {k: torch.from_numpy(v) for k, v in make_params(gsh, seed=61).items()}
    PD = {k: torch.from_numpy(v) for k, v in make_params(dsh, seed=62).items()}
    fpG = E.FlatParams(gsh, E.dead_params("G", s), "cpu", PG)
    fpD = E.FlatParams(dsh, E.dead_params("D", s), "cpu", PD)
    ops = RecordingOps()
    eng = E.StepEngine(ops, TINY_DEPTHS, s, B, "cpu")
    eng.bind(fpG, fpD, E.Hyper())
    st = make_inputs(B, 4 * 2 ** s, seed=63)[0]
    r, z1, z2 = (torch.from_numpy(st[k]) for k in ("real", "z1", "z2"))
    ops.calls.clear()
    eng.train_step(r, z1, z2, alpha, alpha)
    eng.flush()
    return [[n, [list(x) for x in sh]] for n, sh in ops.calls]


@pytest.mark.parametrize("name,s,B,alpha", STEP_CASES)
def test_training_step_issues_the_same_calls(name, s, B, alpha):
    """tests/golden/step_calls.json holds the op-call sequence (names and tensor shapes) of a
    training step recorded with this file's step_calls() on the engine as it was before
    g_backward got its switch: with the defaults the step must issue exactly those calls."""
    torch.set_num_threads(4)
    with open(os.path.join(GOLDEN, "step_calls.json")) as f:
        before = json.load(f)[name]
    now = step_calls(s, B, alpha)
    assert len(now) == len(before), (len(now), len(before))
    for i, (a, b) in enumerate(zip(now, before)):
        assert a == b, (i, a, b)
    assert any(n == "conv_wgrad" for n, _ in now) and not any(n == "linear_dgrad" and
                                                                  sh[-1] == [B, 512] for n, sh in now)


# ---- recovery works ---------------------------------------------------------------------------
CONV_CASES = [(2, 1.0, 4, 3), (1, 0.5, 3, 2)]                         # (s, alpha, B, levels)


def convergence(s, alpha, B, levels, device="cpu", dtype=torch.float32, steps=60, lr=0.1):
    """Targets G(z1), start z2: (first loss, best loss) per sample, and the loss history."""
    G = make_generator(s, alpha, device, dtype)
    st = make_inputs(B, 4 * 2 ** s, seed=83)[0]
    z1, z2 = (torch.from_numpy(st[k]).to(device) for k in ("z1", "z2"))
    with torch.no_grad():
        targets = G(z1)
    trace = []
    z, loss, mse0, img = R.recover_latents(G, targets, steps=steps, lr=lr, levels=levels, z0=z2,
                                           batch=B, trace=trace)
    hist = torch.stack(trace[0]).cpu()
    assert z.shape == (B, 512) and img.shape == targets.shape and mse0.shape == (B,)
    # what is returned is the best latent visited, and its image
    assert torch.allclose(loss.cpu(), hist.min(0).values, rtol=1e-5, atol=0)
    return hist[0], loss.cpu(), hist, (targets, z2)


@pytest.mark.parametrize("s,alpha,B,levels", CONV_CASES)
def test_recovery_converges(monkeypatch, s, alpha, B, levels):
    torch.set_num_threads(4)
    monkeypatch.setattr(nets, "OPS_FACTORY", CpuOpsRecover)
    nets._ENGINES.clear()
    first, best, hist, _ = convergence(s, alpha, B, levels)
    ratio = best / first
    print(f"best / first loss: {[f'{float(r):.4f}' for r in ratio]}")
    assert bool((ratio <= 0.25).all()), ratio
    nets._ENGINES.clear()


def test_partial_batches_reuse_the_engine(monkeypatch):
    """5 targets in batches of 2: three runs on one engine, results in target order, each equal
    to the same target recovered alone in its batch position (per-sample arithmetic)."""
    torch.set_num_threads(4)
    monkeypatch.setattr(nets, "OPS_FACTORY", CpuOpsRecover)
    nets._ENGINES.clear()
    G = make_generator(1, 1.0)
    st = make_inputs(5, 8, seed=84)[0]
    tg, z0 = torch.from_numpy(st["real"]), torch.from_numpy(st["z1"])
    made = []
    init = R.LatentRecovery.__init__
    monkeypatch.setattr(R.LatentRecovery, "__init__",
                        lambda self, *a, **kw: (made.append(1), init(self, *a, **kw))[1])
    z, loss, mse0, img = R.recover_latents(G, tg, steps=3, z0=z0, batch=2)
    assert len(made) == 1 and z.shape == (5, 512) and img.shape == tg.shape
    z4, loss4, _, _ = R.recover_latents(G, tg[4:], steps=3, z0=z0[4:], batch=2)
    assert torch.allclose(z[4:], z4, rtol=0, atol=1e-6) and torch.allclose(loss[4:], loss4, rtol=1e-6)
    with pytest.raises(ValueError):
        R.recover_latents(G, tg[:, :, :4, :4])
    with pytest.raises(RuntimeError):
        R.recover_latents(G, tg, steps=1, levels=5)          # 8 x 8 has 4 levels
    assert R.default_levels(4) == 1 and R.default_levels(8) == 2 and R.default_levels(1024) == 5


def test_cpu_double_matches_the_reference():
    """The closed forms of the CPU double against the autograd reference (the GPU kernels are
    held to the same reference in test_gpu_recover.py)."""
    torch.manual_seed(5)
    ops = CpuOpsRecover()
    for B, Rr, levels in [(3, 4, 3), (2, 32, 6), (1, 64, 4)]:
        img, tgt = torch.randn(B, 3, Rr, Rr), torch.randn(B, 3, Rr, Rr)
        gimg, loss, mse0 = torch.empty_like(img), torch.empty(B), torch.empty(B)
        ops.recon_loss(img, tgt, levels, gimg, loss, mse0)
        rl, rm, rg = RR.recon_loss_grad(img, tgt, levels)
        assert K.rel_l2(loss, rl) <= 1e-5 and K.rel_l2(mse0, rm) <= 1e-5
        assert float((gimg.double() - rg).abs().max()) <= 1e-5 * float(rg.abs().max())
    with pytest.raises(RuntimeError):
        ops.recon_loss(img, tgt, 7, gimg, loss, mse0)


def test_validation_entry_on_the_cpu_double(monkeypatch, tmp_path):
    """recover_images through validation() at 4 x 4 (where it is the whole dict): the csv row,
    the figure, the three keys; uint8 and fp32 targets through ProgressiveGAN.recover; and the
    training state of a model that validated equals that of one that did not."""
    import csv

    from pggan_amd.model import ProgressiveGAN
    from test_model_api import fresh_model, make_args
    torch.set_num_threads(4)
    monkeypatch.setattr(ProgressiveGAN, "ops_factory", staticmethod(CpuOpsRecover))
    monkeypatch.setattr(nets, "OPS_FACTORY", CpuOpsRecover)
    nets._ENGINES.clear()
    models = []
    for name, nrec in (("a", 3), ("b", None)):
        torch.manual_seed(7)
        args = make_args(tmp_path / name, use_validation=True, swd_images=8, valid_cycle=1,
                         recover_images=nrec, recover_steps=4, isMaster=True)
        m = fresh_model(args)
        m.set_validation()
        m.train_step()
        models.append(m)
    with_, without = models
    out = with_.validation(2)
    assert sorted(out) == ["rec_fake", "rec_real", "rec_train"]
    rows = list(csv.reader(open(tmp_path / "a" / "t" / "recover.csv")))
    assert len(rows) == 1 and rows[0][:4] == ["2", "0", "4", "1"] and len(rows[0]) == 7
    assert os.path.getsize(tmp_path / "a" / "t" / "recover" / "e2.jpg") > 0
    assert without.validation(2) is None
    x = torch.rand(2, 3, 4, 4) * 2 - 1
    u8 = ((x.permute(0, 2, 3, 1) + 1) * 127.5).round().clamp(0, 255).to(torch.uint8)
    z, loss, mse0, img = with_.recover(u8, steps=2)
    z2, loss2, _, _ = with_.recover(u8.permute(0, 3, 1, 2).float() / 127.5 - 1, steps=2)
    assert z.shape == (2, 512) and img.shape == (2, 3, 4, 4) and torch.equal(z, z2)
    with pytest.raises(ValueError):
        with_.recover(torch.zeros(2, 3, 8, 8))
    for m in models:
        m.train_step()
        m.flush()
    for a, b in ((with_.fpG, without.fpG), (with_.fpD, without.fpD)):
        for k in ("flat", "grad", "m", "v"):
            assert torch.equal(getattr(a, k), getattr(b, k)), k
    with pytest.raises(ValueError):
        bad = make_args(tmp_path / "c", use_validation=True, swd_images=8, recover_images=9)
        fresh_model(bad).set_validation()
    nets._ENGINES.clear()
