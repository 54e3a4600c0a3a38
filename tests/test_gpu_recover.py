"""Latent recovery on the HIP kernels: pg_recon_loss and pg_latent_step against the float64
reference (tests/recover_ref.py), pg_linear_dgrad at the latent layer's shape, dL/dz through
the generator's input-gradient pass, the autograd surface, the convergence case of
test_recover_cpu.py, and the validation entry end to end."""
import csv
import os

import pytest
import torch

import kink_parity as K
import recover_ref as RR
from cpu_ops import CpuOps
from gen_inputs import TINY_DEPTHS
from test_gpu_graph import build
from test_model_api import make_args
from test_recover_cpu import CONV_CASES, autograd_dz, convergence, dz_parity

pytestmark = pytest.mark.gpu


def hip(dtype=torch.float32):
    from pggan_amd import _lib
    return _lib.HipOps(dtype)


def use_hip():
    from pggan_amd import nets
    from pggan_amd.model import ProgressiveGAN
    nets.OPS_FACTORY = None
    ProgressiveGAN.ops_factory = None
    nets._ENGINES.clear()


def rnd(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


# ------------------------------------------------------------------ pg_recon_loss
# (B, R, levels); the last two: more tiles than the launch has workgroups, so a workgroup takes
# several tiles (unevenly: 12 tiles over 10 workgroups; 48 over 25)
RECON_CASES = [(3, 4, 1), (3, 4, 3), (2, 32, 6), (2, 64, 6), (1, 128, 4), (100, 64, 6), (40, 128, 5)]


def run_recon(ops, img, tgt, levels):
    B = img.shape[0]
    gimg = torch.full_like(img, 7.0)
    loss, mse0 = (torch.full((B,), 7.0, device="cuda") for _ in range(2))
    ops.recon_loss(img, tgt, levels, gimg, loss, mse0)
    return loss, mse0, gimg


@pytest.mark.parametrize("B,R,levels", RECON_CASES)
def test_recon_loss(B, R, levels):
    ops = hip()
    img, tgt = rnd(B, 3, R, R, seed=R + levels), rnd(B, 3, R, R, seed=R + levels + 100)
    ref_loss, ref_mse0, ref_g = RR.recon_loss_grad(img, tgt, levels)
    loss, mse0, gimg = run_recon(ops, img.cuda(), tgt.cuda(), levels)
    e = {"loss": float(((loss.cpu().double() - ref_loss) / ref_loss).abs().max()),
         "mse0": float(((mse0.cpu().double() - ref_mse0) / ref_mse0).abs().max()),
         "gimg": float((gimg.cpu().double() - ref_g).abs().max() / ref_g.abs().max())}
    print(f"recon_loss B={B} R={R} levels={levels}: {e}")
    assert all(v <= 1e-5 for v in e.values()), e
    # bitwise repeatable
    again = run_recon(ops, img.cuda(), tgt.cuda(), levels)
    for a, b in zip((loss, mse0, gimg), again):
        assert torch.equal(a, b)
    # img == tgt: exact zeros
    for t in run_recon(ops, img.cuda(), img.cuda().clone(), levels):
        assert int(t.count_nonzero()) == 0


def test_recon_loss_refuses_bad_levels():
    ops = hip()
    x = torch.zeros(1, 3, 8, 8, device="cuda")
    for R, levels in [(8, 0), (8, 5), (64, 7)]:
        x = torch.zeros(1, 3, R, R, device="cuda")
        with pytest.raises(RuntimeError, match="recon_loss"):
            run_recon(ops, x, x.clone(), levels)
    run_recon(ops, x, x.clone(), 6)
    torch.cuda.synchronize()


# ------------------------------------------------------------------ pg_latent_step
@pytest.mark.parametrize("B,Lz", [(3, 512), (5, 64)])
def test_latent_step(B, Lz):
    ops = hip()
    lr, betas = 0.1, (0.9, 0.999)
    z0 = rnd(B, Lz, seed=Lz)
    ref = RR.LatentSteps(z0, lr, betas)
    z = z0.cuda().clone()
    m, v, gz, best_z = (torch.zeros(B, Lz, device="cuda") for _ in range(4))
    best_loss = torch.full((B,), float("inf"), device="cuda")
    z_in = []
    for t, lv in enumerate((3.0, 1.0, 2.0), start=1):
        gzn = rnd(B, Lz, seed=100 * t + Lz)
        loss = torch.full((B,), lv)
        z_in.append(z.clone())
        ops.latent_step(z, gzn.cuda(), m, v, lr=lr, beta1=betas[0], beta2=betas[1], eps=1e-8, step=t,
                        loss=loss.cuda(), best_loss=best_loss, best_z=best_z, gz_out=gz)
        rgz = ref.step(gzn, loss)
        rz, rm, rv = ref.state()
        e = {k: K.rel_l2(a.cpu(), b) for k, a, b in (("z", z, rz), ("m", m, rm), ("v", v, rv),
                                                     ("gz", gz, rgz))}
        print(f"latent_step B={B} Lz={Lz} step {t}: {e}")
        assert all(x <= 1e-6 for x in e.values()), (t, e)
    assert torch.equal(best_loss.cpu(), torch.full((B,), 1.0))
    assert torch.equal(best_z, z_in[1])
    assert K.rel_l2(best_z.cpu(), ref.best_z) <= 1e-6


def test_latent_step_refuses_other_widths():
    ops = hip()
    for Lz in (96, 576, 32):
        t = [torch.zeros(2, Lz, device="cuda") for _ in range(5)]
        l = [torch.zeros(2, device="cuda") for _ in range(2)]
        with pytest.raises(RuntimeError, match="latent_step"):
            ops.latent_step(t[0], t[1], t[2], t[3], lr=0.1, beta1=0.9, beta2=0.999, eps=1e-8, step=1,
                            loss=l[0], best_loss=l[1], best_z=t[4])


# ------------------------------------------------------------------ the latent layer's dgrad
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("B", [3, 8])
def test_linear_dgrad_latent_shape(dtype, B):
    """N = 16 * 32, K = 512, OUT_CHW on gy, fp32 gx: the launch g_input_grad ends with."""
    from pggan_amd import _lib
    d0, K_ = 32, 512
    gy = rnd(B, 4, 4, d0, seed=B).to(dtype).float()
    w = rnd(16 * d0, K_, seed=B + 1) * 0.05
    ref = torch.zeros(B, K_)
    CpuOps().linear_dgrad(gy, w, ref, B=B, flags=_lib.LIN_OUT_CHW, scale=0.3)
    gx = torch.full((B, K_), 7.0, device="cuda")
    hip(dtype).linear_dgrad(gy.cuda().to(dtype), w.cuda(), gx, B=B, flags=_lib.LIN_OUT_CHW, scale=0.3)
    e = K.rel_l2(gx.cpu(), ref)
    print(f"linear_dgrad latent shape {dtype} B={B}: {e:.2e}")
    assert e <= (2e-5 if dtype == torch.float32 else 2e-2), e


# ------------------------------------------------------------------ dz
DZ_TOL = {torch.float32: 1e-3, torch.bfloat16: 5e-2}


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("s,alpha,B", [(2, 0.5, 4), (0, 1.0, 3)])
def test_dz_on_hip(dtype, s, alpha, B):
    err, _ = dz_parity(hip(dtype), s, alpha, B, device="cuda")
    print(f"dz {dtype} s={s} alpha={alpha}: rel L2 {err:.2e}")
    assert err <= DZ_TOL[dtype], err


def fused_stage(ops, B=4):
    """The smallest stage at which the engine answers true for the fused PixelNorm forward, its
    fused backward and the toRGB + PixelNorm backward with TINY_DEPTHS (asked, not guessed)."""
    from pggan_amd import _lib as L
    from pggan_amd import engine as E
    d = TINY_DEPTHS
    for s in range(1, 6):                  # up to 128^2: larger stages are not a quick test
        eng = E.StepEngine(ops, d, s, B, "cuda", forward_only="G")
        R = 4 * 2 ** s
        if (eng._pn_fused(R, d[s], d[s], L.CONV_LRELU) and eng._pnb_fused(R, d[s - 1], d[s]) and
                d[s] in (16, 32) and eng.fuse_rgb_pnbwd and hasattr(ops, "rgb_out_bwd_pn")):
            return s
    return None


def test_dz_with_fused_epilogues_bf16():
    """Where a pass without weight gradients runs the fused epilogues with operands the
    training step never omits (rgb_out_bwd_pn without dw / db)."""
    ops = hip(torch.bfloat16)
    s = fused_stage(ops)
    if s is None:
        pytest.skip("with TINY_DEPTHS the engine fuses these epilogues at no stage up to 128^2")
    err, eng = dz_parity(ops, s, 1.0, 4, device="cuda")
    print(f"dz bf16 fused epilogues, stage {s} ({4 * 2 ** s}^2): rel L2 {err:.2e}")
    assert err <= DZ_TOL[torch.bfloat16], err


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_autograd_dz_on_hip(dtype):
    use_hip()
    err, g_with, g_without = autograd_dz(device="cuda", dtype=dtype)
    print(f"autograd dz {dtype}: rel L2 {err:.2e}")
    assert err <= DZ_TOL[dtype], err
    for k in g_with:
        assert torch.equal(g_with[k], g_without[k]), k


# ------------------------------------------------------------------ recovery works
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("s,alpha,B,levels", CONV_CASES)
def test_recovery_converges_on_hip(dtype, s, alpha, B, levels):
    use_hip()
    first, best, hist, _ = convergence(s, alpha, B, levels, device="cuda", dtype=dtype)
    ratio = best / first
    print(f"{dtype} s={s}: best / first loss {[f'{float(r):.4f}' for r in ratio]}")
    assert bool((ratio <= 0.25).all()), ratio


# ------------------------------------------------------------------ validation end to end
def model(tmp_path, nrec):
    args = make_args(tmp_path, depths=list(TINY_DEPTHS), use_validation=True, swd_images=8,
                     valid_cycle=1, recover_images=nrec, recover_steps=5, isMaster=True)
    m = build(args, False, 1)
    m.set_validation()
    m.G.alpha = m.D.alpha = 0.5
    return m


def test_validation_recovers_and_leaves_training_alone(tmp_path):
    with_, without = model(tmp_path / "a", 4), model(tmp_path / "b", None)
    for m in (with_, without):
        m.train_step()
    out = with_.validation(3)
    assert {"rec_train", "rec_real", "rec_fake"} <= set(out), out
    assert all(out[k] >= 0 and out[k] == out[k] for k in ("rec_train", "rec_real", "rec_fake"))
    d = tmp_path / "a" / "t"
    rows = list(csv.reader(open(d / "recover.csv")))
    assert len(rows) == 1 and len(rows[0]) == 7, rows
    assert rows[0][:4] == ["3", "1", "5", "2"], rows
    assert [float(x) for x in rows[0][4:]] == [out["rec_train"], out["rec_real"], out["rec_fake"]]
    assert os.path.getsize(d / "recover" / "e3.jpg") > 0
    assert without.validation(3) is None                  # 8 x 8: nothing else is defined there
    for m in (with_, without):
        m.train_step()
        m.flush()
    for a, b in ((with_.fpG, without.fpG), (with_.fpD, without.fpD)):
        for k in ("flat", "grad", "m", "v"):
            assert torch.equal(getattr(a, k), getattr(b, k)), k
    assert torch.equal(with_._z, without._z)
