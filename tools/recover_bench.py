"""Times one latent-recovery iteration (pggan_amd/recover.py over csrc/recover.hip and the step
engine) and its parts, per DESIGN.md "Validation: latent recovery", at the paper's depths in
bf16.  Device events around back-to-back calls of each part, a warm-up, then the median of
--runs repetitions.

    python tools/recover_bench.py [--res 128 1024] [--batch 4 16] [--json profiles/recover_bench.json]

"iteration": g_forward -> recon_loss -> g_input_grad -> latent_step, as LatentRecovery.run
issues them; "forward", "recon_loss", "input_grad", "latent_step": each alone.  "iteration_full_bwd":
the same iteration with the full g_backward in place of g_input_grad, every weight and bias
gradient included: what dL/dz costs through the autograd path of a generator whose parameters
require grad.  "recon_torch": the same loss and image gradient with torch ops (an avg_pool2d
chain and autograd); nothing in that baseline is tuned.  "copy": dst.copy_(src) of one image
tensor, which reads and writes its bytes once each; recon_loss reads two such tensors and writes
one, so 1.5 x the copy time is its HBM floor."""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from pggan_amd import nets, recover  # noqa: E402

PAPER_DEPTHS = [512, 512, 512, 512, 256, 128, 64, 32, 16]


def timed(fn, runs, inner, warm=2):
    """Median / min device time of one fn() in ms: events around `inner` calls issued back to
    back, so the figure is the device's time per call, not the host's time to issue one."""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) / inner)
    return statistics.median(ts), min(ts)


def torch_recon(img, tgt, levels):
    x = img.detach().requires_grad_()
    B, _, R, _ = x.shape
    d = x - tgt
    loss = 0
    for l in range(levels):
        dl = F.avg_pool2d(d, 2 ** l) if l else d
        loss = loss + (dl * dl).reshape(B, -1).sum(1) / (3 * (R >> l) ** 2)
    g, = torch.autograd.grad(loss.sum(), x)
    return loss.detach(), g


def bench(G, R, B, runs):
    s = G.scale_index
    rec = recover.LatentRecovery(G, B)
    eng, ops, P = rec.eng, rec.ops, rec.P
    gen = torch.Generator(device="cuda").manual_seed(R + B)
    tgt = torch.rand(B, 3, R, R, device="cuda", generator=gen) * 2 - 1
    rec.z.copy_(torch.randn(B, G.latent_dim, device="cuda", generator=gen))
    rec.best_loss.fill_(float("inf"))
    GR = {n: torch.zeros_like(p) for n, p in P.items()}
    kw = dict(lr=rec.lr, beta1=rec.betas[0], beta2=rec.betas[1], eps=rec.eps, step=1, loss=rec.loss,
              best_loss=rec.best_loss, best_z=rec.best_z)
    z_keep = rec.z.clone()

    def forward():
        return eng.g_forward(P, rec.z, rec.alpha)

    def loss():
        ops.recon_loss(eng.g["img"], tgt, rec.levels, rec.gimg, rec.loss, rec.mse0)

    def input_grad():
        eng.g_input_grad(P, rec.gimg, rec.alpha)

    def step():
        rec.z.copy_(z_keep)      # the timed latents stay finite whatever the step does to them
        ops.latent_step(rec.z, eng.g["gzn"], rec.m, rec.v, **kw)

    def iteration():
        forward(); loss(); input_grad(); step()

    def iteration_full():
        forward(); loss()
        eng.g_backward(P, GR, rec.gimg, rec.alpha, gzn=eng.g["gzn"])
        step()

    inner = 10 if R <= 128 else 3
    res = {"R": R, "B": B, "stage": s, "dtype": "bf16", "levels": rec.levels,
           "image_MB": B * 3 * R * R * 4 / 1e6}
    iteration()
    for name, fn in (("iteration", iteration), ("forward", forward), ("recon_loss", loss),
                     ("input_grad", input_grad), ("latent_step", step),
                     ("iteration_full_bwd", iteration_full)):
        res[name + "_ms"], res[name + "_min_ms"] = timed(fn, runs, inner)
    res["full_bwd_over_input_grad"] = res["iteration_full_bwd_ms"] / res["iteration_ms"]
    img = eng.g["img"].clone()
    res["recon_torch_ms"], _ = timed(lambda: torch_recon(img, tgt, rec.levels), runs, inner)
    dst = torch.empty_like(img)
    res["copy_ms"], _ = timed(lambda: dst.copy_(img), runs, inner)
    res["recon_floor_ms"] = 1.5 * res["copy_ms"]
    res["recon_GBps"] = 3 * B * 3 * R * R * 4 / (res["recon_loss_ms"] * 1e-3) / 1e9
    res["recon_vs_floor"] = res["recon_loss_ms"] / res["recon_floor_ms"]
    res["recon_speedup_vs_torch"] = res["recon_torch_ms"] / res["recon_loss_ms"]
    # the two losses agree
    loss()
    tl, tg = torch_recon(img, tgt, rec.levels)
    res["recon_loss_rel_diff_vs_torch"] = float(((rec.loss - tl) / tl).abs().max())
    res["recon_gimg_rel_diff_vs_torch"] = float((rec.gimg - tg).abs().max() / tg.abs().max())
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, nargs="+", default=[128, 1024])
    ap.add_argument("--batch", type=int, nargs="+", default=[4, 16])
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("recover_bench: needs a GPU (timings on a CPU would say nothing)")
    out = []
    torch.manual_seed(0)
    for R in a.res:
        s = R.bit_length() - 3
        if 4 * 2 ** s != R or not 1 <= s < len(PAPER_DEPTHS):
            raise SystemExit(f"recover_bench: --res {R} is not a stage size of the paper's generator")
        G = nets.Generator(512, PAPER_DEPTHS[0]).cuda()
        for i in range(1, s + 1):
            G.add_block(PAPER_DEPTHS[i])
        G.alpha = 1.0
        G.compute_dtype = torch.bfloat16
        G.requires_grad_(False)
        for B in a.batch:
            r = bench(G, R, B, a.runs)
            out.append(r)
            print(json.dumps(r), flush=True)
            if a.json:
                with open(a.json, "w") as f:
                    json.dump(out, f, indent=1)
    torch.cuda.synchronize()


if __name__ == "__main__":
    main()
