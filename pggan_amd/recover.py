"""Latent recovery: which images can a generator produce?

Given target images x, minimise a multi-scale pixel loss between G(z) and x over the latent z
(DESIGN.md "Validation: latent recovery").  A generator that reconstructs its training images
clearly better than held-out reals has memorised them; how well any real image is reconstructed
is a coverage figure; and the recovered z is the entry point for projecting or editing an
image.

Every iteration runs on the HIP kernels with nothing read back to the host:

    StepEngine.g_forward -> pg_recon_loss -> StepEngine.g_input_grad -> pg_latent_step

g_input_grad is the generator's input-gradient chain alone (no weight gradient), pg_recon_loss
the loss and its image gradient in one launch, pg_latent_step the PixelNorm backward, Adam and
the best-so-far bookkeeping (the loss is not monotone under Adam) in one launch.
"""
from __future__ import annotations

import math

import torch

from . import engine as E
from . import nets


def default_levels(R):
    """min(5, log2 R - 1), at least 1: the coarsest level compared is 4 x 4 up to 128^2."""
    return max(1, min(5, int(math.log2(R)) - 1))


class LatentRecovery:
    """The buffers and the weights of one generator, packed once, for batches of B targets:
    an engine of its own (the generator's forward and first-order backward buffers), so
    neither a training engine nor the autograd modules' engines are touched."""

    def __init__(self, G, B, levels=None, lr=0.1, betas=(0.9, 0.999), eps=1e-8):
        from . import _lib
        p0 = next(G.parameters())
        self.dev, self.B = p0.device, int(B)
        self.s, self.alpha = G.scale_index, float(G.alpha)
        self.R = 4 * 2 ** self.s
        self.levels = default_levels(self.R) if levels is None else int(levels)
        self.lr, self.betas, self.eps = float(lr), (float(betas[0]), float(betas[1])), float(eps)
        factory = nets.OPS_FACTORY or _lib.HipOps
        self.ops = factory(G.compute_dtype)
        self.eng = eng = E.StepEngine(self.ops, G.block_depths, self.s, self.B, self.dev,
                                      G.latent_dim, forward_only="Gtrain")
        eng.hyper = E.Hyper(slope_cfg=G.LReLU_slope)
        self.P = {k: v.detach() for k, v in G.named_parameters()}
        eng.pack("G", self.P)
        f32 = dict(dtype=torch.float32, device=self.dev)
        Lz = G.latent_dim
        self.z, self.m, self.v, self.best_z = (torch.zeros(self.B, Lz, **f32) for _ in range(4))
        self.gimg = torch.zeros(self.B, 3, self.R, self.R, **f32)
        self.loss, self.mse0, self.best_loss = (torch.zeros(self.B, **f32) for _ in range(3))

    def _loss(self, tgt):
        """Forward of the current z and the loss against tgt: self.loss, self.mse0, self.gimg."""
        img = self.eng.g_forward(self.P, self.z, self.alpha)
        self.ops.recon_loss(img, tgt, self.levels, self.gimg, self.loss, self.mse0)
        return img

    def run(self, tgt, z0, steps, trace=None):
        """`steps` Adam steps from z0 on B targets.  Returns (z, loss, mse0, images) of the best
        of the steps + 1 latents visited, as fresh tensors.  trace: a list that receives the
        loss [B] of every latent visited, in order (device tensors: no read-back here)."""
        eng, ops, P = self.eng, self.ops, self.P
        self.z.copy_(z0)
        self.best_z.copy_(z0)
        self.m.zero_()
        self.v.zero_()
        self.best_loss.fill_(float("inf"))
        b1, b2 = self.betas
        for t in range(1, steps + 1):
            self._loss(tgt)
            if trace is not None:
                trace.append(self.loss.clone())
            gzn = eng.g_input_grad(P, self.gimg, self.alpha)
            ops.latent_step(self.z, gzn, self.m, self.v, lr=self.lr, beta1=b1, beta2=b2,
                            eps=self.eps, step=t, loss=self.loss, best_loss=self.best_loss,
                            best_z=self.best_z)
        # the latent the last step produced has not been looked at yet
        self._loss(tgt)
        if trace is not None:
            trace.append(self.loss.clone())
        better = self.loss < self.best_loss
        self.best_z.copy_(torch.where(better[:, None], self.z, self.best_z))
        self.z.copy_(self.best_z)
        img = self._loss(tgt)        # G at the best z: its image, loss and level-0 term
        return self.z.clone(), self.loss.clone(), self.mse0.clone(), img.clone()


def recover_latents(G, targets, steps=200, lr=0.1, levels=None, seed=0, z0=None,
                    betas=(0.9, 0.999), batch=16, trace=None):
    """Latents whose images are nearest to `targets` (fp32 [N, 3, R, R] in [-1, 1] at G's
    current size, on G's device) under the multi-scale pixel loss of pg_recon_loss, by
    `steps` Adam steps on z at G's current alpha.

    Returns (z [N, latent], loss [N], mse0 [N], images [N, 3, R, R]): per target the best
    latent visited, its loss, the loss's full-resolution term (the mean squared pixel error;
    sqrt(mse0) * 127.5 is the RMS error on the 0..255 scale) and G at that latent.

    levels: box-pyramid levels compared, 1 <= levels <= min(6, log2 R + 1); default
    min(5, log2 R - 1), at least 1.  z0: the starting latents [N, latent]; default N(0, 1)
    draws from `seed`.  batch: targets optimised together (the engine's batch size; a last
    partial batch is filled up with its first targets).  trace: a list that receives, per
    batch, the list of per-latent loss tensors (LatentRecovery.run).

    The defaults (lr, steps, levels) are what converged on the float64 oracle with random
    weights at 8^2 and 16^2 (tests/test_recover_cpu.py).  Nobody has measured them on a
    trained network: treat them as a starting point."""
    if targets.dim() != 4 or targets.shape[1] != 3 or targets.shape[2] != targets.shape[3]:
        raise ValueError(f"recover_latents: targets must be [N, 3, R, R], got {tuple(targets.shape)}")
    R = 4 * 2 ** G.scale_index
    if targets.shape[-1] != R:
        raise ValueError(f"recover_latents: targets are {targets.shape[-1]}^2, the generator "
                         f"produces {R}^2")
    N = targets.shape[0]
    B = min(N, int(batch))
    rec = LatentRecovery(G, B, levels=levels, lr=lr, betas=betas)
    tg = targets.to(rec.dev, torch.float32).contiguous()
    if z0 is None:
        gen = torch.Generator().manual_seed(int(seed))
        z0 = torch.randn(N, G.latent_dim, generator=gen)
    z0 = z0.reshape(N, -1).to(rec.dev, torch.float32)
    outs = []
    with torch.no_grad():
        for i in range(0, N, B):
            n = min(B, N - i)
            idx = [i + (j % n) for j in range(B)]      # a partial batch wraps around
            tr = None
            if trace is not None:
                tr = []
                trace.append(tr)
            res = rec.run(tg[idx].contiguous() if n < B else tg[i:i + B], z0[idx], steps, tr)
            outs.append([t[:n] for t in res])
    return tuple(torch.cat([o[k] for o in outs]) for k in range(4))
