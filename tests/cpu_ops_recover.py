"""CPU test double of the latent-recovery ops (pg_recon_loss, pg_latent_step) on top of
tests/cpu_ops.py's CpuOps -- TEST INFRASTRUCTURE ONLY.  Same argument meaning as
pggan_amd._lib.HipOps.recon_loss / latent_step, plain fp32 PyTorch, written from the
definitions in include/pggan_hip.h (closed forms, no autograd: tests/recover_ref.py is the
independent float64 autograd reference both are held to).  Every op call is appended to
`calls` as (name, shapes of its tensor arguments), for the schedule tests."""
import math

import torch
import torch.nn.functional as F

from cpu_ops import CpuOps


class CpuOpsRecover(CpuOps):
    def recon_loss(self, img, tgt, levels, gimg, loss, mse0):
        B, _, R, _ = img.shape
        if not 1 <= levels <= min(6, int(math.log2(R)) + 1):
            raise RuntimeError(f"recon_loss failed (-1): levels ({levels}) out of range at R = {R}")
        d = img - tgt
        g = torch.zeros_like(d)
        tot = torch.zeros(B)
        for l in range(levels):
            dl = F.avg_pool2d(d, 2 ** l) if l else d
            term = (dl * dl).reshape(B, -1).sum(1) / (3 * (R >> l) ** 2)
            if l == 0:
                mse0.copy_(term)
            tot = tot + term
            g = g + (dl.repeat_interleave(2 ** l, 2).repeat_interleave(2 ** l, 3) if l else dl)
        loss.copy_(tot)
        gimg.copy_(g * (2.0 / (3 * R * R)))

    def latent_step(self, z, gzn, m, v, *, lr, beta1, beta2, eps, step, loss, best_loss, best_z,
                    gz_out=None):
        B, Lz = z.shape
        if Lz % 64 or not 64 <= Lz <= 512:
            raise RuntimeError(f"latent_step failed (-1): Lz ({Lz}) must be a multiple of 64 in [64, 512]")
        better = loss < best_loss
        best_loss.copy_(torch.where(better, loss, best_loss))
        best_z.copy_(torch.where(better[:, None], z, best_z))
        r = ((z * z).mean(1, keepdim=True) + 1e-8).rsqrt()
        zn = z * r
        gz = r * (gzn - zn * (zn * gzn).mean(1, keepdim=True))
        self.adam(z, gz, m, v, lr=lr, beta1=beta1, beta2=beta2, eps=eps, step=step)
        if gz_out is not None:
            gz_out.copy_(gz)


def _shapes(args, kw):
    out = []
    for a in list(args) + [kw[k] for k in sorted(kw)]:
        if isinstance(a, torch.Tensor):
            out.append(tuple(a.shape))
        elif hasattr(a, "x0"):           # _lib.ImgMix
            out.append(("mix",) + tuple(a.x0.shape))
    return tuple(out)


class RecordingOps(CpuOpsRecover):
    """CpuOpsRecover that records every op call as (name, tensor shapes) in `calls`."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.calls = []

    def __getattribute__(self, name):
        v = super().__getattribute__(name)
        if name.startswith("_") or name in ("calls", "tdtype", "fused") or not callable(v):
            return v
        calls = super().__getattribute__("calls")

        def rec(*a, **kw):
            calls.append((name, _shapes(a, kw)))
            return v(*a, **kw)
        return rec
