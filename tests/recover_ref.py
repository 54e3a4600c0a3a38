"""Float64 torch reference of latent recovery (test infrastructure): the multi-scale pixel loss
by avg_pool2d with autograd for its image gradient, the latent step as torch.optim.Adam on z
through oracle.pixel_norm, and the whole loop on oracle.generator_forward.  Independent of the
closed forms in csrc/recover.hip and tests/cpu_ops_recover.py: every gradient here is autograd's."""
import torch
import torch.nn.functional as F

from oracle import pggan_oracle as O


def recon_loss(img, tgt, levels):
    """(loss [B], mse0 [B]) of pg_recon_loss's definition, in the dtype of img (differentiable)."""
    B, _, R, _ = img.shape
    d = img - tgt
    terms = []
    for l in range(levels):
        dl = F.avg_pool2d(d, 2 ** l) if l else d
        terms.append((dl * dl).reshape(B, -1).sum(1) / (3 * (R >> l) ** 2))
    return sum(terms), terms[0]


def recon_loss_grad(img, tgt, levels):
    """(loss, mse0, gimg) in float64; gimg by autograd."""
    x = img.detach().double().clone().requires_grad_()
    loss, mse0 = recon_loss(x, tgt.detach().double(), levels)
    g, = torch.autograd.grad(loss.sum(), x)
    return loss.detach(), mse0.detach(), g


class LatentSteps:
    """pg_latent_step's contract in float64: torch.optim.Adam on z, the gradient arriving at
    zn = oracle.pixel_norm(z); best (loss, z) tracked before each step."""

    def __init__(self, z0, lr, betas=(0.9, 0.999), eps=1e-8):
        self.z = z0.detach().double().clone().requires_grad_()
        self.opt = torch.optim.Adam([self.z], lr=lr, betas=betas, eps=eps)
        self.best_loss = torch.full((z0.shape[0],), float("inf"), dtype=torch.float64)
        self.best_z = self.z.detach().clone()

    def step(self, gzn, loss):
        """Returns gz, the gradient Adam used."""
        better = loss.double() < self.best_loss
        self.best_loss = torch.where(better, loss.double(), self.best_loss)
        self.best_z = torch.where(better[:, None], self.z.detach(), self.best_z)
        self.opt.zero_grad()
        O.pixel_norm(self.z).backward(gzn.double())
        gz = self.z.grad.detach().clone()
        self.opt.step()
        return gz

    def state(self):
        st = self.opt.state[self.z]
        return self.z.detach().clone(), st["exp_avg"].clone(), st["exp_avg_sq"].clone()


def dz(P, z, s, alpha, gimg_fn, kinks=None, slope_cfg=0.2):
    """(img, dL/dz) on the oracle generator in float64: gimg_fn(img) -> dL/dimg."""
    P64 = {k: v.detach().double() for k, v in P.items()}
    zz = z.detach().double().clone().requires_grad_()
    img = O.generator_forward(P64, zz, s, alpha, slope_cfg=slope_cfg, kinks=kinks)
    img.backward(gimg_fn(img.detach()).double())
    return img.detach(), zz.grad.detach()


def recover(P, targets, z0, s, alpha, steps, lr, levels, betas=(0.9, 0.999), dtype=torch.float64):
    """The loop of pggan_amd.recover.LatentRecovery.run on oracle.generator_forward with
    autograd: (best z, best loss, losses of the steps + 1 latents visited [steps + 1, B])."""
    Pd = {k: v.detach().to(dtype) for k, v in P.items()}
    tgt = targets.detach().to(dtype)
    z = z0.detach().to(dtype).clone().requires_grad_()
    opt = torch.optim.Adam([z], lr=lr, betas=betas)
    best = torch.full((z.shape[0],), float("inf"), dtype=dtype)
    best_z = z.detach().clone()
    hist = []
    for t in range(steps + 1):
        loss, _ = recon_loss(O.generator_forward(Pd, z, s, alpha), tgt, levels)
        hist.append(loss.detach().clone())
        better = loss.detach() < best
        best = torch.where(better, loss.detach(), best)
        best_z = torch.where(better[:, None], z.detach(), best_z)
        if t == steps:
            break
        opt.zero_grad()
        loss.sum().backward()
        opt.step()
    return best_z, best, torch.stack(hist)
