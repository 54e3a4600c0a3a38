"""ProgressiveGAN's validation (config `use_validation`): one `Validation` per model, which
streams reals and generated images once through the parts that are configured -- the paper's
sliced Wasserstein distance, its MS-SSIM, the nearest training images, latent recovery and the
radial power spectrum -- and owns what they share: the settings, one fp32 op set, the stage's nearest-neighbour
database.  The metrics themselves are pggan_amd.metrics and pggan_amd.recover.

A part is a plain class with
  name, min_res        what it is called when undefined, and the smallest stage it is defined at
  wants(s, master)     how many leading images of each set it reads (0 / None: not configured)
  feed(which, x)       a batch of the "real" or the "fake" set, in stream order
  finish(step, d, master) -> dict
                       print, append its csv row under d, write its figure, return its keys
and is listed in PARTS, whose order is that of the dict, the printed lines and the files."""
from __future__ import annotations

import math
import os

import numpy as np
import torch

from .config import cfg_get
from .data import image_paths, load_u8
from .metrics import (NN_MAX_K, SETS, MultiScaleSSIM, NearestNeighbours, PowerSpectrum,
                      SlicedWasserstein, spectrum_compare, spectrum_db)
from .recover import default_levels, recover_latents


# ---------------------------------------------------------------------- shared helpers
def u8_to_f32(u8):
    """uint8 NHWC -> fp32 NCHW in [-1, 1]."""
    return u8.permute(0, 3, 1, 2).float() / 127.5 - 1


def append_csv(path, *row):
    """One row: floats by repr() (they read back exactly), everything else by str()."""
    with open(path, "a") as f:
        f.write(",".join(repr(v) if isinstance(v, float) else str(v) for v in row) + "\n")


def write_grid_jpg(rows, d, step):
    """make_grid_image(rows) as {d}/e{step}.jpg, as save_image writes its own."""
    from .model import save_grid_jpg        # model imports this module
    save_grid_jpg(rows, d, step)


class Leading:
    """The first n images of each set as they pass by: cut(which, x) is the part of batch x
    that still belongs to them (empty once n have passed)."""

    def __init__(self, n):
        self.n, self.seen = n, dict.fromkeys(SETS, 0)

    def cut(self, which, x):
        x = x[:max(self.n - self.seen[which], 0)]
        self.seen[which] += x.shape[0]
        return x


# ---------------------------------------------------------------------- settings
def leading_count(args, key, what, images, each=1):
    """Config `key` (blank: None, the part is off): a count of `what` that takes `each` of the
    leading swd_images of a set apiece."""
    n = cfg_get(args, key, None)
    if not n:
        return None
    n = int(n)
    if n < 1 or each * n > images:
        need = f"{each} * {n}" if each > 1 else f"{n}"
        raise ValueError(f"{key}: {n} {what} need {need} of the swd_images = {images} images of a set")
    return n


def nn_settings(args):
    """(k, comparison resolution) of config `nn_k` (blank: 3) and `nn_resolution` (blank: 64)."""
    k = int(cfg_get(args, "nn_k", None) or 3)
    if k < 1 or k > NN_MAX_K:
        raise ValueError(f"nn_k: must be in [1, {NN_MAX_K}], got {k}")
    rc = int(cfg_get(args, "nn_resolution", None) or 64)
    if rc < 8 or rc > 128 or rc & (rc - 1):
        raise ValueError(f"nn_resolution: must be a power of two in [8, 128], got {rc}")
    return k, rc


def recover_settings(args):
    """recover_latents' keywords from config `recover_steps` (blank: 200), `recover_lr`
    (blank: 0.1) and `recover_levels` (blank: the module's default for the stage)."""
    steps = int(cfg_get(args, "recover_steps", None) or 200)
    lr = float(cfg_get(args, "recover_lr", None) or 0.1)
    levels = cfg_get(args, "recover_levels", None)
    if steps < 1 or not lr > 0:
        raise ValueError(f"recover_steps / recover_lr: must be positive, got {steps} / {lr}")
    if levels is not None and levels != "" and not 1 <= int(levels) <= 6:
        raise ValueError(f"recover_levels: must be in [1, 6], got {levels}")
    return dict(steps=steps, lr=lr, levels=int(levels) if levels not in (None, "") else None)


class Settings:
    """The validation keys of the config, read and checked once (set_validation).  The counts
    are None where their part is off; `nn` and `recover` are read only for a part that is on."""

    def __init__(self, args):
        self.images = int(cfg_get(args, "swd_images", None) or 4096)
        self.seed = int(cfg_get(args, "swd_seed", None) or 0)
        self.valid_cycle = int(cfg_get(args, "valid_cycle", None) or args.ckpt_cycle)
        self.msssim_pairs = leading_count(args, "msssim_pairs", "pairs", self.images, each=2)
        self.nn_queries = leading_count(args, "nn_queries", "queries", self.images)
        self.nn = nn_settings(args) if self.nn_queries else None
        self.recover_images = leading_count(args, "recover_images", "targets", self.images)
        self.recover = recover_settings(args) if self.recover_images else None
        self.spectrum_images = leading_count(args, "spectrum_images", "images", self.images)


# ---------------------------------------------------------------------- the parts
class SwdPart:
    """{R: v, .., 16: v, "avg": v}: the sliced Wasserstein distance x 1e3 per Laplacian level;
    swd.csv: step,scale,levels..,avg."""
    name, min_res = "SWD", 16

    @staticmethod
    def wants(s, master):
        return s.images

    def __init__(self, val, R, n):
        self.n, self.val = n, val
        self.swd = SlicedWasserstein(val.ops, R, n, seed=val.settings.seed)

    def feed(self, which, x):
        self.swd.feed(which, x)

    def finish(self, step, d, master):
        out = self.swd.result()
        if master:
            print(f"step {step}: SWD x1e3 " + " ".join(f"{k}:{out[k]:.4f}" for k in self.swd.sizes) +
                  f" avg:{out['avg']:.4f}")
        append_csv(f"{d}/swd.csv", step, self.val.model.scale_index,
                   *[out[k] for k in self.swd.sizes], out["avg"])
        return out


class MsssimPart:
    """Keys "msssim": the mean MS-SSIM over pairs of the first 2 * msssim_pairs generated images
    (lower is more diverse), "msssim_real": the reals' own, what the former is read against;
    msssim.csv: step,scale,msssim,msssim_real."""
    name, min_res = None, 16        # silent below 16 x 16

    @staticmethod
    def wants(s, master):
        return 2 * (s.msssim_pairs or 0)

    def __init__(self, val, R, n):
        self.n, self.val, self.first = n, val, Leading(n)
        self.ms = {w: MultiScaleSSIM(val.ops, R, n // 2) for w in SETS}

    def feed(self, which, x):
        x = self.first.cut(which, x)
        if len(x):
            self.ms[which].feed(x)

    def finish(self, step, d, master):
        out = {"msssim": self.ms["fake"].result(), "msssim_real": self.ms["real"].result()}
        if master:
            print(f"step {step}: MS-SSIM {out['msssim']:.4f} (reals {out['msssim_real']:.4f})")
        append_csv(f"{d}/msssim.csv", step, self.val.model.scale_index, out["msssim"],
                   out["msssim_real"])
        return out


class NnPart:
    """The first nn_queries images of each set against the stage's training images.  "nn",
    "nn_real": the median over the queries of the RMS pixel distance (0..255 scale) to the
    nearest training image, and "nn_min", the generated images' smallest: a generator that
    copies training images shows as nn, nn_min far below nn_real, the held-out reals' own
    distance.  nn.csv: step,scale,Rc,nn,nn_min,nn_real; nn/e{step}.jpg: the first 8 generated
    images in the top row, under each its k nearest training images."""
    name, min_res = "the nearest-neighbour search", 8

    @staticmethod
    def wants(s, master):
        return s.nn_queries

    def __init__(self, val, R, n):
        k, rc = val.settings.nn
        self.n, self.val = n, val
        self.nn = NearestNeighbours(val.ops, R, k, min(rc, R))
        self.first, self.first8 = Leading(n), Leading(min(n, 8))
        self.queries = {w: [] for w in SETS}    # (rows, sums) at the comparison resolution
        self.fakes = []                         # the generated images of the figure

    def feed(self, which, x):
        q = self.first.cut(which, x)
        if len(q):
            self.queries[which].append(self.nn.descriptors(q))
        x = self.first8.cut(which, x)
        if which == "fake" and len(x):
            self.fakes.append(x.detach().float().cpu())

    def finish(self, step, d, master):
        nn, val = self.nn, self.val
        desc, sq = val.nn_database(nn)
        near, res = {}, {}
        for w in ("fake", "real"):
            nn.set_query_descriptors(torch.cat([q for q, _ in self.queries[w]]),
                                     torch.cat([s for _, s in self.queries[w]]))
            nn.feed_descriptors(desc, sq, 0)
            near[w] = nn.rms()[:, 0].cpu().numpy()
            res[w] = nn.result()[0].cpu()
        out = {"nn": float(np.median(near["fake"])), "nn_real": float(np.median(near["real"])),
               "nn_min": float(near["fake"].min())}
        if master:
            print(f"step {step}: nearest training image at {nn.Rc}x{nn.Rc}, RMS of 255: median "
                  f"{out['nn']:.3f} min {out['nn_min']:.3f} (reals {out['nn_real']:.3f})")
        append_csv(f"{d}/nn.csv", step, val.model.scale_index, nn.Rc, out["nn"], out["nn_min"],
                   out["nn_real"])
        fakes = torch.cat(self.fakes)
        idx = res["fake"][:fakes.shape[0]]
        write_grid_jpg([fakes] + [val.nn_images(idx[:, j].tolist()) for j in range(nn.k)],
                       f"{d}/nn", step)
        return out


class RecoverPart:
    """Latent recovery of the first recover_images held-out reals, generated images and
    (fetched here, un-augmented) training images, on the master.  "rec_train", "rec_real",
    "rec_fake": the median over each set of sqrt(mse0) * 127.5, the RMS reconstruction error
    on the 0..255 scale nn.csv uses.  rec_fake calibrates the optimiser (the generator can
    produce its own samples: if this is not near zero the search fails, not the generator);
    rec_train far below rec_real is memorisation.  recover.csv:
    step,scale,steps,levels,rec_train,rec_real,rec_fake; recover/e{step}.jpg: the first 8
    training targets, their reconstructions, the first 8 held-out targets, their
    reconstructions."""
    name, min_res = "latent recovery", 4

    @staticmethod
    def wants(s, master):
        return s.recover_images if master else None

    def __init__(self, val, R, n):
        self.n, self.val, self.first = n, val, Leading(n)
        self.kw = dict(val.settings.recover)
        if self.kw["levels"] is None:
            self.kw["levels"] = default_levels(R)
        self.kw["levels"] = min(self.kw["levels"], int(math.log2(R)) + 1)
        self.sets = {w: [] for w in SETS}

    def feed(self, which, x):
        x = self.first.cut(which, x)
        if len(x):
            self.sets[which].append(x.detach().float().cpu())

    def finish(self, step, d, master):
        val, m, kw = self.val, self.val.model, self.kw
        sets = {w: torch.cat(t) for w, t in self.sets.items()}
        if m.train_dataset is None:
            if m.synthetic is None:
                raise RuntimeError("latent recovery: no training images (set_dataset first)")
            sets["train"] = m.synthetic[[j % m.synthetic.shape[0] for j in range(self.n)]].float()
        else:
            idx = [j % len(m.train_dataset) for j in range(self.n)]
            sets["train"] = m._stage_loader().raw_u8(idx)
        out, shown = {}, {}
        for w in ("train", "real", "fake"):
            # the starting latents come from seed + 2: not the draws (seed) behind the generated set
            _, _, mse0, img = val.recover(sets[w], fade=w != "fake", batch=int(m.args.batch_per_gpu),
                                          seed=val.settings.seed + 2, **kw)
            out[f"rec_{w}"] = float(np.median(np.sqrt(mse0.double().cpu().numpy()) * 127.5))
            shown[w] = img[:8].float().cpu()
        print(f"step {step}: latent recovery, {kw['steps']} steps, {kw['levels']} levels, RMS of 255: "
              f"train {out['rec_train']:.3f} held-out {out['rec_real']:.3f} "
              f"generated {out['rec_fake']:.3f}")
        append_csv(f"{d}/recover.csv", step, m.scale_index, kw["steps"], kw["levels"],
                   out["rec_train"], out["rec_real"], out["rec_fake"])
        tr = sets["train"][:8]
        if tr.dtype == torch.uint8:
            tr = u8_to_f32(tr)
        write_grid_jpg([tr.float().cpu(), shown["train"], sets["real"][:8], shown["real"]],
                       f"{d}/recover", step)
        return out


class SpectrumPart:
    """The radial power spectra of the first spectrum_images images of each set (luma of the
    8-bit image, |DFT2|^2 averaged over integer radius bins 0 .. K = R/2), compared bin by bin
    in dB, generated over real.  "spec_dist": the mean of |dB| over the bins 1 .. K;
    "spec_hf": the signed mean of dB over the top quarter of the bins -- positive: the
    generator has too much fine detail or noise, negative: too little (during the fade-in of a
    new block this quarter fills as alpha rises).  spectrum.csv: step,scale,spec_dist,spec_hf;
    spectrum/e{step}.csv, on the master: k,S_real,S_fake,dB per bin, bin 0 included."""
    name, min_res = "the power spectrum", 16

    @staticmethod
    def wants(s, master):
        return s.spectrum_images

    def __init__(self, val, R, n):
        self.n, self.val, self.first = n, val, Leading(n)
        self.ps = {w: PowerSpectrum(val.ops, R) for w in SETS}

    def feed(self, which, x):
        x = self.first.cut(which, x)
        if len(x):
            self.ps[which].feed(x)

    def finish(self, step, d, master):
        S = {w: self.ps[w].profile() for w in SETS}
        _, dist, hf = spectrum_compare(S["real"], S["fake"])
        out = {"spec_dist": dist, "spec_hf": hf}
        if master:
            print(f"step {step}: power spectrum, dB fake/real: mean |.| {dist:.3f}, "
                  f"top quarter {hf:+.3f}")
        append_csv(f"{d}/spectrum.csv", step, self.val.model.scale_index, dist, hf)
        if master:
            os.makedirs(f"{d}/spectrum", exist_ok=True)
            path = f"{d}/spectrum/e{step}.csv"
            open(path, "w").close()         # a step validated again replaces its table
            db = spectrum_db(S["real"], S["fake"])
            for k in range(len(db)):
                append_csv(path, k, float(S["real"][k]), float(S["fake"][k]), float(db[k]))
        return out


PARTS = (SwdPart, MsssimPart, NnPart, RecoverPart, SpectrumPart)


# ---------------------------------------------------------------------- the model's side
class Validation:
    """What ProgressiveGAN keeps for validation(), nearest_neighbours() and recover()."""

    def __init__(self, model):
        self.model = model
        self.settings = None    # Settings once set_validation found `use_validation` on
        self.nn_db = None       # ((scale_index, Rc), rows, sums) of the stage's training images
        self._ops = None

    def configure(self):
        """set_validation: the settings, or None with `use_validation` off."""
        self.settings = None
        if cfg_get(self.model.args, "use_validation", False):
            self.settings = Settings(self.model.args)
        return self.settings

    @property
    def ops(self):
        """The fp32 op set of everything here, made on first use."""
        if self._ops is None:
            from . import _lib
            self._ops = (type(self.model).ops_factory or _lib.HipOps)(torch.float32)
        return self._ops

    def stage_changed(self):
        """reset_solver: the nearest-neighbour database is that of the stage that ends."""
        self.nn_db = None

    # ------------------------------------------------------------------ the run
    def reals(self, R, n, B):
        """n validation reals at R x R as fp32 [-1, 1] batches of at most B: the images under
        `valid_dataset_root`, else the held-out 30 % of set_dataset, decoded like the training
        images without flip or jitter (wrapping around a shorter list); with `synthetic_data`
        fresh U[-1, 1) draws.  Nothing here is shared with the training loader."""
        m = self.model
        root = cfg_get(m.args, "valid_dataset_root", None)
        if root:
            paths = sorted(image_paths([root]))
            if not paths:
                raise RuntimeError(f"valid_dataset_root: no images under {root}")
        else:
            paths = list(getattr(m, "valid_paths", None) or [])
        if paths:
            for i in range(0, n, B):
                u8 = np.stack([load_u8(paths[j % len(paths)], R) for j in range(i, min(i + B, n))])
                yield u8_to_f32(torch.from_numpy(u8)).contiguous().to(m.device)
        elif cfg_get(m.args, "synthetic_data", False):
            g = torch.Generator().manual_seed(self.settings.seed + 1)
            for i in range(0, n, B):
                yield (torch.rand(min(B, n - i), 3, R, R, generator=g) * 2 - 1).to(m.device)
        else:
            raise RuntimeError("validation: no real images (set valid_dataset_root, or train on "
                               "a dataset so that its held-out 30 % is used)")

    def fakes(self, n, B):
        """n images of the averaged generator (G itself without `ema_decay`) for latents of a
        private generator, always sampled in whole batches: one sampling engine shape."""
        m = self.model
        g = torch.Generator().manual_seed(self.settings.seed)
        for i in range(0, n, B):
            z = torch.randn(B, m.args.latent_dim, generator=g).to(m.device)
            yield m.sample(z, ema=m.G_ema is not None)[:n - i]

    def run(self, step):
        """ProgressiveGAN.validation: None when off or when no configured part is defined at
        the stage, else the parts' keys in the order of PARTS."""
        s, m = self.settings, self.model
        if s is None:
            return None
        master = cfg_get(m.args, "isMaster", False)
        R = 4 * 2 ** m.scale_index
        parts = []
        for P in PARTS:
            n = P.wants(s, master)
            if n and R >= P.min_res:
                parts.append(P(self, R, n))
            elif n and master and P.name:
                print(f"step {step}: {P.name} is undefined below {P.min_res}x{P.min_res} "
                      f"(stage is {R}x{R})")
        if not parts:
            return None
        # every image SWD reads from 16 x 16 on; below, the leading ones the other parts read
        n, B = max(p.n for p in parts), int(m.args.batch_per_gpu)
        for which, images in (("real", self.reals(R, n, B)), ("fake", self.fakes(n, B))):
            for x in images:
                for p in parts:
                    p.feed(which, x)
        d = f"{m.args.save_root}/{m.args.run_id}"
        os.makedirs(d, exist_ok=True)
        out = {}
        for p in parts:
            out.update(p.finish(step, d, master))
        return out

    # ------------------------------------------------------------------ nearest neighbours
    def nn_database(self, nn):
        """(rows int8 [N, D], sums int32 [N]) of every image of train_dataset at the stage size,
        un-augmented (BatchLoader.raw_u8), or of the synthetic batch: built at the first use in
        a stage and kept until stage_changed.  N * D bytes of device memory."""
        m = self.model
        key = (m.scale_index, nn.Rc)
        if self.nn_db is not None and self.nn_db[0] == key:
            return self.nn_db[1:]
        if m.train_dataset is None:
            if m.synthetic is None:
                raise RuntimeError("nearest neighbours: no training images (set_dataset first)")
            desc, sq = nn.descriptors(m.synthetic)
        else:
            loader, n = m._stage_loader(), len(m.train_dataset)
            desc = torch.empty(n, nn.D, dtype=torch.int8, device=m.device)
            sq = torch.empty(n, dtype=torch.int32, device=m.device)
            for i in range(0, n, 64):
                j = min(i + 64, n)
                desc[i:j], sq[i:j] = nn.descriptors(loader.raw_u8(range(i, j)))
        self.nn_db = (key, desc, sq)
        return desc, sq

    def nn_images(self, idx):
        """Training images idx (a list; -1: none, left grey) at the stage size, fp32 NCHW on the CPU."""
        m = self.model
        R = 4 * 2 ** m.scale_index
        out = torch.zeros(len(idx), 3, R, R)
        live = [k for k, i in enumerate(idx) if i >= 0]
        if live and m.train_dataset is None:
            out[live] = m.synthetic[[idx[k] for k in live]].float().cpu()
        elif live:
            out[live] = u8_to_f32(m._stage_loader().raw_u8([idx[k] for k in live]).cpu())
        return out

    def nearest_neighbours(self, images, k=None):
        """ProgressiveGAN.nearest_neighbours; reads `nn_k` / `nn_resolution` itself, so it
        works without set_validation."""
        m = self.model
        R = 4 * 2 ** m.scale_index
        k0, rc = nn_settings(m.args)
        nn = NearestNeighbours(self.ops, R, k0 if k is None else k, min(rc, R))
        nn.set_queries(images.to(m.device))
        nn.feed_descriptors(*self.nn_database(nn), 0)
        idx, d2 = nn.result()
        return idx.clone(), d2.clone()

    # ------------------------------------------------------------------ latent recovery
    def recover(self, images, fade=True, **kw):
        """ProgressiveGAN.recover."""
        m = self.model
        m.flush()
        net = m.G
        if m.G_ema is not None:
            net = m.G_ema
            net.alpha = m.G.alpha
        R = 4 * 2 ** m.scale_index
        x = images.to(m.device)
        if x.dtype == torch.uint8 and x.dim() == 4 and x.shape[3] == 3:
            x = u8_to_f32(x)
        if x.dim() != 4 or tuple(x.shape[1:]) != (3, R, R):
            raise ValueError(f"recover: images must be fp32 [N, 3, {R}, {R}] or uint8 [N, {R}, {R}, 3], "
                             f"got {images.dtype} {tuple(images.shape)}")
        x = x.float().contiguous()
        alpha = float(net.alpha)
        if fade and m.scale_index >= 1 and alpha != 1.0:
            faded = torch.empty_like(x)
            self.ops.img_fade(x, alpha, faded)
            x = faded
        return recover_latents(net, x, **kw)
