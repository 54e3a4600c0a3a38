"""Input-pipeline throughput (GPU box): pggan_amd.data.BatchLoader on image
files written at run time, at every stage a BASELINE config trains (128^2 .. 1024^2 targets from
1024^2 sources: the host decodes the full image and resizes, lib/dataset.py:101-107), with the
decode threads the box's CPU share allows (16), next to the training step's rate.

    python tools/loader_bench.py [--n 64] [--workers 16] [--source-cache-gb G] [--out FILE]

Images: smooth synthetic RGB content (colour gradients + low-amplitude noise; pure noise
compresses like no photograph does) saved as 1024^2 PNG (the format of the reference's own sample
assets, assets/k-celeb).  Per target size, two epochs over the n images in the config's batch
size through `next(idx, prefetch)` exactly as ProgressiveGAN.load_next_batch chains them:
  cold -- the first epoch: every image decoded + resized on the host (the HBM cache fills);
  warm -- the second epoch: every batch gathered from the HBM cache (HbmImageCache).
img/s = images delivered on the GPU / wall time, synchronised per epoch.  One JSON line each.

--source-cache-gb G (> 0) adds, in the same process and on the same files:
  cold_source_cache -- per target size, the first epoch of a fresh loader (empty per-stage cache)
      that shares an HbmSourceCache filled beforehand by an untimed epoch at 64^2: the cold epoch
      of a stage entered after the first one, resized on the GPU (pg_resize_bilinear_u8; at
      1024^2 Pillow's plain copy), next to `cold`, the same epoch without the source cache.  Such
      an epoch lasts milliseconds, so five fresh loaders run it: the line is the median run,
      `runs_img_per_s` all five; `step_img_per_s` is the training step's rate at that stage as DESIGN.md records it;
  kernel -- pg_resize_bilinear_u8 alone on 16 cached 1024^2 sources -> 4^2, 128^2, 512^2: device
      events around 50 calls after 5 warm-up calls, as us per image and GB/s of source read.
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# (stage, batch per GPU) of the BASELINE configs: C2 128^2 B16, C3 256^2 B8, C4 512^2 B8, C5 1024^2 B4
STAGES = [(5, 16), (6, 8), (7, 8), (8, 4)]
# the step's rate at those stages, img/s (C2 R1, C3, the C4 shard, C5)
STEP_RATE = {5: 1052, 6: 515, 7: 566, 8: 375}


def epoch(ld, nb, B, base=0):
    """One epoch of nb batches through next(idx, prefetch) -> (seconds, last batch)."""
    idx = lambda k: list(range((k % nb) * B, (k % nb) * B + B))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for k in range(base, base + nb):
        out = ld.next(idx(k), prefetch=idx(k + 1))
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def kernel_lines(ops, sc, paths, n=16, iters=50, warmup=5):
    """pg_resize_bilinear_u8 alone on n cached 1024^2 sources."""
    from pggan_amd.data import device_resize_coeffs
    ent = [sc.entries[p] for p in paths[:n]]
    assert all(e[1:] == [1024, 1024, True] for e in ent)
    so = torch.tensor([e[0] for e in ent], dtype=torch.int64, device="cuda")
    lines = []
    for S in (4, 128, 512):
        dst = torch.empty(n, S, S, 3, dtype=torch.uint8, device="cuda")
        do = torch.arange(n, dtype=torch.int64, device="cuda") * (3 * S * S)
        tab = device_resize_coeffs(1024, S, "cuda")
        ws = None
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        for it in range(warmup + iters):
            if it == warmup:
                ev[0].record()
            ws = ops.resize_u8(sc.buf, so, 1024, 1024, S, tab, tab, dst, do, ws=ws)
        ev[1].record()
        torch.cuda.synchronize()
        us = ev[0].elapsed_time(ev[1]) * 1e3 / iters / n
        lines.append(dict(epoch="kernel", source_px=1024, target_px=S, images_per_call=n, calls=iters,
                          us_per_image=round(us, 2),
                          source_gb_per_s=round(3 * 1024 * 1024 / us / 1e3, 1)))
    return lines


def synth(rng, size):
    y, x = np.mgrid[0:size, 0:size].astype(np.float32) / size
    base = np.stack([x, y, 1.0 - 0.5 * (x + y)], axis=-1)
    a = rng.uniform(0.3, 1.0, size=3).astype(np.float32)
    img = base * a * 200 + rng.normal(0, 6, size=(size, size, 3)).astype(np.float32) + 20
    return np.clip(img, 0, 255).astype(np.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=64)
    ap.add_argument("--workers", type=int, default=16)
    ap.add_argument("--source-cache-gb", type=float, default=0.0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from PIL import Image

    from pggan_amd import _lib
    from pggan_amd.data import BatchLoader, HbmSourceCache, ImageFolderDataset

    ops = _lib.HipOps(torch.bfloat16)
    rng = np.random.default_rng(0)
    lines = []
    with tempfile.TemporaryDirectory() as tmp:
        t0 = time.perf_counter()
        for i in range(a.n):
            Image.fromarray(synth(rng, 1024)).save(os.path.join(tmp, f"{i:04d}.png"))
        write_s = time.perf_counter() - t0
        mb = sum(os.path.getsize(os.path.join(tmp, f)) for f in os.listdir(tmp)) / a.n / 1e6
        # untimed warm-up: the thread pool, the pinned-memory pool and the first launches of
        # the gather / augmentation kernels (~50 ms once per process)
        ds = ImageFolderDataset([tmp], scale_index=STAGES[0][0])
        ld = BatchLoader(ds, "cuda", ops, seed=0, workers=a.workers, cache_bytes=1 << 30)
        for _ in range(2):
            ld.next(list(range(STAGES[0][1])))
        torch.cuda.synchronize()
        ld.close()
        sc = None
        if a.source_cache_gb > 0:
            # fill the source cache as an earlier stage would have (untimed), then warm up the
            # resize kernels of every timed shape
            sc = HbmSourceCache("cuda", int(a.source_cache_gb * (1 << 30)))
            ds = ImageFolderDataset([tmp], scale_index=4)
            ld = BatchLoader(ds, "cuda", ops, seed=0, workers=a.workers, cache_bytes=0, source_cache=sc)
            epoch(ld, a.n // 16, 16)
            ld.close()
            assert len(sc.entries) == a.n and all(e[3] for e in sc.entries.values())
            for stage, B in STAGES:
                ld = BatchLoader(ImageFolderDataset([tmp], scale_index=stage), "cuda", ops, seed=0,
                                 workers=a.workers, cache_bytes=0, source_cache=sc)
                ld.next(list(range(B)))
                torch.cuda.synchronize()
                ld.close()
        for stage, B in STAGES:
            ds = ImageFolderDataset([tmp], scale_index=stage)
            S = ds.size
            assert len(ds) == a.n and a.n % B == 0
            ld = BatchLoader(ds, "cuda", ops, seed=0, workers=a.workers, cache_bytes=8 << 30)
            nb = a.n // B
            for name in ("cold", "warm") + (("cold_source_cache",) if sc is not None else ()):
                if name == "cold_source_cache":
                    # an epoch here is tens of milliseconds: five fresh (cold) loaders, the median
                    runs = []
                    for _ in range(5):
                        ld.close()
                        ld = BatchLoader(ds, "cuda", ops, seed=0, workers=a.workers,
                                         cache_bytes=8 << 30, source_cache=sc)
                        runs.append(epoch(ld, nb, B))
                    dt, out = sorted(runs, key=lambda r: r[0])[2]
                else:
                    dt, out = epoch(ld, nb, B, base=nb if name == "warm" else 0)
                assert out.shape == (B, 3, S, S)
                line = dict(epoch=name, format="png", source_px=1024, target_px=S, stage=stage,
                            batch=B, workers=a.workers, host_cpu_count=os.cpu_count(),
                            omp_num_threads=os.environ.get("OMP_NUM_THREADS"), images=nb * B,
                            seconds=round(dt, 4), img_per_s=round(nb * B / dt, 1),
                            decoded=ld.decoded, cached=ld.cache.used, mean_file_mb=round(mb, 2),
                            write_s=round(write_s, 1))
                if name == "cold_source_cache":
                    line.update(runs_img_per_s=[round(nb * B / r[0], 1) for r in runs],
                                step_img_per_s=STEP_RATE[stage],
                                faster_than_step=bool(nb * B / dt > STEP_RATE[stage]))
                print(json.dumps(line), flush=True)
                lines.append(line)
            ld.close()
        if sc is not None:
            for line in kernel_lines(ops, sc, ImageFolderDataset([tmp]).paths):
                print(json.dumps(line), flush=True)
                lines.append(line)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(lines, f, indent=1)


if __name__ == "__main__":
    main()
