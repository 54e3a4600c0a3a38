"""Times the sliced Wasserstein path (pggan_amd/metrics.py over csrc/swd.hip) against the same
pipeline written with plain torch ops on the GPU, per DESIGN.md "Validation: sliced Wasserstein
distance".  One 64-image feed (Gaussian pyramid + descriptors of every level) plus one level of
result() (statistics, projections, sort, L1) at a given resolution; device events around each
part, a warm-up, then the median of --runs repetitions.  The host-side draw of the patch
centres is timed separately (host clock): it is not device work.

    python tools/swd_bench.py --res 256 1024 [--images 64] [--runs 12] [--json out.json]

Baseline ("torch"): F.conv2d on reflect-padded input for both filters (stride 2 down, zero
insert + 4 k(x)k up), the full-resolution Laplacian materialised, an advanced-index gather,
mean / std, matmul, torch.sort, mean |a - b|.  Nothing in it is tuned."""
import argparse
import json
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from pggan_amd import _lib, metrics  # noqa: E402


def timed(fn, runs, warm=3):
    """Median / min device time of fn() in ms (events on the current stream)."""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return statistics.median(ts), min(ts)


# ------------------------------------------------------------------ the torch baseline
def _kernel(dev, scale=1.0):
    k = torch.tensor([1.0, 4.0, 6.0, 4.0, 1.0], device=dev) / 16
    return (torch.outer(k, k) * scale).expand(3, 1, 5, 5).contiguous()


def torch_pyramid(x, sizes):
    g = [torch.round(torch.clamp(x * 127.5 + 127.5, 0, 255))]
    w = _kernel(x.device)
    for _ in sizes[1:]:
        g.append(F.conv2d(F.pad(g[-1], (2, 2, 2, 2), mode="reflect"), w, stride=2, groups=3))
    return g


def torch_descriptors(g, pos, K):
    w4 = _kernel(g[0].device, 4.0)
    out = []
    dy = torch.arange(-3, 4, device=g[0].device)
    for l, gl in enumerate(g):
        lap = gl
        if l + 1 < len(g):
            z = torch.zeros_like(gl)
            z[..., ::2, ::2] = g[l + 1]
            lap = gl - F.conv2d(F.pad(z, (2, 2, 2, 2), mode="reflect"), w4, groups=3)
        p = pos[l].long().view(gl.shape[0], K, 2)
        b = torch.arange(gl.shape[0], device=gl.device).view(-1, 1, 1, 1, 1)
        c = torch.arange(3, device=gl.device).view(1, 1, 3, 1, 1)
        yy = (p[..., 0].view(-1, K, 1, 1, 1) + dy.view(1, 1, 1, 7, 1))
        xx = (p[..., 1].view(-1, K, 1, 1, 1) + dy.view(1, 1, 1, 1, 7))
        out.append(lap[b, c, yy, xx].reshape(-1, 147))
    return out


def torch_level(da, db, dirs):
    def norm(d):
        d = d.view(-1, 3, 49)
        return ((d - d.mean(dim=(0, 2), keepdim=True)) / d.std(dim=(0, 2), unbiased=False,
                                                               keepdim=True)).view(-1, 147)
    a, b = norm(da), norm(db)
    tot = 0.0
    for d in dirs:
        pa, pb = torch.sort((a @ d).t().contiguous(), dim=1).values, \
            torch.sort((b @ d).t().contiguous(), dim=1).values
        tot = tot + (pa - pb).abs().mean()
    return tot / len(dirs) * 1e3


# ------------------------------------------------------------------ one resolution
def bench(R, B, runs, K=128):
    dev = torch.device("cuda")
    ops = _lib.HipOps(torch.float32)
    g = torch.Generator(device=dev).manual_seed(R)
    # on the 8-bit grid (what decoded reals are), so that no rounding tie separates the two
    # pipelines and their descriptors can be compared
    u8 = lambda lo, hi: torch.randint(lo, hi, (B, 3, R, R), device=dev, generator=g).float() / 127.5 - 1
    real, fake = u8(0, 256), u8(32, 224)
    m = metrics.SlicedWasserstein(ops, R, B, per_image=K)
    m.feed("real", real)
    m.feed("fake", fake)
    sizes, nl = m.sizes, len(m.sizes)
    res = {"resolution": R, "images": B, "per_image": K, "levels": nl}

    t0 = time.perf_counter()
    pos = [metrics.draw_positions(0, l, 0, B, s, K).to(dev) for l, s in enumerate(sizes)]
    torch.cuda.synchronize()
    res["host_positions_ms"] = (time.perf_counter() - t0) * 1e3

    pyr = [real] + list(m._pyr)
    desc = [m.desc["real"][l] for l in range(nl)]

    def hip_pyr():
        for l in range(nl - 1):
            ops.swd_pyr_down(pyr[l], pyr[l + 1], l == 0)

    def hip_desc():
        for l in range(nl):
            ops.swd_descriptors(pyr[l], pyr[l + 1] if l + 1 < nl else None, pos[l], desc[l], K, l == 0)

    def hip_level():            # what result() does for one level
        n = B * K
        for k, w in enumerate(metrics.SETS):
            ops.swd_stats(m.desc[w][0], stat[2 * k], stat[2 * k + 1])
        for r in range(m.repeats):
            for k, w in enumerate(metrics.SETS):
                ops.swd_project(m.desc[w][0], stat[2 * k], stat[2 * k + 1], m.dirs[r], proj[k])
            a, b = (torch.sort(t, dim=1).values for t in proj)
            ops.swd_l1(a, b, n, acc)

    stat = torch.empty(4, 3, device=dev)
    proj = [torch.empty(m.P, B * K, device=dev) for _ in range(2)]
    acc = torch.zeros(1, device=dev)
    res["hip_pyramid_ms"], _ = timed(hip_pyr, runs)
    res["hip_descriptors_ms"], _ = timed(hip_desc, runs)
    res["hip_level_ms"], _ = timed(hip_level, runs)
    res["hip_feed_plus_level_ms"], _ = timed(lambda: (hip_pyr(), hip_desc(), hip_level()), runs)
    # the first pyramid step alone: one read of the level-0 images, one write of level 1
    t, tmin = timed(lambda: ops.swd_pyr_down(pyr[0], pyr[1], True), runs) if nl > 1 else (0.0, 0.0)
    if nl > 1:
        nbytes = B * 3 * R * R * 4 * 1.25
        res["pyr_down0_ms"], res["pyr_down0_GBps"] = t, nbytes / (t * 1e-3) / 1e9

    fake_desc = torch_descriptors(torch_pyramid(fake, sizes), pos, K)[0]

    def t_pyr():
        return torch_pyramid(real, sizes)

    gp = t_pyr()
    res["torch_pyramid_ms"], _ = timed(t_pyr, runs)
    res["torch_descriptors_ms"], _ = timed(lambda: torch_descriptors(gp, pos, K), runs)
    td = torch_descriptors(gp, pos, K)
    res["torch_level_ms"], _ = timed(lambda: torch_level(td[0], fake_desc, m.dirs), runs)
    res["torch_feed_plus_level_ms"], _ = timed(
        lambda: torch_level(torch_descriptors(t_pyr(), pos, K)[0], fake_desc, m.dirs), runs)
    # the two pipelines compute the same thing
    hip_pyr(), hip_desc()
    torch.cuda.synchronize()
    res["max_desc_diff"] = max(float((desc[l] - td[l]).abs().max()) for l in range(nl))
    res["speedup_feed_plus_level"] = res["torch_feed_plus_level_ms"] / res["hip_feed_plus_level_ms"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, nargs="+", default=[256, 1024])
    ap.add_argument("--images", type=int, default=64)
    ap.add_argument("--runs", type=int, default=12)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("swd_bench: needs a GPU (timings on a CPU would say nothing)")
    if a.runs < 10:
        raise SystemExit("swd_bench: --runs must be >= 10")
    out = []
    for R in a.res:
        r = bench(R, a.images, a.runs)
        out.append(r)
        print(json.dumps(r), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
