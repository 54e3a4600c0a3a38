"""Times the MS-SSIM path (pggan_amd/metrics.py over csrc/msssim.hip) against the same metric
written with plain torch ops on the GPU, per DESIGN.md "Validation: MS-SSIM".  One feed of
--pairs pairs (five scales) plus the combine at a given resolution; device events around each
part, a warm-up, then the median of --runs repetitions.  In the same call it times
pg_swd_pyr_down level 0 on the same images: the yardstick for a filter that stages its input
in LDS and reads it once on this chip.

    python tools/msssim_bench.py --res 256 1024 [--pairs 32] [--runs 12] [--json out.json]

Baseline ("torch"): per scale ten F.conv2d calls with groups=3 (the 11x11 window on x, y and
the materialised x^2, y^2, xy), the two ratios, their means, F.avg_pool2d for the next scale.
Nothing in it is tuned."""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from pggan_amd import _lib, metrics  # noqa: E402

C1, C2 = (0.01 * 255) ** 2, (0.03 * 255) ** 2
WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)


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
def torch_msssim(x, taps):
    """x [2P,3,R,R] in [-1,1] -> pair values [P]."""
    x = torch.round(torch.clamp(x * 127.5 + 127.5, 0, 255))
    a, b = x[0::2], x[1::2]
    v = None
    for s, g in enumerate(taps):
        g = torch.as_tensor(g, device=x.device)
        w = torch.outer(g, g).expand(3, 1, len(g), len(g)).contiguous()
        f = lambda t: F.conv2d(t, w, groups=3)
        mu1, mu2 = f(a), f(b)
        s11, s22, s12 = f(a * a) - mu1 * mu1, f(b * b) - mu2 * mu2, f(a * b) - mu1 * mu2
        cs = (2 * s12 + C2) / (s11 + s22 + C2)
        if s + 1 < len(taps):
            m = cs.mean(dim=(1, 2, 3))
            a, b = F.avg_pool2d(a, 2), F.avg_pool2d(b, 2)
        else:
            m = ((2 * mu1 * mu2 + C1) / (mu1 * mu1 + mu2 * mu2 + C1) * cs).mean(dim=(1, 2, 3))
        m = m.clamp_min(0) ** WEIGHTS[s]
        v = m if v is None else v * m
    return v


# ------------------------------------------------------------------ one resolution
def bench(R, P, runs):
    dev = torch.device("cuda")
    ops = _lib.HipOps(torch.float32)
    g = torch.Generator(device=dev).manual_seed(R)
    # on the 8-bit grid (what decoded reals are); each pair a noisy copy, so the values are not 0
    a = torch.randint(32, 224, (P, 3, R, R), device=dev, generator=g).float()
    b = torch.clamp(a + torch.randint(-24, 25, a.shape, device=dev, generator=g).float(), 0, 255)
    x = torch.stack([a, b], dim=1).reshape(2 * P, 3, R, R) / 127.5 - 1
    res = {"resolution": R, "pairs": P}

    def hip_all():
        m = metrics.MultiScaleSSIM(ops, R, P)
        m._pool = pool
        m.feed(x)
        return m.values()

    warm = metrics.MultiScaleSSIM(ops, R, P)
    warm.feed(x)
    pool, taps = warm._pool, warm.taps
    res["hip_ms"], _ = timed(hip_all, runs)
    sums = torch.empty(P, 2, device=dev)
    t, _ = timed(lambda: ops.msssim_scale(x[0::2], x[1::2], taps[0], True, sums, pool[0][0, :P],
                                          pool[0][1, :P]), runs)
    nbytes = 2 * P * 3 * R * R * 4 * 1.25          # both sides read once, both pooled sides written
    res["hip_scale0_ms"], res["hip_scale0_GBps"] = t, nbytes / (t * 1e-3) / 1e9
    y = torch.empty(2 * P, 3, R // 2, R // 2, device=dev)
    t, _ = timed(lambda: ops.swd_pyr_down(x, y, True), runs)
    res["pyr_down0_ms"], res["pyr_down0_GBps"] = t, nbytes / (t * 1e-3) / 1e9
    res["scale0_vs_pyr_down0"] = res["hip_scale0_GBps"] / res["pyr_down0_GBps"]
    res["torch_ms"], _ = timed(lambda: torch_msssim(x, taps), runs)
    res["speedup"] = res["torch_ms"] / res["hip_ms"]
    # the two pipelines compute the same thing
    res["max_value_diff"] = float((hip_all() - torch_msssim(x, taps)).abs().max())
    res["mean_value"] = float(hip_all().double().mean())
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, nargs="+", default=[256, 1024])
    ap.add_argument("--pairs", type=int, default=32)
    ap.add_argument("--runs", type=int, default=12)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("msssim_bench: needs a GPU (timings on a CPU would say nothing)")
    if a.runs < 10:
        raise SystemExit("msssim_bench: --runs must be >= 10")
    out = []
    for R in a.res:
        r = bench(R, a.pairs, a.runs)
        out.append(r)
        print(json.dumps(r), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
