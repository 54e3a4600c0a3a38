"""Times the power-spectrum path (pggan_amd/metrics.py over csrc/spectrum.hip) against the same
profile built from plain torch ops on the GPU and against one read of the images, per DESIGN.md
"Validation: power spectrum".  One feed of --images images at a given resolution (fewer at
1024 with --images-1024): the library call alone ("hip") and through a fresh PowerSpectrum
("feed"); device events around each part, a warm-up, then the median of --runs repetitions.

    python tools/spectrum_bench.py --res 128 512 1024 [--images 64] [--runs 12] [--json out.json]

Baselines.  "torch": quantise, luma, torch.fft.rfft2, abs()^2, the half-plane weights, one
index_add_ into the bins -- it writes and re-reads the complex half spectrum; nothing in it is
tuned.  "read": torch.sum over the batch, one pass over the bytes the kernel has to read."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

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
def torch_tables(R, dev):
    """(bin of every point of the rfft2 half plane, bins > K sent to K + 1; its weights)."""
    K = R // 2
    bins = np.minimum(metrics.spectrum_bins(R)[:, :K + 1], K + 1).ravel()
    w = np.full(K + 1, 2.0, np.float32)
    w[0] = w[K] = 1.0
    return torch.from_numpy(bins).to(dev), torch.from_numpy(w).to(dev)


def torch_profile(x, bins, w):
    """x [B,3,R,R] in [-1,1] -> prof [B, K + 1]."""
    B, R = x.shape[0], x.shape[-1]
    q = torch.round(torch.clamp(x * 127.5 + 127.5, 0, 255)) - 127.5
    y = 0.299 * q[:, 0] + 0.587 * q[:, 1] + 0.114 * q[:, 2]
    f = torch.fft.rfft2(y)
    p = (f.abs() ** 2 * w).reshape(B, -1)
    out = torch.zeros(B, R // 2 + 2, device=x.device)
    out.index_add_(1, bins, p)
    return out[:, :R // 2 + 1]


# ------------------------------------------------------------------ one resolution
def bench(R, B, runs):
    dev = torch.device("cuda")
    ops = _lib.HipOps(torch.float32)
    g = torch.Generator(device=dev).manual_seed(R)
    x = torch.randint(0, 256, (B, 3, R, R), device=dev, generator=g).float() / 127.5 - 1
    res = {"resolution": R, "images": B}

    out = torch.empty(B, R // 2 + 1, device=dev)

    def hip():                  # the library call: what a feed costs on the device
        ops.spectrum_profile(x, True, out)
        return out

    def feed():                 # the same through the metric: a fresh PowerSpectrum, one feed
        m = metrics.PowerSpectrum(ops, R)
        m.feed(x)
        return m.per_image()

    bins, w = torch_tables(R, dev)
    nbytes = x.numel() * 4
    res["workspace_MB"] = int(ops.lib.pg_spectrum_workspace_bytes(B, R)) / 2 ** 20
    res["hip_ms"], res["hip_min_ms"] = timed(hip, runs)
    res["feed_ms"], _ = timed(feed, runs)
    res["torch_ms"], res["torch_min_ms"] = timed(lambda: torch_profile(x, bins, w), runs)
    res["read_ms"], res["read_min_ms"] = timed(lambda: torch.sum(x), runs)
    res["hip_GBps"] = nbytes / (res["hip_ms"] * 1e-3) / 1e9
    res["read_GBps"] = nbytes / (res["read_ms"] * 1e-3) / 1e9
    res["hip_over_read"] = res["hip_ms"] / res["read_ms"]
    res["torch_over_hip"] = res["torch_ms"] / res["hip_ms"]
    # the two pipelines compute the same thing (bin 0 apart: one point, the little that the
    # shift by 127.5 leaves of a uniform image's mean)
    a, b, c = hip().double(), torch_profile(x, bins, w).double(), feed().double()
    assert torch.equal(a, c)
    d = (a - b).abs() / b
    res["max_rel_diff_bin0"], res["max_rel_diff"] = float(d[:, 0].max()), float(d[:, 1:].max())
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, nargs="+", default=[128, 512, 1024])
    ap.add_argument("--images", type=int, default=64)
    ap.add_argument("--images-1024", type=int, default=None,
                    help="images at 1024 x 1024 (default: --images)")
    ap.add_argument("--runs", type=int, default=12)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("spectrum_bench: needs a GPU (timings on a CPU would say nothing)")
    if a.runs < 10:
        raise SystemExit("spectrum_bench: --runs must be >= 10")
    out = []
    for R in a.res:
        r = bench(R, a.images_1024 if R == 1024 and a.images_1024 else a.images, a.runs)
        out.append(r)
        print(json.dumps(r), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
