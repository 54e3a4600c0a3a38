"""What training health (config health_cycle; pggan_amd/health.py over csrc/health.hip) costs,
measured in one process on the GPU, per DESIGN.md "Training health".

    python tools/health_bench.py [--stage 8 --batch 4 --dtype bf16 --runs 20 --rounds 6 --steps 10]
                                 [--json profiles/health_bench.json]

1. The kernels on the flat buffers of the benchmark model (paper depths, stage 8), both nets:
   pg_tensor_stats over p, g, m, v and pg_nonfinite_watch over m, each against the same
   quantities from torch ops -- torch._foreach_norm on the views, isfinite counts and the Adam
   formula ("torch") -- and against one read of the same bytes (torch.sum, "read").  Device
   events, a warm-up, the median of --runs repetitions.
2. train_step img/s of two models built like bench.py's, health off and on (the probe every
   step; health_cycle beyond the run, so no report falls into a timing), stepped alternately
   as tools/ab.sh alternates its variants.  train_step itself is the code of the commit before
   the feature (health() is a call after it), so the off line is that commit's step."""
import argparse
import json
import math
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PAPER_DEPTHS = [512, 512, 512, 512, 256, 128, 64, 32, 16]


def build(a, cycle):
    from pggan_amd.config import Config
    from pggan_amd.model import ProgressiveGAN
    cfg = Config.from_yaml(os.path.join(ROOT, "pggan_amd", "default_config.yaml"))
    cfg.update(depths=list(PAPER_DEPTHS), batch_per_gpu=a.batch, compute_dtype=a.dtype,
               synthetic_data=True, isMaster=False, use_mGPU=False, gpu_num=1, run_id="health_bench",
               health_cycle=cycle, health_on_bad="warn")
    torch.manual_seed(1234)
    m = ProgressiveGAN(cfg, 0)
    m.initialize_models()
    for i in range(1, a.stage + 1):
        m.G.add_block(PAPER_DEPTHS[i])
        m.D.add_block(PAPER_DEPTHS[i])
    m.scale_index = a.stage
    m.G.alpha = m.D.alpha = 1.0
    m.set_optimizers()
    m.set_dataset()
    m.set_data_iterator()
    m.set_loss_collector()
    return m


def timed(fn, runs, warm=3):
    """Median / min device time of fn() in ms (events on the current stream)."""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return statistics.median(ts), min(ts)


def kernels(m, runs):
    from pggan_amd import health as H
    ops = m._health.ops
    nets = []
    for w, fp, lr in (("G", m.fpG, m.opt_G.lr), ("D", m.fpD, m.opt_D.lr)):
        net = H._Net(w, fp, m.device)
        n = net.n
        gen = torch.Generator(device=m.device).manual_seed(len(nets))
        fp.grad.normal_(generator=gen)
        fp.m.normal_(generator=gen).mul_(1e-3)
        fp.v.normal_(generator=gen).square_().mul_(1e-6)
        views = {b: [fp._view(t, k) for k in net.names]
                 for b, t in (("p", fp.flat), ("g", fp.grad), ("m", fp.m), ("v", fp.v))}
        nets.append(dict(net=net, fp=fp, n=n, views=views, pair=ops.adam_pair(lr, 0.0, 0.99, 10),
                         out=torch.zeros(len(net.names), 10, dtype=torch.float64, device=m.device),
                         lat=torch.zeros(len(net.names), dtype=torch.int32, device=m.device)))
    live = sum(sum(x["net"].numel) for x in nets)
    res = {"live_floats": {x["net"].which: sum(x["net"].numel) for x in nets},
           "tensors": {x["net"].which: len(x["net"].names) for x in nets},
           "stats_bytes": 16 * live, "watch_bytes": 4 * live, "chunk": ops.tensor_stats_chunk}
    eps = m.hyper.eps

    def stats():
        for x in nets:
            fp, n = x["fp"], x["n"]
            ops.tensor_stats(x["net"].table, fp.flat[:n], fp.grad[:n], fp.m[:n], fp.v[:n],
                             step_size=x["pair"][0], bc2_sqrt=x["pair"][1], eps=eps, out=x["out"])

    def watch():
        for x in nets:
            ops.nonfinite_watch(x["net"].table, x["fp"].m[:x["n"]], 1, x["lat"])

    def torch_stats():      # norms and maxima per tensor, non-finite counts, the update's norm
        keep = []
        for x in nets:
            v = x["views"]
            keep += [torch._foreach_norm(v["p"]), torch._foreach_norm(v["g"]),
                     torch._foreach_norm(v["p"], float("inf")), torch._foreach_norm(v["g"], float("inf"))]
            u = torch._foreach_div(v["m"], torch._foreach_add(
                torch._foreach_div(torch._foreach_sqrt(v["v"]), x["pair"][1]), eps))
            keep += [torch._foreach_norm(u), torch._foreach_norm(u, float("inf"))]
            fp, n = x["fp"], x["n"]
            keep += [(~torch.isfinite(t[:n])).sum() for t in (fp.flat, fp.grad, fp.m, fp.v)]
        return keep

    def torch_watch():
        return [torch.isfinite(x["fp"].m[:x["n"]]).all() for x in nets]

    def read_stats():
        return [t[:x["n"]].sum() for x in nets for t in (x["fp"].flat, x["fp"].grad, x["fp"].m, x["fp"].v)]

    def read_watch():
        return [x["fp"].m[:x["n"]].sum() for x in nets]

    for name, fn in (("stats", stats), ("watch", watch), ("torch_stats", torch_stats),
                     ("torch_watch", torch_watch), ("read_stats", read_stats), ("read_watch", read_watch)):
        res[name + "_ms"], res[name + "_min_ms"] = timed(fn, runs)
    res["stats_GBps"] = res["stats_bytes"] / (res["stats_ms"] * 1e-3) / 1e9
    res["watch_GBps"] = res["watch_bytes"] / (res["watch_ms"] * 1e-3) / 1e9
    for k in ("stats", "watch"):
        res[k + "_over_read"] = res[k + "_ms"] / res[f"read_{k}_ms"]
        res[f"torch_over_{k}"] = res[f"torch_{k}_ms"] / res[k + "_ms"]
    # the two pipelines agree (fp32 norms against double sums)
    stats()
    for x in nets:
        want = torch.stack(torch._foreach_norm(x["views"]["g"])).double()
        got = x["out"][:, 1].sqrt()
        assert float(((got - want).abs() / want).max()) < 1e-4
        assert not x["lat"].any() and not x["out"][:, 6:].any()
    return res


def steps(a):
    models = {"off": build(a, None), "on": build(a, 10 ** 9)}
    count = {k: 0 for k in models}

    def run(k, n):
        m = models[k]
        for _ in range(n):
            m.train_step()
            count[k] += 1
            m.health(count[k])          # None at once with the key blank
    for k in models:
        run(k, 5)
    torch.cuda.synchronize()
    assert all(m.graph_replays >= 2 for m in models.values())
    for buf in ("flat", "m", "v"):
        assert torch.equal(getattr(models["on"].fpD, buf), getattr(models["off"].fpD, buf)), buf
    t = {k: [] for k in models}
    for _ in range(a.rounds):
        for k in models:
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            run(k, a.steps)
            e1.record()
            e1.synchronize()
            t[k].append(e0.elapsed_time(e1) / a.steps)
    res = {"stage": a.stage, "batch": a.batch, "dtype": a.dtype, "rounds": a.rounds, "steps": a.steps}
    for k in models:
        med = statistics.median(t[k])
        res[f"step_{k}_ms"], res[f"step_{k}_min_ms"] = med, min(t[k])
        res[f"step_{k}_img_s"] = a.batch / (med * 1e-3)
        res[f"step_{k}_spread_pct"] = 100 * (max(t[k]) - min(t[k])) / med
    res["on_vs_off_pct"] = 100 * (res["step_on_ms"] / res["step_off_ms"] - 1)
    return res, models["on"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--stage", type=int, default=8)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--dtype", choices=["bf16", "f32"], default="bf16")
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("health_bench: needs a GPU (timings on a CPU would say nothing)")
    torch.cuda.set_device(0)
    step_res, m = steps(a)
    print(json.dumps(step_res), flush=True)
    kern = kernels(m, a.runs)               # scribbles on the model's gradients and moments: last
    print(json.dumps(kern), flush=True)
    assert math.isfinite(kern["stats_ms"])
    if a.json:
        with open(a.json, "w") as f:
            json.dump({"step": step_res, "kernels": kern}, f, indent=1)


if __name__ == "__main__":
    main()
