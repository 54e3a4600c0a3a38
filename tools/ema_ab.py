"""What the generator's weight average (config ema_decay) costs, measured in one process (GPU box).

  python tools/ema_ab.py [--stage 8 --batch 4 --dtype bf16 --decay 0.999 --rounds 6 --steps 10]

Two ProgressiveGAN models built like bench.py's (paper depths, resident synthetic batch, the
C++-replayed step), one with the average off and one with it on, stepped alternately: `steps`
train_steps per timing under HIP events, `rounds` timings each; printed: median and minimum
ms/step of both.  Then the Adam_G launch alone over G's live range, alternating three forms:
adam_dev (off), adam_dev_ema (the fused update the product runs) and adam_dev followed by a
separate lerp_ launch (what a Python-side average would cost at best), median and minimum us.
bench.py has no switch for the key, hence this script; its off line is bench.py's step."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PAPER_DEPTHS = [512, 512, 512, 512, 256, 128, 64, 32, 16]


def build(a, decay):
    from pggan_amd.config import Config
    from pggan_amd.model import ProgressiveGAN
    cfg = Config.from_yaml(os.path.join(ROOT, "pggan_amd", "default_config.yaml"))
    cfg.update(depths=list(PAPER_DEPTHS), batch_per_gpu=a.batch, compute_dtype=a.dtype,
               synthetic_data=True, isMaster=False, use_mGPU=False, gpu_num=1, run_id="ema_ab",
               ema_decay=decay)
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


def timed(fn, n):
    """Milliseconds per call of fn over n calls, between two events on the current stream."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / n


def report(name, xs, unit):
    print(f"{name:28s} median {statistics.median(xs):9.3f} min {min(xs):9.3f} {unit}  "
          f"({len(xs)} timings)", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--stage", type=int, default=8)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--dtype", choices=["bf16", "f32"], default="bf16")
    ap.add_argument("--decay", type=float, default=0.999)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--steps", type=int, default=10)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    torch.cuda.set_device(0)
    models = {"off": build(a, None), "on": build(a, a.decay)}
    for m in models.values():          # two host-enqueued steps, one recorded, two replayed
        for _ in range(5):
            m.train_step()
        m.flush()
    torch.cuda.synchronize()
    assert all(m.graph_replays >= 2 for m in models.values())
    assert len(models["on"]._gstate["rec"]) == len(models["off"]._gstate["rec"])
    for buf in ("flat", "m", "v"):     # the average leaves training as it is
        assert torch.equal(getattr(models["on"].fpG, buf), getattr(models["off"].fpG, buf)), buf
    t = {k: [] for k in models}
    for _ in range(a.rounds):
        for k, m in models.items():
            def steps(m=m):
                m.train_step()
            t[k].append(timed(steps, a.steps))
            m.flush()
    print(f"stage {a.stage} batch {a.batch} {a.dtype}, decay {a.decay}: "
          f"{len(models['on']._gstate['rec'])} launches per step in both")
    for k in models:
        report(f"step, average {k}", t[k], "ms/step")
    d = statistics.median(t["on"]) / statistics.median(t["off"]) - 1
    print(f"on vs off (medians): {100 * d:+.2f} %")

    # Adam_G alone, on G's own buffers (the values are scratch from here on)
    fp, hp = models["on"].fpG, models["on"].hyper
    ops = next(iter(models["on"]._engines.values())).ops
    n = fp.n_live
    fp.grad.normal_()
    kw = dict(lr=hp.lr_G, beta1=hp.beta1, beta2=hp.beta2, eps=hp.eps, step_dev=fp.step_dev)
    c = 1.0 - a.decay

    def plain():
        ops.adam_dev(fp.flat[:n], fp.grad[:n], fp.m[:n], fp.v[:n], **kw)

    def fused():
        ops.adam_dev_ema(fp.flat[:n], fp.grad[:n], fp.m[:n], fp.v[:n], fp.ema[:n],
                         decay=a.decay, **kw)

    def separate():
        plain()
        fp.ema[:n].lerp_(fp.flat[:n], c)

    forms = {"adam_dev": plain, "adam_dev_ema (fused)": fused, "adam_dev + lerp_": separate}
    for f in forms.values():
        timed(f, 5)
    kt = {k: [] for k in forms}
    for _ in range(max(a.rounds, 10)):
        for k, f in forms.items():
            kt[k].append(1e3 * timed(f, 20))
    print(f"Adam_G over {n} live parameters ({n * 4 / 2 ** 20:.1f} MiB per buffer):")
    for k in forms:
        report(k, kt[k], "us")


if __name__ == "__main__":
    main()
