"""Training health (config `health_cycle`): per-tensor norms of parameters, gradients and Adam
updates over the run, a record of which tensor went non-finite first and at which step, and a
checkpoint that is never overwritten by a diverged run.  One `Health` per model; everything is
off, and launches nothing, unless `health_cycle` is set.  DESIGN.md "Training health".

Every call of run(step) (ProgressiveGAN.health, after train_step, on every rank) launches the
non-finite probe (pg_nonfinite_watch) on each net's first Adam moment `m`, tagged with the
net's count of Adam updates, on the weight average and on the engine's loss scalars: nothing is
read back.  Every `health_cycle`-th call is the full report: flush(), pg_tensor_stats on p, g,
m, v of both nets, one read-back of the statistics and of the latches, health.csv, a summary
line on the master, and -- when anything is non-finite -- TrainingDiverged (`health_on_bad:
stop`, the default) or a warning (`warn`).

Per net and stage the module owns a segment table built from FlatParams: the live names in
flat order with their offsets and true element counts (not the padded spans), and the
`first_bad` latches, zeroed when the table is rebuilt (reset_solver makes new FlatParams)."""
from __future__ import annotations

import math
import os

import numpy as np
import torch

from .config import cfg_get
from .validation import append_csv

COLS = ("sumsq_p", "sumsq_g", "sumsq_u", "maxabs_p", "maxabs_g", "maxabs_u",
        "bad_p", "bad_g", "bad_m", "bad_v")
CSV_HEADER = "step,scale,net,name,numel,rms_p,rms_g,rms_u,ratio,max_p,max_g,bad,first_bad_step"
ROW_KEYS = tuple(CSV_HEADER.split(","))
N_LOSS = 5                      # the engine's device loss scalars (StepEngine.loss[:5])


class TrainingDiverged(RuntimeError):
    """A non-finite value in the training state.  `net` ("G", "D" or "loss"), `name` (the
    tensor), `buffer` ("p", "g", "m", "v", "ema" or "loss") and `step` (the first bad global
    step) are those of the earliest finding; `findings` holds them all."""

    def __init__(self, findings):
        self.findings = list(findings)
        f = self.findings[0]
        self.net, self.name, self.buffer, self.step = f["net"], f["name"], f["buffer"], f["step"]
        super().__init__(describe(self.findings))


def describe(findings):
    """The text of a finding list: the earliest first, the rest counted."""
    f = findings[0]
    text = (f"non-finite values in {f['net']} {f['name']} buffer {f['buffer']} "
            f"({f['count']} element{'s' if f['count'] != 1 else ''}), first bad step {f['step']}")
    if len(findings) > 1:
        text += f" (+{len(findings) - 1} more finding{'s' if len(findings) > 2 else ''})"
    return text


class Settings:
    """The health keys of the config, read and checked once: `health_cycle` (blank: off;
    N >= 1: the full report every N steps) and `health_on_bad` (blank: stop; or warn)."""

    def __init__(self, args):
        c = cfg_get(args, "health_cycle", None)
        if isinstance(c, bool) or not isinstance(c, (int, str)) or \
                (isinstance(c, str) and not c.strip().isdigit()) or int(c) < 1:
            raise ValueError(f"health_cycle: must be an integer >= 1, or blank for off, got {c!r}")
        self.cycle = int(c)
        b = cfg_get(args, "health_on_bad", None)
        b = "stop" if b in (None, "") else b
        if b not in ("stop", "warn"):
            raise ValueError(f"health_on_bad: must be stop or warn (blank: stop), got {b!r}")
        self.on_bad = b


def segment_table(fp):
    """(names, offsets, counts) of a FlatParams' live tensors in flat order: fp.offsets[n] and
    the true element count prod(shapes[n]), not the padded span."""
    names = [n for n in fp.offsets if n not in fp.dead]
    return (names, [int(fp.offsets[n]) for n in names],
            [int(math.prod(fp.shapes[n])) for n in names])


def adam_pair(ops, lr, beta1, beta2, t):
    """{lr / (1 - beta1^t), sqrt(1 - beta2^t)} of Adam update t as the op set applies it."""
    return ops.adam_pair(lr, beta1, beta2, max(int(t), 1))


class _Net:
    """One net's segment table on the device, its latch slots and the host's record of the
    global step at which each update count was first seen."""

    def __init__(self, which, fp, device):
        self.which, self.fp = which, fp
        self.names, offs, self.numel = segment_table(fp)
        self.table = torch.tensor(list(zip(offs, self.numel)), dtype=torch.int64,
                                  device=device).reshape(-1, 2).contiguous()
        self.n = int(fp.n_live)
        self.seen = {}          # update count -> the step of the run() that first saw it
        self.first = {}         # (name, buffer) -> first bad global step, once reported

    def see(self, step):
        self.seen.setdefault(self.fp.step, step)

    def step_of(self, tag, step):
        """The global step of the update with count `tag`: the call that first saw that count;
        for a count no call of this report period saw, step - (fp.step - tag)."""
        return self.seen.get(tag, step - (self.fp.step - tag))


class Health:
    def __init__(self, model):
        self.model = model
        self._ops = None
        self._nets = None
        self.settings = None
        self.configure()

    def configure(self):
        """Read the config again: the settings, or None with `health_cycle` blank."""
        self.settings = None
        c = cfg_get(self.model.args, "health_cycle", None)
        if c is not None and c != "":
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
        """reset_solver: the flat buffers are replaced; tables and latches start over."""
        self._nets = None

    # ------------------------------------------------------------------ tables
    def _bind(self):
        """The tables of the model's current FlatParams; new ones (and zeroed latches) when
        the buffers were replaced."""
        m = self.model
        nets = self._nets
        if nets is not None and nets["G"].fp is m.fpG and nets["D"].fp is m.fpD and \
                (nets["ema"] is not None) == (m.fpG.ema is not None):
            return nets
        G, D = _Net("G", m.fpG, m.device), _Net("D", m.fpD, m.device)
        ema = m.fpG.ema is not None
        nG, nD = len(G.names), len(D.names)
        # one latch buffer: m of G, m of D, the loss scalars, the weight average
        lat = torch.zeros(nG + nD + 1 + (nG if ema else 0), dtype=torch.int32, device=m.device)
        out = torch.zeros(nG + nD, len(COLS), dtype=torch.float64, device=m.device)
        self._nets = nets = {
            "G": G, "D": D, "latch": lat, "out": out,
            "lat_G": lat[:nG], "lat_D": lat[nG:nG + nD], "lat_loss": lat[nG + nD:nG + nD + 1],
            "ema": lat[nG + nD + 1:] if ema else None,
            "out_G": out[:nG], "out_D": out[nG:],
            "loss_table": torch.tensor([[0, N_LOSS]], dtype=torch.int64, device=m.device),
            "loss_first": None}
        return nets

    def _engine_loss(self):
        for eng in self.model._engines.values():
            return eng.loss
        return None

    def _watch(self, nets, step):
        """The every-step probe: one launch per watched buffer, nothing read back."""
        ops = self.ops
        for w in ("G", "D"):
            net = nets[w]
            fp = net.fp
            if fp.step < 1:              # no update yet: m is all zeros
                continue
            net.see(step)
            ops.nonfinite_watch(net.table, fp.m[:net.n], fp.step, nets["lat_" + w])
            if w == "G" and nets["ema"] is not None:
                ops.nonfinite_watch(net.table, fp.ema[:net.n], fp.step, nets["ema"])
        loss = self._engine_loss()
        if loss is not None:
            ops.nonfinite_watch(nets["loss_table"], loss, step + 1, nets["lat_loss"])

    def _stats(self, nets, w, g_buffer=None):
        """pg_tensor_stats of net w into its rows of `out`; g_buffer: what rides in the
        gradient's place (save_checkpoint counts the weight average there)."""
        m = self.model
        net = nets[w]
        fp, hp = net.fp, m.hyper
        lr = m.opt_G.lr if w == "G" else m.opt_D.lr
        step_size, bc2_sqrt = adam_pair(self.ops, lr, hp.beta1, hp.beta2, fp.step)
        g = fp.grad if g_buffer is None else g_buffer
        self.ops.tensor_stats(net.table, fp.flat[:net.n], g[:net.n], fp.m[:net.n], fp.v[:net.n],
                              step_size=step_size, bc2_sqrt=bc2_sqrt, eps=hp.eps,
                              out=nets["out_" + w])

    # ------------------------------------------------------------------ the call
    def run(self, step):
        """ProgressiveGAN.health: None when off; the probe every call; on every
        `health_cycle`-th step the report dict (see report)."""
        s = self.settings
        if s is None:
            return None
        nets = self._bind()
        self._watch(nets, step)
        if step % s.cycle:
            return {"step": step, "report": False}
        return self.report(step)

    def report(self, step):
        """The full report at `step`:
          {"step", "scale", "report": True,
           "rows": one dict per live tensor with the keys of health.csv,
           "stats": {"G" / "D": float64 [tensors, 10] in the order of COLS},
           "grad_rms": {"G", "D"}, "worst": (net, name, ratio) with the largest rms_u / rms_p,
           "findings": [{"net", "name", "buffer", "count", "step"}], earliest first}
        health.csv and the printed line are the master's; a finding raises TrainingDiverged
        (`health_on_bad: stop`) on every rank or is printed (`warn`)."""
        m, s = self.model, self.settings
        master = bool(cfg_get(m.args, "isMaster", False))
        m.flush()
        nets = self._bind()
        self._watch(nets, step)          # a deferred generator update flush() just applied
        for w in ("G", "D"):
            self._stats(nets, w)
        out = nets["out"].cpu().numpy()
        lat = nets["latch"].cpu().numpy()
        nG = len(nets["G"].names)
        rows, findings, stats, grad_rms = [], [], {}, {}
        for w, o, l in (("G", out[:nG], lat[:nG]), ("D", out[nG:], lat[nG:nG + len(nets["D"].names)])):
            net = nets[w]
            stats[w] = o
            grad_rms[w] = math.sqrt(float(o[:, 1].sum()) / max(sum(net.numel), 1))
            e = lat[len(lat) - nG:] if (w == "G" and nets["ema"] is not None) else None
            for i, name in enumerate(net.names):
                n = net.numel[i]
                rp, rg, ru = (math.sqrt(float(o[i, c]) / n) for c in (0, 1, 2))
                ratio = ru / rp if rp > 0 else (0.0 if ru == 0 else math.inf)
                bad = [int(o[i, 6 + k]) for k in range(4)]
                first = -1
                if any(bad) or l[i] or (e is not None and e[i]):
                    first = net.first.get(name)
                    if first is None:
                        tags = [int(t) for t in (l[i], e[i] if e is not None else 0) if t]
                        first = min(net.step_of(t, step) for t in tags) if tags else step
                        net.first[name] = first
                    for k, buf in enumerate("pgmv"):
                        if bad[k]:
                            findings.append(dict(net=w, name=name, buffer=buf, count=bad[k], step=first))
                    if l[i] and not bad[2]:      # latched, and finite again (never after Adam's m)
                        findings.append(dict(net=w, name=name, buffer="m", count=0, step=first))
                    if e is not None and e[i]:
                        findings.append(dict(net=w, name=name, buffer="ema", count=0, step=first))
                rows.append(dict(step=step, scale=m.scale_index, net=w, name=name, numel=n, rms_p=rp,
                                 rms_g=rg, rms_u=ru, ratio=ratio, max_p=float(o[i, 3]),
                                 max_g=float(o[i, 4]), bad=sum(bad), first_bad_step=first))
        tag = int(lat[nG + len(nets["D"].names)])
        if tag:
            if nets["loss_first"] is None:
                nets["loss_first"] = tag - 1
            findings.append(dict(net="loss", name="loss", buffer="loss", count=0,
                                 step=nets["loss_first"]))
        for w in ("G", "D"):             # counts seen before this report are settled now
            nets[w].seen = {nets[w].fp.step: nets[w].seen.get(nets[w].fp.step, step)}
        # the earliest first; within a step the watched moment before the other buffers
        order = {b: k for k, b in enumerate(("m", "g", "v", "p", "ema", "loss"))}
        findings.sort(key=lambda f: (f["step"], order[f["buffer"]]))
        worst = max(rows, key=lambda r: r["ratio"] if math.isfinite(r["ratio"]) else -1.0)
        result = dict(step=step, scale=m.scale_index, report=True, rows=rows, stats=stats,
                      grad_rms=grad_rms, worst=(worst["net"], worst["name"], worst["ratio"]),
                      findings=findings)
        if master:
            d = f"{m.args.save_root}/{m.args.run_id}"
            os.makedirs(d, exist_ok=True)
            path = f"{d}/health.csv"
            if not os.path.exists(path) or os.path.getsize(path) == 0:
                with open(path, "a") as f:
                    f.write(CSV_HEADER + "\n")
            for r in rows:
                append_csv(path, *[r[k] for k in ROW_KEYS])
            print(f"step {step}: health grad rms G {grad_rms['G']:.3e} D {grad_rms['D']:.3e}, "
                  f"largest update/param {worst['ratio']:.3e} ({worst['net']} {worst['name']})" +
                  (f"; {describe(findings)}" if findings else ""))
        if findings:
            if s.on_bad == "stop":
                raise TrainingDiverged(findings)
            if master:
                print(f"step {step}: WARNING training has diverged: {describe(findings)}")
        return result

    # ------------------------------------------------------------------ checkpoints
    def checkpoint_findings(self):
        """save_checkpoint's guard (after its flush()): the non-finite counts of p, m, v of both
        nets and of the weight average, one statistics call per net.  [] when all are finite."""
        nets = self._bind()
        ema = self.model.fpG.ema
        self._stats(nets, "G", g_buffer=ema if ema is not None else nets["G"].fp.flat)
        self._stats(nets, "D", g_buffer=nets["D"].fp.flat)
        out = nets["out"].cpu().numpy()
        nG = len(nets["G"].names)
        found = []
        for w, o in (("G", out[:nG]), ("D", out[nG:])):
            for i, name in enumerate(nets[w].names):
                for c, buf in ((6, "p"), (7, "ema"), (8, "m"), (9, "v")):
                    if o[i, c] and not (buf == "ema" and (w == "D" or ema is None)):
                        found.append(dict(net=w, name=name, buffer=buf, count=int(o[i, c]),
                                          step=nets[w].first.get(name, -1)))
        return found


def newest_checkpoint(args):
    """The most recently written {save_root}/{run_id}/ckpt/*_latest.pt, or None."""
    import glob
    files = glob.glob(f"{args.save_root}/{args.run_id}/ckpt/*_latest.pt")
    return max(files, key=os.path.getmtime) if files else None
