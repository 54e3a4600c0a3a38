"""CPU test double of the training-health ops (pg_tensor_stats, pg_nonfinite_watch) on top of
tests/cpu_ops.py's CpuOps -- TEST INFRASTRUCTURE ONLY.  Same argument meaning as
pggan_amd._lib.HipOps.tensor_stats / nonfinite_watch / adam_pair, plain float64 PyTorch written
from the definitions in include/pggan_hip.h, so that pggan_amd.health's host logic runs without
a GPU (tests/health_ref.py is the independent numpy reference both are held to)."""
import math

import numpy as np
import torch

from cpu_ops import CpuOps

CHUNK = 2048        # no kernel here: any value serves the tests that place sizes around it


class CpuOpsHealth(CpuOps):
    TS_COLS = 10
    tensor_stats_chunk = CHUNK

    def adam_pair(self, lr, beta1, beta2, t):
        """pg_adam's scalars for update t: double arithmetic on the fp32 betas, rounded to fp32."""
        b1, b2 = float(np.float32(beta1)), float(np.float32(beta2))
        t = max(int(t), 1)
        return (float(np.float32(float(np.float32(lr)) / (1.0 - b1 ** t))),
                float(np.float32(math.sqrt(1.0 - b2 ** t))))

    def tensor_stats(self, table, p, g, m, v, *, step_size, bc2_sqrt, eps, out):
        ss, bc, e = (float(np.float32(x)) for x in (step_size, bc2_sqrt, eps))
        out.zero_()
        for s, (off, cnt) in enumerate(table.tolist()):
            sl = slice(off, off + cnt)
            for k, x in enumerate((p, g)):
                if x is not None:
                    a = x[sl].double().abs()
                    a = a[torch.isfinite(a)]
                    out[s, k] = (a * a).sum()
                    out[s, 3 + k] = a.max() if a.numel() else 0.0
            for k, x in enumerate((p, g, m, v)):
                if x is not None:
                    out[s, 6 + k] = int((~torch.isfinite(x[sl])).sum())
            if m is not None and v is not None:
                md, vd = m[sl].double(), v[sl].double()
                ok = torch.isfinite(md) & torch.isfinite(vd)
                md, vd = md[ok], vd[ok]
                u = ((ss * md) / (vd.sqrt() / bc + e)).abs()
                out[s, 2] = (u * u).sum()
                out[s, 5] = u.max() if u.numel() else 0.0

    def nonfinite_watch(self, table, x, tag, first_bad):
        if tag < 1:
            raise RuntimeError(f"nonfinite_watch failed (-1): tag ({tag}) must be positive")
        for s, (off, cnt) in enumerate(table.tolist()):
            if int(first_bad[s]) == 0 and not bool(torch.isfinite(x[off:off + cnt]).all()):
                first_bad[s] = tag


class RecordingHealthOps(CpuOpsHealth):
    """CpuOpsHealth that appends the name of every op call to the class-wide `calls`."""
    calls = []

    def __getattribute__(self, name):
        v = super().__getattribute__(name)
        if name.startswith("_") or name in ("calls", "tdtype", "fused") or not callable(v):
            return v
        calls = type(self).calls

        def rec(*a, **kw):
            calls.append(name)
            return v(*a, **kw)
        return rec
