"""Times the nearest-training-image search (pggan_amd/metrics.py over csrc/nn.hip) against the
same search written with plain torch ops on the GPU, and against a plain device copy of the
database bytes, per DESIGN.md "Validation: nearest training images".  One pg_nn_search call of
--queries queries against --rows database rows at each comparison resolution; device events
around ten back-to-back calls of each part, a warm-up, then the median of --runs repetitions.

    python tools/nn_bench.py --res 64 128 [--queries 64] [--rows 30000] [--k 3] [--json out.json]

"search": the int8 rows read once, v_mfma_i32_16x16x64_i8, the per-workgroup lists and their
merge (both launches).  "torch": the rows cast to fp32, q @ db.T, the norms, topk; and the
same with the fp32 database already resident ("torch_resident", 4 x the memory).  "copy":
dst.copy_(db), which reads and writes the database bytes once each: the search reads them once
and writes next to nothing, so half the copy time is its HBM floor.  Nothing in the baseline is
tuned."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from pggan_amd import _lib, metrics  # noqa: E402


INNER = 10      # calls between two events


def timed(fn, runs, warm=3):
    """Median / min device time of one fn() in ms: events on the current stream around INNER
    calls issued back to back, so that the stream stays busy and the figure is the device's
    time per call, not the host's time to issue one (a search at 64 x 64 is shorter than
    that)."""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(INNER):
            fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) / INNER)
    return statistics.median(ts), min(ts)


def torch_search(q, qsq, dbf, dbsq, k):
    """(d2 fp32 [Q, k], idx [Q, k]) with dbf the database as fp32."""
    d2 = qsq.float()[:, None] + dbsq.float()[None, :] - 2 * (q.float() @ dbf.T)
    v, i = torch.topk(d2, k, dim=1, largest=False)
    return v, i


def bench(Rc, Q, N, k, runs):
    dev = torch.device("cuda")
    ops = _lib.HipOps(torch.float32)
    D = 3 * Rc * Rc
    g = torch.Generator(device=dev).manual_seed(Rc)
    # smooth rows (a coarse pattern per image plus small noise), queries near database rows
    base = torch.randint(-100, 100, (N, D // 64, 1), device=dev, generator=g)
    db = (base + torch.randint(-20, 21, (N, D // 64, 64), device=dev, generator=g)).reshape(N, D)
    db = db.to(torch.int8).contiguous()
    pick = torch.randint(0, N, (Q,), device=dev, generator=g)
    q = (db[pick].int() + torch.randint(-2, 3, (Q, D), device=dev, generator=g)).clamp(-128, 127)
    q = q.to(torch.int8).contiguous()
    dbsq = db.int().square().sum(1).int()
    qsq = q.int().square().sum(1).int()
    res = {"compare": Rc, "D": D, "queries": Q, "rows": N, "k": k, "database_MB": N * D / 1e6}

    best_d2 = torch.full((Q, k), metrics.NN_NONE, dtype=torch.int64, device=dev)
    best_idx = torch.full((Q, k), -1, dtype=torch.int64, device=dev)

    def search():       # both launches; from the second call on the lists are full: the same work
        ops.nn_search(q, qsq, db, dbsq, 0, best_d2, best_idx)

    t, tmin = timed(search, runs)
    res["search_ms"], res["search_min_ms"] = t, tmin
    res["search_GBps"] = N * D / (t * 1e-3) / 1e9
    res["search_TOPS"] = 2.0 * Q * N * D / (t * 1e-3) / 1e12
    dst = torch.empty_like(db)
    t, _ = timed(lambda: dst.copy_(db), runs)
    res["copy_ms"], res["copy_GBps"] = t, 2 * N * D / (t * 1e-3) / 1e9
    res["read_floor_ms"] = t / 2
    res["search_vs_read_floor"] = res["search_ms"] / res["read_floor_ms"]
    del dst
    res["torch_ms"], _ = timed(lambda: torch_search(q, qsq, db.float(), dbsq, k), runs)
    dbf = db.float()
    res["torch_resident_ms"], _ = timed(lambda: torch_search(q, qsq, dbf, dbsq, k), runs)
    res["speedup"] = res["torch_ms"] / res["search_ms"]
    res["speedup_resident"] = res["torch_resident_ms"] / res["search_ms"]
    # the two pipelines find the same nearest rows (fp32 sums of this size are not exact, so
    # only the planted neighbour is compared)
    best_d2.fill_(metrics.NN_NONE)
    best_idx.fill_(-1)
    search()
    res["nearest_is_planted"] = bool((best_idx[:, 0] == pick).all() or
                                     (best_d2[:, 0] <= 4 * D).all())
    res["torch_agrees_on_nearest"] = bool((torch_search(q, qsq, dbf, dbsq, k)[1][:, 0] ==
                                           best_idx[:, 0]).all())
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, nargs="+", default=[64, 128])
    ap.add_argument("--queries", type=int, default=64)
    ap.add_argument("--rows", type=int, default=30000)
    ap.add_argument("--k", type=int, default=3)
    ap.add_argument("--runs", type=int, default=12)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("nn_bench: needs a GPU (timings on a CPU would say nothing)")
    if a.runs < 10:
        raise SystemExit("nn_bench: --runs must be >= 10")
    out = []
    for Rc in a.res:
        r = bench(Rc, a.queries, a.rows, a.k, a.runs)
        out.append(r)
        print(json.dumps(r), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
