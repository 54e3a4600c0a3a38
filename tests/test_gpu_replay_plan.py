"""The planned C++ replay (pg_record_optimize: dead records and redundant waits dropped) on
the device: BITWISE what the recording re-issued as recorded, and what the eager sequence,
computes.  The plan removes bookkeeping only, so any difference is an ordering edge it should
have kept.

A stream left waiting for ever would hang a synchronize, so nothing here blocks in one:
`finish` polls both streams and ends the whole session at its deadline.  Work is then still
queued, and the process may block in the runtime when it exits: run these under an outer time
limit as well, which remains the real guard."""
import time

import pytest
import torch

from gen_inputs import TINY_DEPTHS
from test_gpu_graph import build_replay, state
from test_model_api import make_args

pytestmark = pytest.mark.gpu


def finish(*streams, seconds=60.0):
    """Wait for the current stream and `streams` without blocking in the runtime."""
    streams = (torch.cuda.current_stream(),) + streams
    t0 = time.perf_counter()
    while not all(s.query() for s in streams):
        if time.perf_counter() - t0 > seconds:
            pytest.exit("a stream did not drain: the device is left alone", returncode=3)
        time.sleep(0.0005)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_planned_replay_matches_unplanned_bitwise(tmp_path, dtype):
    """The tiny model (stage 2, batch 4) stepped from identical state with replay_plan on and
    off: step 0 packs the weights, step 1 is the key's first step, step 2 records while it
    runs, steps 3-5 replay -- parameters, gradients, Adam moments, latents and losses equal
    bit for bit after every step.  The plan must have had something to do: at least one record
    dropped (the pass binds no record to a launch: that rule was measured and left out)."""
    args = make_args(tmp_path, depths=list(TINY_DEPTHS), compute_dtype=dtype)
    s = 2
    models = {plan: build_replay(args, s) for plan in (1, 0)}
    for m in models.values():
        m.G.alpha = m.D.alpha = 0.5
    replayed = {1: 0, 0: 0}
    for step in range(6):
        for plan, m in models.items():
            n0 = m.graph_replays
            m.train_step()
            eng = next(iter(m._engines.values()))
            eng.replay_plan = plan          # read when the step is recorded (step 2)
            finish(eng.side)
            replayed[plan] += m.graph_replays - n0
        a, b = state(models[1]), state(models[0])
        for k in a:
            assert torch.equal(a[k], b[k]), (step, k, float((a[k].double() - b[k].double()).abs().max()))
    assert replayed == {1: 3, 0: 3}, replayed
    assert "plan" not in models[0]._gstate
    st = models[1]._gstate["plan"]
    assert st["closed"] == 1 and 1 <= st["records_dropped"] < st["records"], st


def test_two_stream_recording_replayed_with_the_plan_matches_eager():
    """main: fill X, X += a/2, record | side: wait, Y = X/2 + a/4, record | main: wait,
    Z = Y + 0.94 X, a <- Z: a shrinks by 0.97 per round, each stage reads what the other stream
    just wrote, and the fill clears X first, so a stage that starts early reads zeros or the
    previous round's values.  Recorded once and replayed 50 times with the plan (both records
    are waited on and survive it) against 51 eager rounds: bitwise."""
    from pggan_amd import _lib
    ops = _lib.HipOps(torch.float32)
    side = ops.side_stream()
    n = (4 << 20) + 4
    torch.manual_seed(3)
    a0 = torch.randn(n, device="cuda")

    def buffers():
        return dict(a=a0.clone(), X=torch.full_like(a0, 7.0), Y=torch.full_like(a0, 7.0),
                    Z=torch.full_like(a0, 7.0))

    ev_m, ev_s = ops.event(), ops.event()

    def one_round(t):
        ops.zero_(t["X"])
        ops.blend(0.5, t["a"], 1.0, t["X"], t["X"])                 # X = a/2 (+ the zeros)
        ev_m.record()
        ev_m.wait(side)
        with torch.cuda.stream(side):
            ops.blend(0.5, t["X"], 0.25, t["a"], t["Y"])            # Y = X/2 + a/4
        ev_s.record(side)
        ev_s.wait()
        ops.blend(1.0, t["Y"], 0.94, t["X"], t["Z"])                # Z = Y + 0.94 X = 0.97 a
        ops.copy_(t["a"], t["Z"])

    eager, rep = buffers(), buffers()
    torch.cuda.synchronize()
    for _ in range(51):
        one_round(eager)
    finish(side)
    ops.record_begin()
    one_round(rep)
    rec = ops.record_end()
    st = rec.optimize(closed=True)
    assert (st["ops"], st["records"], st["waits"]) == (9, 2, 2), st
    assert st == dict(st, closed=1, records_dropped=0, waits_dropped=0), st
    for _ in range(50):
        rec.replay()
    finish(side)
    for k in eager:
        assert torch.equal(eager[k], rep[k]), (k, float((eager[k] - rep[k]).abs().max()))
    assert 0.1 < float(rep["a"].abs().max() / a0.abs().max()) < 0.5     # 0.97 ** 51 = 0.21
