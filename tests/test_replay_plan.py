"""The replay plan pass (pg_record_optimize) on the host, through pg_replay_plan_host: the same
pass over synthetic (kind, stream, event) ops.  One hand-written sequence per rule, and a
seeded property test against a happens-before simulator written here: whatever the plan drops,
every pair of work ops (launch / fill / copy) the original list orders stays ordered.

The simulator's model of the streams: ops of one stream run in list order; a record takes a
snapshot of everything its stream is ordered behind at that point; a wait adds the snapshot of
its event's latest record before it in the list (the order the host resolves it in) to its
stream.

The pass binds no record to a launch (that rule was measured and left out, DESIGN.md
"Streams"): a surviving record is always issued as a plain record, so the flags are KEEP and
DROP only."""
import os
import random

import pytest

from pggan_amd import _lib

L, R, W, F, C = _lib.OP_LAUNCH, _lib.OP_RECORD, _lib.OP_WAIT, _lib.OP_FILL, _lib.OP_COPY
KEEP, DROP = _lib.PLAN_KEEP, _lib.PLAN_DROP
MAIN, SIDE, THIRD = 0, 1, 2


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libpggan_hip.so not built")
    return _lib.load_library()


def plan(lib, ops, closed):
    return _lib.replay_plan_host(lib, ops, closed)


# ------------------------------------------------------------------ one sequence per rule
def test_overwritten_unwaited_side_record_is_dropped_only_when_closed(lib):
    """Two side calls in the engine's form; only the second side record (event 11) is joined.
    The first (event 10) is never waited on: dead with closed=1, kept without."""
    ops = [(L, MAIN, 0), (R, MAIN, 1), (W, SIDE, 1), (L, SIDE, 0), (R, SIDE, 10),
           (L, MAIN, 0), (R, MAIN, 2), (W, SIDE, 2), (L, SIDE, 0), (R, SIDE, 11),
           (W, MAIN, 11), (L, MAIN, 0)]
    assert plan(lib, ops, 1) == [KEEP] * 4 + [DROP] + [KEEP] * 7    # no wait is redundant here
    assert plan(lib, ops, 0) == [KEEP] * 12
    # the same event re-recorded un-waited (a ring slot that comes round): the first is dead
    ops = [(L, SIDE, 0), (R, SIDE, 10), (L, SIDE, 0), (R, SIDE, 10), (W, MAIN, 10), (L, MAIN, 0)]
    assert plan(lib, ops, 1) == [KEEP, DROP, KEEP, KEEP, KEEP, KEEP]
    assert plan(lib, ops, 0) == [KEEP] * 6


def test_last_record_of_an_event_is_kept_when_not_closed(lib):
    ops = [(L, SIDE, 0), (F, SIDE, 0), (R, SIDE, 10)]
    assert plan(lib, ops, 0) == [KEEP, KEEP, KEEP]
    assert plan(lib, ops, 1) == [KEEP, KEEP, DROP]


def test_surviving_records_stay_plain_records(lib):
    """A waited-on record is issued as recorded wherever it stands: behind a fill or a copy,
    behind nothing (it covers the previous replay's work: its wait is not redundant), right
    behind a launch, and behind a wait on its own stream, redundant or not."""
    for kind in (F, C, L):
        ops = [(L, MAIN, 0), (kind, MAIN, 0), (R, MAIN, 1), (W, SIDE, 1), (L, SIDE, 0)]
        assert plan(lib, ops, 1) == [KEEP] * 5
    ops = [(R, MAIN, 1), (W, SIDE, 1), (L, SIDE, 0)]
    assert plan(lib, ops, 1) == [KEEP] * 3
    ops = [(L, SIDE, 0), (R, SIDE, 10), (L, MAIN, 0), (W, MAIN, 10), (R, MAIN, 1), (W, THIRD, 1),
           (L, THIRD, 0)]
    assert plan(lib, ops, 1) == [KEEP] * 7
    ops = [(L, SIDE, 0), (R, SIDE, 10), (W, MAIN, 10), (L, MAIN, 0), (W, MAIN, 10), (R, MAIN, 1),
           (W, THIRD, 1), (L, THIRD, 0)]
    assert plan(lib, ops, 1) == [KEEP] * 4 + [DROP] + [KEEP] * 3


def test_redundant_waits(lib):
    # a second wait on the same record; a wait on an earlier record of the same stream
    ops = [(L, SIDE, 0), (R, SIDE, 10), (L, SIDE, 0), (R, SIDE, 11), (W, MAIN, 11), (W, MAIN, 11),
           (W, MAIN, 10), (L, MAIN, 0)]
    assert plan(lib, ops, 0)[4:7] == [KEEP, DROP, DROP]
    # through a third stream: main waits on side behind side's wait on third
    ops = [(L, THIRD, 0), (R, THIRD, 20), (W, SIDE, 20), (L, SIDE, 0), (R, SIDE, 10),
           (W, MAIN, 10), (W, MAIN, 20), (L, MAIN, 0)]
    assert plan(lib, ops, 0)[5:7] == [KEEP, DROP]
    # not implied: the record on third follows more work there
    ops = [(L, THIRD, 0), (R, THIRD, 20), (W, SIDE, 20), (L, SIDE, 0), (R, SIDE, 10),
           (L, THIRD, 0), (R, THIRD, 21), (W, MAIN, 10), (W, MAIN, 21), (L, MAIN, 0)]
    assert plan(lib, ops, 0)[7:9] == [KEEP, KEEP]
    # a stream's wait on its own record orders nothing
    ops = [(L, MAIN, 0), (R, MAIN, 1), (W, MAIN, 1), (L, MAIN, 0)]
    assert plan(lib, ops, 0)[2] == DROP


def test_wait_on_an_event_never_recorded_leaves_a_closed_recording_untouched(lib):
    ops = [(W, MAIN, 99),                                   # recorded by an earlier step
           (L, MAIN, 0), (R, MAIN, 1), (W, SIDE, 1), (W, SIDE, 1), (L, SIDE, 0), (R, SIDE, 10)]
    assert plan(lib, ops, 1) == [KEEP] * len(ops)
    # ... also where the event is recorded later in the list
    assert plan(lib, ops + [(R, SIDE, 99)], 1) == [KEEP] * (len(ops) + 1)
    # without the promise the unknown wait stays and the local rules apply
    got = plan(lib, ops, 0)
    assert got == [KEEP, KEEP, KEEP, KEEP, DROP, KEEP, KEEP]


def test_bad_ops_are_refused(lib):
    for ops in ([(7, 0, 0)], [(L, -1, 0)], [(W, 0, -1)]):
        with pytest.raises(RuntimeError):
            plan(lib, ops, 0)
    assert plan(lib, [], 1) == []


# ------------------------------------------------------------------ the property test
def simulate(ops):
    """ops: (kind, stream, event, id) in issue order.  Returns (before, final): before[id] the
    work ops ordered before work op `id`; final[event] the snapshot of the event's last record.
    Each stream starts behind its own earlier work (("prior", s): the previous replay)."""
    behind, ev, before = {}, {}, {}
    for kind, s, e, ident in ops:
        cur = behind.setdefault(s, {("prior", s)})
        if kind == R:
            ev[e] = set(cur)
        elif kind == W:
            cur |= ev.get(e, set())
        else:
            before[ident] = set(cur)
            cur.add(ident)
    return before, ev


def apply_plan(ops, flags):
    """The list the planned recording issues: the dropped records and waits gone."""
    assert all(f == KEEP or (f == DROP and op[0] in (R, W)) for f, op in zip(flags, ops))
    return [(k, s, e, i) for i, (k, s, e) in enumerate(ops) if flags[i] == KEEP]


def random_ops(rng):
    ns, ne = rng.choice((2, 3)), rng.randint(1, 8)
    ops, recorded = [], []
    for _ in range(rng.randint(1, 40)):
        s = rng.randrange(ns)
        x = rng.random()
        if x < 0.40:
            ops.append((L, s, 0))
        elif x < 0.48:
            ops.append((rng.choice((F, C)), s, 0))
        elif x < 0.75 or not recorded:
            e = rng.randrange(ne)
            ops.append((R, s, e))
            recorded.append(e)
        else:
            ops.append((W, s, rng.choice(recorded)))
    return ops


def test_plan_keeps_every_ordering_of_random_sequences(lib):
    rng = random.Random(20240607)
    seen = {"drop_record": 0, "drop_wait": 0}
    for _ in range(400):
        ops = random_ops(rng)
        before0, final0 = simulate([(k, s, e, i) for i, (k, s, e) in enumerate(ops)])
        for closed in (0, 1):
            flags = plan(lib, ops, closed)
            assert len(flags) == len(ops)
            before1, final1 = simulate(apply_plan(ops, flags))
            for ident, pre in before0.items():
                assert pre <= before1[ident], (ops, closed, flags, ident)
            if not closed:
                assert not any(f == DROP and op[0] == R for f, op in zip(flags, ops)), (ops, flags)
                for e, snap in final0.items():
                    assert snap <= final1[e], (ops, flags, e)
            for f, op in zip(flags, ops):
                seen["drop_record"] += f == DROP and op[0] == R
                seen["drop_wait"] += f == DROP and op[0] == W
    assert all(v > 50 for v in seen.values()), seen
