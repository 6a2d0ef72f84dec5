"""CPU: the model of the deferred one-level path's bookkeeping (tests/defer_model.py) against its own invariants, over random
sequences of submit, sync and reset -- the GPU test compares the engine with this model, so the model must be right on its own."""
import numpy as np
import pytest

from tests import defer_model as dm

SEEDS = (1, 2, 3, 4, 5, 6, 7, 8)


@pytest.mark.parametrize("depth,room", [(2, None), (3, None), (4, None), (8, None), (3, 2), (8, 3), (4, 4)])
def test_every_batch_is_flushed_once_or_dropped(depth, room):
    for seed in SEEDS:
        ops = dm.fixed_ops(seed, 60)
        m, seen, holds = dm.run_model(ops + ["sync"], depth, room)
        flushed = [b for f in m.flushes for b in f]
        assert sorted(flushed + m.dropped) == list(range(m.next_batch)), (seed, depth, room)       # each exactly once
        assert flushed == sorted(flushed)                                                          # in submit order
        assert all(1 <= len(f) <= min(depth, m.room) for f in m.flushes)
        assert all(f == list(range(f[0], f[0] + len(f))) for f in m.flushes)                      # a flush holds consecutive batches
        assert m.pending == [] and seen[-1][0] == 0
        for (pend, nfl, nb, full), op in zip(seen, ops + ["sync"]):
            assert pend < depth and pend <= m.room
            if op != "submit":
                assert pend == 0
        assert m.full_flushes == 0 or m.room < depth
        # what the vector holds at the end: the batches since the last reset
        last_reset = max([i for i, op in enumerate(ops) if op == "reset"], default=-1)
        n_before = sum(1 for op in ops[:last_reset + 1] if op == "submit")
        assert holds[-1] == list(range(n_before, m.next_batch)) == [b for b in flushed if b >= n_before]


def test_depth_edges():
    for n, want in ((2, (1, 2)), (3, (1, 3)), (4, (2, 4))):      # D - 1, D, D + 1 batches at depth 3, then a sync
        m, seen, _ = dm.run_model(["submit"] * n + ["sync"], 3)
        assert seen[-1][1:3] == want and seen[-1][0] == 0
    m, seen, _ = dm.run_model(["submit"] * 3, 3)
    assert seen[-1] == (0, 1, 3, 0)                               # the third submit flushes: nothing waits for the sync


def test_full_arena_and_reset():
    m, seen, _ = dm.run_model(["submit"] * 5 + ["sync"], 8, room=2)
    assert m.flushes == [[0, 1], [2, 3], [4]] and m.full_flushes == 2
    m, seen, holds = dm.run_model(["submit", "submit", "reset", "submit", "sync"], 4)
    assert m.flushes == [[2]] and m.dropped == [0, 1] and holds[-1] == [2]


def test_immediate_path_counts_nothing():
    ops = dm.fixed_ops(11, 30)
    m, seen, _ = dm.run_model(ops, 0)
    assert all(s == (0, 0, 0, 0) for s in seen)


def test_drawn_sequences_cover_the_cases():
    rng = np.random.Generator(np.random.PCG64(5))
    ops = dm.draw_ops(rng, 200)
    assert {"submit", "sync", "reset"} <= set(ops)
    runs = "".join("s" if op == "submit" else "." for op in ops).split(".")
    assert max(len(r) for r in runs) >= 8                         # a run of submits longer than the deepest depth in use
    assert any(a == "sync" and b == "sync" for a, b in zip(ops, ops[1:])) or any(a == "reset" and b == "sync" for a, b in zip(ops, ops[1:]))
