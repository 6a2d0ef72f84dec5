"""A model of the deferred one-level path's bookkeeping (engine option one_level_defer, csrc/kdb_scatter_host.hip.h: OneLevelPending).

Which batches are pending, and which batches each flush (one page sort, one histogram pass) adds to the vector, over a sequence of
submit / sync / reset.  The rules, for batches whose regions all have the same size:

    submit   the batch is scattered into the arena behind those pending; if its region does not fit, what is pending is flushed first
             (a "full" flush); when `depth` batches are pending they are flushed
    sync     what is pending is flushed (no flush when nothing is)
    reset    what is pending is dropped: no flush ever holds it

`room` is the number of regions the arena holds (None: at least `depth`, the arena is never full).  depth = 0 is the immediate path:
nothing is ever pending and no flush is counted.

The CPU tests check the model against its own invariants; the GPU test runs the same sequence on an engine and compares the engine's
counters (pending_batches, hist_flushes, flushed_batches, full_flushes) with the model after every operation."""
import numpy as np


class DeferModel:
    def __init__(self, depth, room=None):
        assert depth == 0 or depth >= 2
        self.depth, self.room = depth, (room if room is not None else max(depth, 2))
        assert depth == 0 or self.room >= 2
        self.pending = []            # batch numbers, in submit order
        self.flushes = []            # one list of batch numbers per flush
        self.full_flushes = 0
        self.dropped = []
        self.next_batch = 0

    def _flush(self):
        if self.pending:
            self.flushes.append(self.pending)
            self.pending = []

    def submit(self):
        b = self.next_batch
        self.next_batch += 1
        if self.depth == 0:
            return b
        if len(self.pending) + 1 > self.room:
            self.full_flushes += 1
            self._flush()
        self.pending.append(b)
        if len(self.pending) >= self.depth:
            self._flush()
        return b

    def sync(self):
        self._flush()

    def reset(self):
        self.dropped += self.pending
        self.pending = []

    def counters(self):
        """(pending_batches, hist_flushes, flushed_batches, full_flushes) as the engine reports them"""
        return len(self.pending), len(self.flushes), sum(len(f) for f in self.flushes), self.full_flushes


def draw_ops(rng, n_ops=40):
    """a random sequence of "submit", "sync", "reset": mostly submits, runs of them longer than any depth in use, syncs and resets
    with and without batches pending"""
    ops = []
    while len(ops) < n_ops:
        r = rng.random()
        if r < 0.70:
            ops += ["submit"] * int(rng.integers(1, 6))
        elif r < 0.88:
            ops.append("sync")
        else:
            ops.append("reset")
    return ops[:n_ops]


def run_model(ops, depth, room=None):
    """-> (model, counters after every op, for every op the batch numbers the vector must hold once synced)"""
    m = DeferModel(depth, room)
    seen, alive, holds = [], [], []
    for op in ops:
        if op == "submit":
            alive.append(m.submit())
        elif op == "sync":
            m.sync()
        else:
            m.reset()
            alive = []
        seen.append(m.counters())
        holds.append(list(alive))
    return m, seen, holds


def fixed_ops(seed, n_ops=40):
    return draw_ops(np.random.Generator(np.random.PCG64(seed)), n_ops)
