"""tests/lifecycle_model.py checked without a GPU: the model and the driver against a stand-in engine that is written another way
(dense numpy vectors, whole batches through oracle.c_count), the continuation pieces against the windows of the whole record, and
the fixed seeds against the list of op orders they must contain (tests/test_gpu_lifecycle.py runs those seeds on the real engine)."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lifecycle_model as lm  # noqa: E402

SEEDS, fixed_sequence = lm.SEEDS, lm.fixed_sequence


class StandInError(ValueError):
    def __init__(self, kind):
        ValueError.__init__(self, kind)
        self.kind = kind


class StandIn:
    """kmerdb_amd.Engine's interface over dense numpy vectors; a batch is counted whole by oracle.c_count.  `mistake` seeds one bug."""

    def __init__(self, oracle, k, canon, n_mode, mistake=None):
        self.o, self.k, self.canon, self.n_mode, self.mistake = oracle, k, canon, n_mode, mistake
        self.nbins = 4 ** k
        self.table = np.zeros(self.nbins, np.uint64)
        self.acc = np.zeros(self.nbins, np.uint64)
        self.emitted = self.folded_total = 0
        self.error = None
        self.algo = 2

    def close(self):
        pass

    def set_option(self, name, value):
        if name == "algo":
            self.algo = value

    def _fail(self, kind):
        if self.error is None:
            self.error = kind

    def _count(self, bases, offsets, continues=False):
        bases, offsets = np.asarray(bases, dtype=np.uint8), np.asarray(offsets, dtype=np.uint64)
        if int(offsets[0]) != 0 or int(offsets[-1]) != bases.size:
            return self._fail("bad_layout")
        if continues and int(offsets[1]) < self.k:          # a continuation piece is no record: not subject to the short check
            bases, offsets = bases[int(offsets[1]):], offsets[1:] - offsets[1]
            if len(offsets) < 2:
                return None
        try:
            c, t = self.o.c_count(bases, offsets, self.k, self.canon, self.o.N_EXPAND if self.n_mode else self.o.N_DROP)
        except self.o.OracleError as e:
            return self._fail("short" if e.status == self.o.SHORT_READ else "bad_residue")
        self.table += c
        self.emitted += t
        return None

    def submit(self, bases, offsets, continues=False):
        self._count(bases, offsets, continues)

    submit_pinned = submit

    def submit_device(self, bases_ptr, nbytes, offsets_ptr, nreads, const=False):
        bases = np.ctypeslib.as_array(ctypes.cast(bases_ptr, ctypes.POINTER(ctypes.c_uint8)), shape=(nbytes,))
        offsets = np.ctypeslib.as_array(ctypes.cast(offsets_ptr, ctypes.POINTER(ctypes.c_uint64)), shape=(nreads + 1,))
        if const and self.algo == 1 and len(set(np.diff(offsets.astype(np.int64)).tolist())) > 1:
            self._fail("not_uniform")
        self._count(bases, offsets)

    def submit_device_const(self, bases_ptr, nbytes, offsets_ptr, nreads):
        self.submit_device(bases_ptr, nbytes, offsets_ptr, nreads, const=True)

    def _check(self):
        if self.error:
            raise StandInError(self.error)

    def sync(self):
        self._check()

    def reset(self):
        self.table[:] = 0
        if self.mistake != "reset keeps the accumulator":
            self.acc[:] = 0
            self.folded_total = 0
        self.emitted = 0
        if self.mistake != "reset keeps the error":
            self.error = None

    def table_stats(self, copy=True):
        self._check()
        return (self.table.copy() if copy else None), int(self.table.sum()), int(np.count_nonzero(self.table))

    def finish(self, copy=True):
        self._check()
        if int(self.table.sum()) != self.emitted:
            raise StandInError("sum")
        return (self.table.copy() if copy else None), self.emitted, int(np.count_nonzero(self.table))

    def fold_file(self, into=None):
        self._check()
        acc = into if into is not None else self
        total, unique = self.emitted, int(np.count_nonzero(self.table))
        acc.acc += self.table
        acc.folded_total += total
        if self.mistake != "fold does not clear the file vector":
            self.table[:] = 0
        if self.mistake != "fold keeps the file's total":
            self.emitted = 0
        return total, unique

    def finish_folded(self, copy=True):
        self._check()
        return (self.acc.copy() if copy else None), self.folded_total, int(np.count_nonzero(self.acc))

    def nullomers(self, n=None, folded=False):
        self._check()
        return np.flatnonzero((self.acc if folded else self.table) == 0).astype(np.uint64)

    def nullomer_count(self, folded):
        return len(self.nullomers(folded=folded))


class CpuHost:
    """Host arrays stand for device buffers and pinned memory; the 'device pointer' is the array's address."""

    def to_device(self, arr):
        a = np.ascontiguousarray(arr).copy()
        return a, a.ctypes.data

    def pinned(self, nbytes):
        return np.empty(nbytes, dtype=np.uint8)

    def add_to_table(self, eng, ids, n):
        eng.table[np.asarray(ids, dtype=np.int64)] += np.uint64(n)


def run_stand_in(oracle, k, seed, mistake=None):
    ops = fixed_sequence(k, seed)
    model = lm.ModelEngine(k, ops[0]["canon"], ops[0]["n_mode"], oracle)
    return lm.run_sequence(lambda canon, n_mode: StandIn(oracle, k, canon, n_mode, mistake), ops, model, host=CpuHost())


CPU_SEEDS = [(k, s) for k in (3, 6) for s in range(1, 9)]


@pytest.mark.parametrize("k,seed", CPU_SEEDS)
def test_drawn_sequences_pass_against_the_stand_in(oracle, k, seed):
    checks = run_stand_in(oracle, k, seed)
    assert len(checks) >= 3


@pytest.mark.parametrize("mistake", ["fold does not clear the file vector", "reset keeps the accumulator", "fold keeps the file's total",
                                     "reset keeps the error"])
def test_a_stand_in_with_one_seeded_mistake_fails(oracle, mistake):
    failed = 0
    for k, seed in CPU_SEEDS:
        try:
            run_stand_in(oracle, k, seed, mistake)
        except (AssertionError, StandInError):
            failed += 1
    assert failed >= 1, mistake


def test_caller_write_op_and_the_sum_check(oracle):
    """The op that drawn sequences leave out: somebody else writes the vector; table_stats sees it, finish() refuses."""
    recs = [b"ACGTTGCAAC", b"GGGTACCATT"]
    ops = [{"op": "create", "canon": True, "n_mode": 0}, {"op": "submit_host", "records": recs},
           {"op": "caller_adds", "ids": [0, 5, 63], "n": 5}, {"op": "table_stats", "copy": True}, {"op": "finish", "copy": True},
           {"op": "reset"}, {"op": "submit_host", "records": recs}, {"op": "finish", "copy": True}]
    checks = lm.run_sequence(lambda canon, n_mode: StandIn(oracle, 3, canon, n_mode), ops, lm.ModelEngine(3, True, 0, oracle), host=CpuHost())
    assert [w for _, w in checks] == ["table_stats totals", "table_stats vector", "finish raises sum", "finish totals", "finish vector"]


def _windows(oracle, piece, k, canon, omode, exempt):
    if exempt and len(piece) < k:
        return []
    ids, pos = oracle.c_shred(piece, k, canon, omode)
    return list(zip(pos.tolist(), ids.tolist()))


@pytest.mark.parametrize("k", [3, 6])
@pytest.mark.parametrize("expand", [False, True])
def test_pieces_carry_every_window_of_the_record_once(oracle, k, expand):
    omode = oracle.N_EXPAND if expand else oracle.N_DROP
    rng = np.random.Generator(np.random.PCG64(k))
    rec = bytearray(lm.LET[rng.integers(0, 4, size=3 * k)].tobytes())
    for with_n in (False, True):
        for cut in range(k, 3 * k):
            r = bytearray(rec)
            if with_n:
                r[cut - 1] = ord("N")             # inside the k - 1 residues that the second piece repeats
            whole = sorted(_windows(oracle, bytes(r), k, True, omode, False))
            for cuts in ([cut], [cut, cut] if cut < 3 * k - 1 else [cut], [cut, cut + 1] if cut + 1 < 3 * k else [cut]):
                ps = lm.pieces(bytes(r), k, cuts)
                ends = cuts + [len(r)]
                got = []
                for j, p in enumerate(ps):
                    start = 0 if j == 0 else ends[j - 1] - (k - 1)
                    got += [(start + q, i) for q, i in _windows(oracle, p, k, True, omode, j > 0)]
                assert sorted(got) == whole, (cuts, with_n)
    # a piece of exactly k residues carries one new window, one of k - 1 none
    ps = lm.pieces(bytes(rec), k, [k, k, k + 1])
    assert [len(p) for p in ps[1:3]] == [k - 1, k]
    assert _windows(oracle, ps[1], k, True, omode, True) == [] and len(_windows(oracle, ps[2], k, True, oracle.N_DROP, True)) == 1
    with pytest.raises(ValueError):
        lm.pieces(bytes(rec), k, [k - 1])         # piece 0 is a record: it must hold a window


def test_fixed_seeds_hold_every_op_kind_and_every_order():
    """A condition on the seeds, not a hope: if a seed set misses an order, change the seeds."""
    kinds, have13 = set(), set()
    for k, seed in SEEDS:
        ops = fixed_sequence(k, seed)
        kinds |= {o["op"] for o in ops}
        names = {(o["name"]) for o in ops if o["op"] == "set_option" and not o.get("init")}
        kinds |= {"set_option:" + n for n in names}
        if k >= 13:
            have13 |= lm.coverage(ops, k)
        # records 1..400 per submit, k..300 bases; long records 5..40 kB
        for o in ops:
            if o["op"].startswith("submit_"):
                assert 1 <= len(o["records"]) <= 400 and all(k <= len(r) <= 300 for r in o["records"])
            if o["op"] == "pieces":
                assert 5000 <= len(o["record"]) <= 40000
    assert set(lm.OP_KINDS) <= kinds, set(lm.OP_KINDS) - kinds
    assert {"set_option:" + n for n in ("algo", "defer_flush", "sc_lo_bits", "sc_grid", "sc_contig_pages", "one_level_max_k", "arena_grow",
                                       "arena_batches", "smallk_old")} <= kinds, kinds
    assert {o["kind"] for k, s in SEEDS for o in fixed_sequence(k, s) if o["op"] == "bad"} == set(lm.KINDS)
    assert set(lm.PATTERNS) <= have13, set(lm.PATTERNS) - have13
    # at most three host copies of a large vector per sequence
    for k, seed in SEEDS:
        if k >= 13:
            assert sum(1 for o in fixed_sequence(k, seed) if o.get("copy")) <= 3


def test_pending_before_follows_the_engine_rules():
    ops = [{"op": "create"}, {"op": "set_option", "init": True, "name": "accum_bytes", "value": 0}, {"op": "submit_host"}, {"op": "submit_device"},
           {"op": "set_option", "name": "algo", "value": 1}, {"op": "submit_host"}, {"op": "set_option", "name": "sc_lo_bits", "value": 9},
           {"op": "set_option", "name": "algo", "value": 2}, {"op": "submit_host"}, {"op": "finish"}, {"op": "finish"}]
    assert lm.pending_before(ops, 14) == [0, 0, 0, 1, 2, 2, 2, 0, 0, 1, 0]
    assert lm.pending_before(ops, 12) == [0] * 11
    ops[1]["value"] = 1 << 20                    # host submits wait in the accumulation buffer: only the device batch is in the arena
    assert lm.pending_before(ops, 14)[:5] == [0, 0, 0, 0, 1]
