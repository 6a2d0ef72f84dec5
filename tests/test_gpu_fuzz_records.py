"""The randomised differential run of the per-record and alignment calls (tests/fuzz_records.py) under the driver: seeded cases of
kdb_minimizers, kdb_record_tables, kdb_score_reads, kdb_align_banded and kdb_align_traceback over their whole parameter ranges, each
compared with the call's CPU restatement and with itself under a shuffle, a subset, another cap and another scratch limit; and
kdb_align_traceback on more tasks than one trip of scan_top_kernel's loop holds (csrc/kdb_align_trace.hip.h).
tests/test_fuzz_records_cpu.py shows, without a device, what the very cases of SEEDED cover.

TIMES, wall, measured on one MI355X (most of a seeded test is the CPU restatement):
    the module alone, 12 tests                    24.5 s
    seeded, per (call, seed) of 20 cases          minimizers 0.23 / 0.11 s, tables 0.07 / 0.08 s, score 4.7 / 1.9 s, align 3.6 / 3.6 s,
                                                  traceback 4.4 / 4.7 s
    524 289 and 1 048 579 tasks, two calls each   0.04 s and 0.07 s
    the whole -m gpu suite                        667 s before this module (1366 tests), 704 s with it and the two designed score tests (1382 tests)
    tests/test_fuzz_records_cpu.py, on the CPU    116 s (13 tests; the alignment cases, restated twice over, are 99 s of it)
The module's budget is a tenth of the suite's time before it, 67 s.  python tests/fuzz_records.py 60 <seed>, once each on two other seeds:
610 and 605 cases, all equal."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import alignment_cases as ac  # noqa: E402
import fuzz_records  # noqa: E402
import minimizer_cases as mc  # noqa: E402
import traceback_cases as tc  # noqa: E402

pytestmark = pytest.mark.gpu

# (call, seed, cases): 200 cases, 40 per call over two seeds
SEEDED = [(call, seed, 20) for call in fuzz_records.CALLS for seed in (101, 202)]
NCASES = sum(n for _, _, n in SEEDED)


@pytest.mark.parametrize("call,seed,ncases", SEEDED)
def test_seeded_fuzz_cases_equal_the_restatements(gpu_engine_cls, call, seed, ncases):
    n, bad = fuzz_records.run_cases(seed, max_cases=ncases, calls=[call], verbose=False)
    assert bad is None, f"case {n} of seed {seed} differs from the restatement of {call}: {bad}"
    assert n == ncases


# ---- more tasks than scan_top_kernel takes in one trip ----

_SCAN = re.search(r"constexpr int SCAN_TPB = (\d+), SCAN_ITEMS = (\d+);", open(os.path.join(fuzz_records.ROOT, "kmerdb_amd", "csrc", "kdb_align_trace.hip.h")).read())
SCAN_BLOCK = int(_SCAN.group(1)) * int(_SCAN.group(2))
SCAN_TOP = int(_SCAN.group(1)) * SCAN_BLOCK    # the tasks of one trip of scan_top_kernel's loop
TINY_BAND = 1
TINY_SCORES = dict(match=2, mismatch=-1, gap_open=-1, gap_extend=-1)


def _tiny_tasks():
    """37 distinct tasks over records of 0 .. 8 residues: copies, copies with one residue more or less, unrelated pairs, empty records,
    both strands, diagonals in and beyond the band -> (queries, refs, [(q, r, d, strand)])"""
    rng = np.random.Generator(np.random.PCG64(524288))
    queries = [mc.random_record(rng, n) for n in (0, 1, 2, 3, 4, 5, 6, 7, 8, 8, 7, 5)]
    refs = [q for q in queries[:9]] + [queries[9][:4] + queries[9][5:], queries[10][:3] + b"G" + queries[10][3:], ac.orient(queries[11], 1)]
    tasks = [(i, i, 0, 0) for i in range(12)] + [(9, 9, 0, 0), (10, 10, 1, 0), (11, 11, 0, 1), (8, 7, 1, 0), (7, 8, -1, 0), (3, 8, 4, 0), (8, 3, -5, 0), (0, 5, 0, 1),
                                                (5, 0, 0, 0), (6, 6, 9, 0), (6, 6, -9, 1), (4, 4, 2 ** 40, 0), (8, 8, 1, 1), (2, 6, 3, 0), (1, 1, 0, 1)]
    tasks += [(int(rng.integers(0, 12)), int(rng.integers(0, 12)), int(rng.integers(-3, 4)), int(rng.integers(0, 2))) for _ in range(37 - len(tasks))]
    assert len(tasks) == 37 and max(len(x) for x in queries + refs) == 8
    return queries, refs, tasks


@pytest.fixture(scope="module")
def tiny(gpu_engine_cls):
    """the distinct tasks, what traceback_cases.trace gives for each, and the output arrays of the largest call, allocated once"""
    from kmerdb_amd import _abi
    queries, refs, tasks = _tiny_tasks()
    traced = [tc.trace(queries[q], refs[r], d, TINY_BAND, strand, **TINY_SCORES) for q, r, d, strand in tasks]
    assert sum(1 for five, _ in traced if five[0] > 0) >= 20 and sum(1 for five, _ in traced if five[0] == 0) >= 5
    assert sum(1 for _, path in traced if any(x & 15 in (tc.OP_I, tc.OP_D) for x in path)) >= 2
    top = 2 * SCAN_TOP + 3
    per_tile = sum(len(path) for _, path in traced)
    outs = dict(score=np.empty(top, dtype=np.int32), nruns=np.empty(top, dtype=np.uint64), runs=np.empty((top // 37 + 1) * per_tile, dtype=np.uint32),
                **{name: np.empty(top, dtype=np.uint32) for name in fuzz_records.FIVE[1:]})
    return dict(lib=_abi.lib(), last_error=_abi.last_error, OK=_abi.KDB_OK, queries=queries, refs=refs, tasks=tasks, traced=traced, outs=outs)


def _tiled_call(tiny, n, scratch_limit):
    """kdb_align_traceback on the 37 tasks tiled to n, into the 0xFF-filled arrays -> (five arrays, nruns, runs up to the total, total)"""
    qb, qo = mc.pack(tiny["queries"])
    rb, ro = mc.pack(tiny["refs"])
    cols = [np.resize(c, n) for c in ac.task_arrays(tiny["tasks"])]          # (np.resize repeats the array)
    outs = tiny["outs"]
    for a in outs.values():
        a.view(np.uint8).fill(0xFF)
    total = ctypes.c_uint64(2 ** 64 - 1)
    rc = tiny["lib"].kdb_align_traceback(0, qb.ctypes.data, qb.size, qo.ctypes.data, len(qo) - 1, rb.ctypes.data, rb.size, ro.ctypes.data, len(ro) - 1,
                                         *(c.ctypes.data for c in cols), n, TINY_BAND, TINY_SCORES["match"], TINY_SCORES["mismatch"], TINY_SCORES["gap_open"],
                                         TINY_SCORES["gap_extend"], scratch_limit, *(outs[name].ctypes.data for name in fuzz_records.FIVE), outs["nruns"].ctypes.data,
                                         outs["runs"].ctypes.data, outs["runs"].size, ctypes.byref(total), None)
    assert rc == tiny["OK"], tiny["last_error"]()
    return [outs[name][:n] for name in fuzz_records.FIVE], outs["nruns"][:n], outs["runs"], int(total.value)


@pytest.mark.parametrize("n", [SCAN_TOP + 1, 2 * SCAN_TOP + 3])
def test_more_tasks_than_one_trip_of_the_top_scan(tiny, n):
    """One chunk of n tasks: scan_top_kernel's loop takes a second (third) trip over the block sums.  Then two chunks cut at a task that is
    no multiple of SCAN_BLOCK: the second chunk's offsets stand on the carry and on block sums that begin in the middle of a block."""
    tasks, traced = tiny["tasks"], tiny["traced"]
    tile = lambda per_task, dtype: np.resize(np.array(per_task, dtype=dtype), n)
    want_five = [tile([five[i] for five, _ in traced], dt) for i, dt in enumerate((np.int32, np.uint32, np.uint32, np.uint32, np.uint32))]
    want_nruns = tile([len(path) for _, path in traced], np.uint64)
    one_tile = np.array([x for _, path in traced for x in path], dtype=np.uint32)
    rest = np.array([x for _, path in traced[:n % 37] for x in path], dtype=np.uint32)
    want_runs = np.concatenate((np.tile(one_tile, n // 37), rest))            # the runs where the exclusive offsets of nruns place them
    sizes = np.resize(np.array([fuzz_records.trace_bytes(len(tiny["queries"][q]), len(tiny["refs"][r]), d, TINY_BAND) for q, r, d, _ in tasks], dtype=np.int64), n)
    used = np.cumsum(sizes)
    assert 100 << 20 < int(used[-1]) < 2 ** 31                                 # a few hundred MB: one chunk under the default limit
    # a limit that ends the first chunk behind task `cut - 1`: the bytes up to there, and the next task holds some
    cut = SCAN_TOP // 2 + 1001 if n == SCAN_TOP + 1 else SCAN_TOP + 1001
    while sizes[cut] == 0:
        cut += 1
    limit = int(used[cut - 1])
    assert cut % SCAN_BLOCK and int(used[-1]) - limit <= limit
    for scratch_limit in (0, limit):
        five, nruns, runs, total = _tiled_call(tiny, n, scratch_limit)
        where = (n, scratch_limit)
        assert total == int(want_nruns.sum()) == want_runs.size, where
        bad = np.flatnonzero(nruns != want_nruns)
        assert bad.size == 0, where + (bad[:8].tolist(),)
        for name, g, x in zip(fuzz_records.FIVE, five, want_five):
            bad = np.flatnonzero(g != x)
            assert bad.size == 0, where + (name, bad[:8].tolist())
        bad = np.flatnonzero(runs[:total] != want_runs)
        assert bad.size == 0, where + (bad[:8].tolist(), int(np.searchsorted(np.cumsum(want_nruns), bad[0], side="right")))
        assert np.all(runs[total:] == 2 ** 32 - 1), where
