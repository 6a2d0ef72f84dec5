"""GPU: kdb_align_traceback -- the banded forward pass with direction stores and the wave-uniform walk over them (csrc/kdb_align_trace.hip.h)
-- against the restatement of tests/traceback_cases.py, and the layers above it: kmerdb_amd.alignment's CIGAR fields and the `alignment`
subcommand's --cigar.

Every output is an integer and compared exactly: the runs, their counts, the total and all five scalars with the restatement, the five
scalars also with kdb_align_banded in the same process.  Every test here fails without kdb_align_traceback: the library does not export
the symbol."""
import contextlib
import ctypes
import io
import os
import re

import numpy as np
import pytest

import alignment_cases as ac
import minimizer_cases as mc
import traceback_cases as tc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONTIGS = os.path.join(ROOT, "tests", "golden", "inputs", "contigs.fa")


def _header_constant(name):
    text = open(os.path.join(ROOT, "include", "kdbhip.h")).read()
    return int(re.search(r"#define\s+%s\s+(\d+)" % name, text).group(1))


S, MAX_BAND, GRID_MAX = _header_constant("KDB_ALIGN_STAGE"), _header_constant("KDB_ALIGN_MAX_BAND"), _header_constant("KDB_ALIGN_GRID_MAX")
FILL32, FILL64 = 2 ** 32 - 1, 2 ** 64 - 1
NAMES = ("score", "qstart", "qend", "rstart", "rend")
FREE = dict(match=1, mismatch=0, gap_open=0, gap_extend=0)
CHEAP = dict(match=3, mismatch=-1, gap_open=-2, gap_extend=-1)
STRICT = dict(match=3, mismatch=-4, gap_open=-2, gap_extend=-1)               # (unrelated sequence does not align, a planted gap is cheap)


@pytest.fixture(scope="module")
def dev(gpu_engine_cls):
    from kmerdb_amd import _abi

    class Dev:
        lib = _abi.lib()
        OK, ARG, BAD = _abi.KDB_OK, _abi.KDB_ERR_ARG, _abi.KDB_ERR_BAD_RESIDUE

        @classmethod
        def raw(cls, q, r, tasks, band=4, match=3, mismatch=-1, gap_open=-10, gap_extend=-1, scratch_limit=0, cap=0, null=(), ntasks=None, nq=None, nr=None,
                q_nbytes=None, r_nbytes=None, ms=False):
            """kdb_align_traceback with the arguments as given -- q, r: (bases, offsets); tasks: the four columns -- and every output filled
            with 0xFF; runs_out holds cap entries and is NULL where cap is 0 -> (status, score, qstart, qend, rstart, rend, nruns, runs, total)"""
            (qb, qo), (rb, ro), (tq, tr, td, ts) = q, r, tasks
            n = int(tq.size) if ntasks is None else ntasks
            outs = [np.full(max(int(tq.size), 1), -1, dtype=np.int32)] + [np.full(max(int(tq.size), 1), FILL32, dtype=np.uint32) for _ in range(4)]
            nruns, runs = np.full(max(int(tq.size), 1), FILL64, dtype=np.uint64), np.full(max(cap, 1), FILL32, dtype=np.uint32)
            total = ctypes.c_uint64(FILL64)
            ptr = lambda name, a: None if name in null or a.size == 0 else a.ctypes.data
            t = ctypes.c_double(-1.0)
            rc = cls.lib.kdb_align_traceback(0, ptr("q_bases", qb), qb.size if q_nbytes is None else q_nbytes, ptr("q_offsets", qo), len(qo) - 1 if nq is None else nq,
                                             ptr("r_bases", rb), rb.size if r_nbytes is None else r_nbytes, ptr("r_offsets", ro), len(ro) - 1 if nr is None else nr,
                                             ptr("task_q", tq), ptr("task_r", tr), ptr("task_diag", td), ptr("task_strand", ts), n, band, match, mismatch, gap_open,
                                             gap_extend, scratch_limit, *(ptr(name, o) for name, o in zip(NAMES, outs)), ptr("nruns", nruns),
                                             None if "runs" in null or (cap == 0 and "runs_given" not in null) else runs.ctypes.data, cap,
                                             None if "total" in null else ctypes.byref(total), ctypes.byref(t) if ms else None)
            if ms:
                assert t.value >= 0.0
            return (rc,) + tuple(outs) + (nruns, runs, total.value)

        @classmethod
        def banded(cls, q, r, tasks, band, **scores):
            from kmerdb_amd import alignment
            return alignment.align_raw(*q, *r, *tasks, band, scores.get("match", 3), scores.get("mismatch", -1), scores.get("gap_open", -10), scores.get("gap_extend", -1))[:5]

        @classmethod
        def packed(cls, q, r, tasks, band, scratch_limit=0, **scores):
            """size, then fill, on packed records; the five scalars are kdb_align_banded's -> (five arrays, nruns, runs)"""
            sized = cls.raw(q, r, tasks, band, scratch_limit=scratch_limit, **scores)
            assert sized[0] == cls.OK, _abi.last_error()
            total = sized[8]
            assert total == int(sized[6].sum()) and np.all(sized[7] == FILL32)
            out = cls.raw(q, r, tasks, band, scratch_limit=scratch_limit, cap=total, **scores)
            assert out[0] == cls.OK and out[8] == total, _abi.last_error()
            _same(out[1:6], sized[1:6], "sizes-only call")
            assert np.array_equal(out[6], sized[6])
            _same(out[1:6], cls.banded(q, r, tasks, band, **scores), "kdb_align_banded")
            return out[1:6], out[6], out[7][:total]

        @classmethod
        def run(cls, queries, refs, tasks, band, scratch_limit=0, **scores):
            """tasks: (q, r, d, strand) over the two lists of records -> (five arrays, [runs per task])"""
            five, nruns, runs = cls.packed(mc.pack(queries), mc.pack(refs), ac.task_arrays(tasks), band, scratch_limit, **scores)
            return five, _split(nruns, runs)
    return Dev


def _split(nruns, runs):
    ends = np.cumsum(nruns.astype(np.int64))
    assert (int(ends[-1]) if ends.size else 0) == runs.size
    return [runs[int(b - n):int(b)].tolist() for n, b in zip(nruns.astype(np.int64), ends)]


def _same(got, want, where=""):
    for name, g, x in zip(NAMES, got, want):
        assert g.dtype == x.dtype and g.shape == x.shape, (where, name, g.dtype, x.dtype, g.shape, x.shape)
        bad = np.flatnonzero(g != x)
        assert bad.size == 0, (where, name, bad[:8].tolist(), g[bad[:8]].tolist(), x[bad[:8]].tolist())


def _check(dev, queries, refs, tasks, band, where="", **scores):
    five, paths = dev.run(queries, refs, tasks, band, **scores)
    want_five, want_paths = tc.run_tasks(queries, refs, tasks, band, **scores)
    _same(five, want_five, (where, band, scores))
    for t, (got, want) in enumerate(zip(paths, want_paths)):
        assert got == want, (where, band, scores, t, tasks[t], tc.text(got), tc.text(want))
    return five, paths


def _gaps(path):
    return [x for x in path if x & 15 in (tc.OP_I, tc.OP_D)]


# ---- every length at which the kernels take another path ----

@pytest.mark.parametrize("strand", [0, 1])
@pytest.mark.parametrize("band", [1, 2, 16, MAX_BAND])
def test_length_ladder(dev, band, strand):
    rng = np.random.Generator(np.random.PCG64(1000 * band + strand))
    lengths = [0, 1, 2, band, band + 1, 2 * band + 1, S - 1, S, S + 1, 2 * S + 7]
    queries = [mc.random_record(rng, n, 0.01) for n in lengths]
    refs = [ac.mutate(rng, ac.orient(q, strand), 0.03, 0.006) for q in queries]          # the partner: a mutated copy of what aligns
    tasks = [(i, i, 0, strand) for i in range(len(lengths))]
    tasks += [(i, j, d, strand) for i, j, d in [(9, 8, 3), (8, 9, -2), (6, 9, S - 1), (3, 7, 0), (1, 9, 2 * S), (0, 9, 0), (9, 0, 0)]]
    five, paths = _check(dev, queries, refs, tasks, band, "ladder", **CHEAP)
    assert five[0][9] > 2 * S and five[0][0] == 0 and paths[0] == [] and len(paths[9]) > 20


@pytest.mark.parametrize("band", [1, 3, 16])
def test_the_group_seam_of_four_steps(dev, band):
    """lengths around one and two groups of 4 steps, on every diagonal of a narrow band: first and last groups that are partly outside
    the task's rows"""
    rng = np.random.Generator(np.random.PCG64(1100 + band))
    queries, refs, tasks = [], [], []
    for n in (3, 4, 5, 7, 8, 9):
        for strand in (0, 1):
            q = mc.random_record(rng, n)
            queries.append(q)
            refs.append(mc.random_record(rng, 3) + ac.orient(q, strand) + mc.random_record(rng, 2))
            tasks += [(len(queries) - 1, len(refs) - 1, d, strand) for d in (3, 2, 4, 3 - band, 3 + band, 0)]
    five, paths = _check(dev, queries, refs, tasks, band, "group seam", **CHEAP)
    for x, n in enumerate((3, 4, 5, 7, 8, 9)):
        assert paths[12 * x] == [(n << 4) | tc.OP_EQ] and paths[12 * x + 6] == [(n << 4) | tc.OP_EQ]      # (d = 3: the copy, end to end)


# ---- diagonals ----

@pytest.mark.parametrize("band", [1, 5, MAX_BAND])
def test_diagonals(dev, band):
    rng = np.random.Generator(np.random.PCG64(1200 + band))
    m, n = 90, 150
    r = mc.random_record(rng, n, 0.01)
    tasks, queries = [], []
    ds = [0, 1, -1, band, -band, -(m - 1), n - 1, -(m - 1) - band, n - 1 + band, -(m - 1) - band - 1, n + band, 2 ** 40, -2 ** 40, 37, -41]
    for d in ds:
        for strand in (0, 1):
            q = bytearray(mc.random_record(rng, m))
            for i in range(m):
                if 0 <= i + d < n and rng.random() < 0.9:
                    q[i] = r[i + d]
            queries.append(ac.orient(bytes(q), strand))
            tasks.append((len(queries) - 1, 0, d, strand))
    five, paths = _check(dev, queries, [r], tasks, band, "diagonals", **CHEAP)
    by_d = dict(zip(ds, zip(five[0][::2].tolist(), paths[::2])))
    assert by_d[0][0] > 100 and by_d[37][0] > 100 and len(by_d[0][1]) > 5
    for d in (-(m - 1) - band - 1, n + band, 2 ** 40, -2 ** 40):              # the first diagonal beyond the band, and far ones: empty tasks, no runs
        assert by_d[d] == (0, [])
    # one cell in the band: the query's last residue against the record's first, the query's first against its last
    one = [(b"CCCCCCCG", b"GTTTTTTT", -7 - band), (b"GCCCCCCC", b"TTTTTTTG", 7 + band)]
    five, paths = dev.run([q for q, _, _ in one], [x for _, x, _ in one], [(0, 0, one[0][2], 0), (1, 1, one[1][2], 0), (0, 0, one[0][2] - 1, 0), (1, 1, one[1][2] + 1, 0)], band)
    assert [g.tolist() for g in five] == [[3, 3, 0, 0], [7, 0, 0, 0], [8, 1, 0, 0], [0, 7, 0, 0], [1, 8, 0, 0]]
    assert paths == [[(1 << 4) | tc.OP_EQ], [(1 << 4) | tc.OP_EQ], [], []]


# ---- seams ----

def test_gaps_on_stage_and_group_seams(dev):
    """In step T lane l is on row T - l; the wave refills its residues every S steps and stores a dword of directions every 4.  Around
    several rows p near both kinds of seam: a gap in either sequence that lies on p -- its placement is unique: the residues on either
    side of it differ from its ends --, found where it was planted."""
    rng = np.random.Generator(np.random.PCG64(1300))
    band = 16
    queries, refs, tasks, want = [], [], [], []
    core = lambda n: bytes(b"ACGT"[(i * 7 + i // 4) % 4] for i in range(n))

    def add(q, r, path):
        queries.append(q)
        refs.append(r)
        tasks.append((len(queries) - 1, len(refs) - 1, 0, 0))
        want.append(path)
    for p in (S - 17, S - 8, S - 4, S - 1, S, S + 3, S + 4, 2 * S - 8, 96, 97, 98, 99, 100):
        x = bytearray(mc.random_record(rng, p + 90))
        x[p - 1], x[p] = ord("A"), ord("C")
        x = bytes(x)
        add(x, x[:p] + b"GTG" + x[p:], [(p, tc.OP_EQ), (3, tc.OP_D), (90, tc.OP_EQ)])              # three reference residues without a partner, after row p - 1
        add(x[:p] + b"GT" + x[p:], x, [(p, tc.OP_EQ), (2, tc.OP_I), (90, tc.OP_EQ)])                # rows p and p + 1 without a partner
    five, paths = _check(dev, queries, refs, tasks, band, "seams", **STRICT)
    for t, path in enumerate(paths):
        assert path == [(n << 4) | op for n, op in want[t]], (t, tc.text(path))


def test_a_path_that_changes_lane_parity_at_a_seam(dev):
    """A deletion of one moves the path from an even diagonal of the band to the odd one of the same lane, the next one to the even
    diagonal of the next lane; an insertion moves it back.  Single gaps a few rows apart, across a stage seam and across group seams."""
    rng = np.random.Generator(np.random.PCG64(1400))
    band = 5
    queries, refs, tasks, want = [], [], [], []
    for p in (S - 8, S - 5, S - 2, 40, 41, 42, 43):
        x = bytearray(mc.random_record(rng, p + 60))
        for at in (p - 1, p + 5, p + 11, p + 17):
            x[at], x[at + 1] = ord("A"), ord("C")
        x = bytes(x)
        ref = x[:p] + b"G" + x[p:p + 6] + b"G" + x[p + 6:p + 12] + b"G" + x[p + 12:]
        queries.append(x[:p + 18] + b"G" + x[p + 18:])
        refs.append(ref)
        tasks.append((len(queries) - 1, len(refs) - 1, 0, 0))
        want.append([(p, 7), (1, 2), (6, 7), (1, 2), (6, 7), (1, 2), (6, 7), (1, 1), (p + 60 - p - 18, 7)])
    five, paths = _check(dev, queries, refs, tasks, band, "lane parity", **STRICT)
    assert paths == [[(n << 4) | op for n, op in w] for w in want]


def test_gap_runs_of_exactly_the_band(dev):
    rng = np.random.Generator(np.random.PCG64(1500))
    for band in (1, 2, 16, MAX_BAND):
        x, y = bytearray(mc.random_record(rng, 120)), bytearray(mc.random_record(rng, 120))
        x[-1], y[0] = ord("A"), ord("C")
        x, y = bytes(x), bytes(y)
        gap = b"G" + b"T" * (band - 1) if band > 1 else b"G"
        gap = gap[:-1] + b"G" if band > 1 else gap
        queries = [x + y, x + gap + y]
        tasks = [(0, 1, 0, 0), (1, 0, 0, 0), (0, 1, band, 0), (1, 0, -band, 0)]
        five, paths = _check(dev, queries, queries, tasks, band, "band edge", match=3, mismatch=-4, gap_open=-2, gap_extend=-1)
        whole = 3 * 240 - 2 - (band - 1)
        assert five[0].tolist() == [whole] * 4
        assert paths[0] == paths[2] == [(120 << 4) | tc.OP_EQ, (band << 4) | tc.OP_D, (120 << 4) | tc.OP_EQ]
        assert paths[1] == paths[3] == [(120 << 4) | tc.OP_EQ, (band << 4) | tc.OP_I, (120 << 4) | tc.OP_EQ]


# ---- ties and extremes ----

def test_ties_and_extremes(dev):
    queries = [b"A" * 70, b"AC" * 40, b"ACGTTTTTACG", b"ACGTACGTAAAAAAAAAAAAACGTACGT", b"AA", b"ACAC", b"AAAAAAAAAA", b"ACGNACG", b"N" * 9,
               b"ACGACGAC" + b"GGACCAGG", b"ACGACGAC" + b"TT" + b"GGACCAGG"]
    refs = [b"A" * 75, b"AC" * 43, b"CA" * 40, b"ACGAAAAAACG", b"ACGTACGTCCCCCCCCCCCCACGTACGT", b"AAA", b"TAA", b"ACACAC", b"AAAA", b"ACGNACG", b"N" * 9,
            b"ACGACGAC" + b"TT" + b"GGACCAGG", b"ACGACGAC" + b"GGACCAGG"]
    pairs = [(0, 0), (1, 1), (1, 2), (2, 3), (3, 4), (4, 5), (4, 6), (5, 7), (6, 8), (6, 0), (7, 9), (8, 10), (0, 8), (1, 7), (9, 11), (10, 12)]
    dear = dict(match=3, mismatch=-4, gap_open=-1, gap_extend=-3)
    for band in (1, 3, 16, MAX_BAND):
        tasks = [(q, r, d, strand) for q, r in pairs for d in (0, 1, -2) for strand in (0, 1)]
        for scores in (ac.DEFAULT, FREE, dict(match=2, mismatch=-1, gap_open=-1, gap_extend=-1), dear, dict(match=2, mismatch=0, gap_open=-1, gap_extend=0),
                       dict(match=127, mismatch=-127, gap_open=-127, gap_extend=-127), dict(match=3, mismatch=-2, gap_open=0, gap_extend=-3)):
            five, paths = _check(dev, queries, refs, tasks, band, "ties", **scores)
            if scores["match"] == 127:
                at = tasks.index((3, 4, 0, 0))                                # two equal segments, nothing worth having between them: the one with the smaller i
                assert [int(g[at]) for g in five] == [8 * 127, 0, 8, 0, 8] and paths[at] == [(8 << 4) | tc.OP_EQ]
            if scores is FREE:
                assert max(sum(x >> 4 for x in p) for p in paths) >= 70       # (all costs 0: the longest walks, from the last row to the first)
            if scores is dear and band >= 3:
                # open > extend: the gap of 2 is two openings, which abut and read as one run
                assert paths[tasks.index((9, 11, 0, 0))] == [(8 << 4) | tc.OP_EQ, (2 << 4) | tc.OP_D, (8 << 4) | tc.OP_EQ]
                assert paths[tasks.index((10, 12, 0, 0))] == [(8 << 4) | tc.OP_EQ, (2 << 4) | tc.OP_I, (8 << 4) | tc.OP_EQ]
                assert int(five[0][tasks.index((9, 11, 0, 0))]) == 46


# ---- chunks, batches, the cap ----

def _short_batch(rng, nq, nr, ntasks, top=40):
    q_lens, r_lens = rng.integers(0, top + 1, size=nq), rng.integers(0, top + 1, size=nr)
    q_lens[rng.random(nq) < 0.05] = 0
    r_lens[rng.random(nr) < 0.05] = 0
    offs = lambda lens: np.concatenate(([0], np.cumsum(lens))).astype(np.uint64)
    letters = np.frombuffer(b"ACGT", dtype=np.uint8)
    qb = letters[rng.integers(0, 4, size=int(q_lens.sum()))].copy()
    qb[rng.random(qb.size) < 0.01] = ord("N")
    rb = letters[rng.integers(0, 2, size=int(r_lens.sum()))].copy()           # (two letters: every pair has something to align)
    qb[rng.random(qb.size) < 0.5] = ord("A")
    tasks = (rng.integers(0, nq, size=ntasks).astype(np.uint32), rng.integers(0, nr, size=ntasks).astype(np.uint32),
             rng.integers(-12, 13, size=ntasks).astype(np.int64), rng.integers(0, 2, size=ntasks).astype(np.uint8))
    tasks[2][rng.random(ntasks) < 0.1] = 100                                  # bands that miss every record
    tasks[2][rng.random(ntasks) < 0.02] = -2 ** 50
    return (qb, offs(q_lens)), (rb, offs(r_lens)), tasks


def _records(x):
    return [x[0][int(a):int(b)].tobytes() for a, b in zip(x[1][:-1], x[1][1:])]


def test_the_result_does_not_depend_on_the_chunks(dev):
    """about 300 tasks -- empty ones, short ones, one of 3 S rows in their midst -- under four scratch limits: a byte (every task a
    chunk), the largest task's bytes, that plus one, and the default"""
    rng = np.random.Generator(np.random.PCG64(1600))
    band = 16
    long_q = mc.random_record(rng, 3 * S, 0.002)
    long_r = mc.random_record(rng, 200) + ac.mutate(rng, long_q, 0.02, 0.004) + mc.random_record(rng, 100)
    q, r, tasks = _short_batch(rng, 100, 80, 300)
    queries, refs = _records(q) + [long_q], _records(r) + [long_r]
    short = list(zip(*(t.tolist() for t in tasks)))
    every = short[:140] + [(100, 80, 200, 0)] + short[140:]
    largest = 256 * -(-(3 * S + band) // 4)
    scores = dict(match=2, mismatch=-1, gap_open=-1, gap_extend=-1)
    first = dev.run(queries, refs, every, band, 0, **scores)
    assert len(first[1][140]) > 30 and sum(1 for p in first[1] if not p) > 30 and sum(1 for p in first[1] if _gaps(p)) > 30
    want = tc.run_tasks(queries, refs, every, band, **scores)
    _same(first[0], want[0], "chunks")
    assert first[1] == want[1]
    for limit in (1, largest, largest + 1):
        five, paths = dev.run(queries, refs, every, band, limit, **scores)
        _same(five, first[0], ("limit", limit))
        assert paths == first[1], limit


def test_a_tasks_runs_do_not_depend_on_the_batch(dev):
    rng = np.random.Generator(np.random.PCG64(1700))
    band = 9
    q, r, tasks = _short_batch(rng, 50, 50, 90)
    queries, refs = _records(q), _records(r)
    others = list(zip(*(t.tolist() for t in tasks)))
    x = mc.random_record(rng, S + 100, 0.01)
    for mine_q, mine_r, d, strand in [(x, ac.mutate(rng, x, 0.05, 0.01), 0, 0), (ac.orient(x[:200], 1), x, 0, 1), (b"A" * 40, b"A" * 50, 3, 0)]:
        task = (len(queries), len(refs), d, strand)
        want_five, want_path = tc.trace(mine_q, mine_r, d, band, strand, **CHEAP)
        assert want_five[0] > 0
        for place in (0, 17, len(others)):                                    # first, in the middle, last
            five, paths = dev.run(queries + [mine_q], refs + [mine_r], others[:place] + [task] + others[place:], band, **CHEAP)
            assert tuple(int(g[place]) for g in five) == want_five and paths[place] == want_path, place
        five, paths = dev.run([mine_q], [mine_r], [(0, 0, d, strand)], band, **CHEAP)                      # alone
        assert tuple(int(g[0]) for g in five) == want_five and paths == [want_path]


def test_twenty_thousand_short_tasks(dev):
    """more tasks than the largest grid has waves; the restatement on a seeded sample of 500, the scalars of all against kdb_align_banded"""
    n = 20000
    assert n > 4 * GRID_MAX
    rng = np.random.Generator(np.random.PCG64(20000))
    q, r, tasks = _short_batch(rng, 3000, 2000, n, top=30)
    scores = dict(match=2, mismatch=-1, gap_open=-1, gap_extend=-1)
    five, nruns, runs = dev.packed(q, r, tasks, 3, **scores)
    paths = _split(nruns, runs)
    queries, refs = _records(q), _records(r)
    sample = sorted(set(rng.integers(0, n, size=500).tolist()) | {0, 1, 4 * GRID_MAX - 1, 4 * GRID_MAX, 4 * GRID_MAX + 1, n - 1})
    gaps = 0
    for t in sample:
        want_five, want_path = tc.trace(queries[tasks[0][t]], refs[tasks[1][t]], int(tasks[2][t]), 3, int(tasks[3][t]), **scores)
        assert tuple(int(g[t]) for g in five) == want_five and paths[t] == want_path, t
        gaps += bool(_gaps(want_path))
    assert gaps > 50 and 0.5 * n < np.count_nonzero(five[0]) < 0.9 * n
    assert np.array_equal(nruns > 0, five[0] > 0)


def test_the_cap_protocol(dev):
    rng = np.random.Generator(np.random.PCG64(1800))
    q, r, tasks = _short_batch(rng, 40, 40, 120)
    sized = dev.raw(q, r, tasks, 5, **CHEAP)                                   # sizes alone: cap = 0, runs_out = NULL
    total = sized[8]
    assert sized[0] == dev.OK and total == int(sized[6].sum()) > 200 and np.all(sized[7] == FILL32)
    short = dev.raw(q, r, tasks, 5, cap=total - 1, **CHEAP)                    # one entry too few: the array stays as it was, the rest is written
    assert short[0] == dev.OK and short[8] == total and np.all(short[7] == FILL32) and np.array_equal(short[6], sized[6])
    _same(short[1:6], sized[1:6], "cap = total - 1")
    full = dev.raw(q, r, tasks, 5, cap=total, **CHEAP)
    assert full[0] == dev.OK and full[8] == total and not np.any(full[7] == FILL32) and np.array_equal(full[6], sized[6])
    roomy = dev.raw(q, r, tasks, 5, cap=total + 7, ms=True, **CHEAP)           # more room than needed: the entries behind the total stay
    assert roomy[0] == dev.OK and np.array_equal(roomy[7][:total], full[7]) and np.all(roomy[7][total:] == FILL32)
    want = tc.run_tasks(_records(q), _records(r), list(zip(*(t.tolist() for t in tasks))), 5, **CHEAP)
    assert _split(full[6], full[7]) == want[1]
    _same(full[1:6], want[0], "cap = total")
    # nothing aligns: a total of 0, and an array of no entries may be NULL
    none = dev.raw(mc.pack([b"AAAA"]), mc.pack([b"CCCC"]), ac.task_arrays([(0, 0, 0, 0)]), 5)
    assert none[0] == dev.OK and none[8] == 0 and none[6].tolist() == [0]


# ---- one long path ----

def test_a_long_path_with_gaps_beyond_row_65536(dev):
    """70 000 rows, 137 stages, 17 500 groups: a copy of the reference with a deletion of 3 and an insertion of 2 planted beyond row
    2^16, each between residues that differ from the gap's ends, so that the path is known by hand"""
    rng = np.random.Generator(np.random.PCG64(70000))
    n, a, b = 70000, (1 << 16) + 123, (1 << 16) + 2001
    x = bytearray(mc.random_record(rng, n))
    x[a - 1], x[a], x[a + 1], x[a + 2], x[a + 3] = b"ACGCA"                    # the reference residues a .. a + 2 (CGC) have no partner: A | A on either side
    x[b - 1], x[b] = b"AC"
    x = bytes(x)
    q = x[:a] + x[a + 3:b] + b"GT" + x[b:]                                     # ... and GT between an A and a C has none in the reference
    band, d = 8, 300
    ref = mc.random_record(rng, d) + x + mc.random_record(rng, 50)
    for strand in (0, 1):
        five, paths = dev.run([b"ACGT", ac.orient(q, strand)], [b"GATTACA", ref], [(1, 1, d, strand)], band, **STRICT)
        path, = paths
        score, qstart, qend, rstart, rend = (int(g[0]) for g in five)
        assert path == [(a << 4) | tc.OP_EQ, (3 << 4) | tc.OP_D, ((b - a - 3) << 4) | tc.OP_EQ, (2 << 4) | tc.OP_I, ((n - b) << 4) | tc.OP_EQ], tc.text(path)
        assert (qstart, qend, rstart, rend) == (0, n - 1, d, d + n) and score == 3 * (n - 3) - 4 - 3
        assert tc.spans(path) == (qend - qstart, rend - rstart) and tc.rescore(path, **STRICT) == score


# ---- refusals ----

def _untouched(out):
    return np.all(out[1] == -1) and all(np.all(o == FILL32) for o in out[2:6]) and np.all(out[6] == FILL64) and np.all(out[7] == FILL32) and out[8] == FILL64


def test_refusals_by_status(dev):
    q, r = mc.pack([b"ACGTACGTAC", b"ACGTNACGT"]), mc.pack([b"ACGTACGTACGGT"])
    tasks = ac.task_arrays([(0, 0, 0, 0), (1, 0, 1, 1)])
    ok = lambda **kw: dev.raw(q, r, tasks, **{"cap": 8, **kw})
    assert ok()[0] == dev.OK and not _untouched(ok()) and 2 <= ok()[8] <= 8
    for kw in (dict(band=0), dict(band=MAX_BAND + 1), dict(band=-1), dict(match=0), dict(match=128), dict(match=-3), dict(mismatch=1), dict(mismatch=-128),
               dict(gap_open=1), dict(gap_open=-128), dict(gap_extend=1), dict(gap_extend=-128)):
        out = ok(**kw)
        assert out[0] == dev.ARG and _untouched(out), kw
        assert ok(ntasks=0, **kw)[0] == dev.ARG, kw                            # (the scalars are checked even where there is nothing to do)
    assert ok(band=MAX_BAND, match=127, mismatch=-127, gap_open=-127, gap_extend=-127)[0] == dev.OK and ok(mismatch=0, gap_open=0, gap_extend=0)[0] == dev.OK
    for null in ("q_bases", "q_offsets", "r_bases", "r_offsets", "task_q", "task_r", "task_diag", "task_strand") + NAMES + ("nruns", "total", "runs"):
        out = ok(null=(null,))
        assert out[0] == dev.ARG and _untouched(out), null
    assert ok(null=("total",), ntasks=0)[0] == dev.ARG and ok(null=("runs",), ntasks=0)[0] == dev.ARG
    bad_offsets = lambda o: (q[0], np.array(o, dtype=np.uint64))
    for o in ([1, 10, 19], [0, 10, 18], [0, 12, 11, 19], [0, 25, 19]):
        assert dev.raw(bad_offsets(o), r, tasks)[0] == dev.ARG, o
        assert dev.raw(r, bad_offsets(o), ac.task_arrays([(0, 0, 0, 0)]))[0] == dev.ARG, o
    for bad in ([(2, 0, 0, 0)], [(0, 1, 0, 0)], [(0, 0, 0, 0), (0, 0, 0, 2)], [(0, 0, 0, 255)], [(2 ** 32 - 1, 0, 0, 0)]):
        out = dev.raw(q, r, ac.task_arrays(bad), cap=8)
        assert out[0] == dev.ARG and _untouched(out), bad
    assert ok(q_nbytes=(1 << 30) + 1)[0] == dev.ARG and ok(r_nbytes=(1 << 30) + 1)[0] == dev.ARG and ok(ntasks=(1 << 26) + 1)[0] == dev.ARG
    assert ok(nq=0)[0] == dev.ARG and ok(nr=0)[0] == dev.ARG
    long_query = (np.full((1 << 20) + 1, ord("A"), dtype=np.uint8), np.array([0, (1 << 20) + 1], dtype=np.uint64))
    out = dev.raw(long_query, r, ac.task_arrays([(0, 0, 0, 0)]), cap=8)
    assert out[0] == dev.ARG and _untouched(out)
    # nothing to do is no error: the total is 0 and nothing else is written
    out = ok(ntasks=0)
    assert out[0] == dev.OK and out[8] == 0 and np.all(out[1] == -1) and np.all(out[6] == FILL64) and np.all(out[7] == FILL32)
    assert dev.raw(q, r, ac.task_arrays([]))[0] == dev.OK
    # empty buffers may be NULL: every task then gives zeros and no runs
    empty = (np.zeros(0, dtype=np.uint8), np.zeros(3, dtype=np.uint64))
    for out in (dev.raw(empty, r, ac.task_arrays([(0, 0, 0, 0), (1, 0, 0, 1)]), cap=4), dev.raw(q, empty, tasks, cap=4)):
        assert out[0] == dev.OK and all(o.tolist() == [0, 0] for o in out[1:7]) and out[8] == 0 and np.all(out[7] == FILL32)
    from kmerdb_amd import alignment
    with pytest.raises(ValueError):
        alignment.align_tasks_cigar(b"ACGTRACGT", [0, 9], b"ACGT", [0, 4], [0], [0], [0], [0])


def test_bad_residues_leave_the_outputs_untouched(dev):
    good = b"ACGTNACGTACGTTGCA" * 3
    tasks = ac.task_arrays([(0, 0, 0, 0), (2, 1, 0, 1), (1, 2, 2, 0)])
    for bad in (b"a", b"R", b"\x00"):
        for at in (0, len(good) - 1):
            rec = good[:at] + bad + good[at + 1:]
            for q, r in [([good, good, rec], [good, good, good]), ([good, good, good], [rec, good, good])]:
                out = dev.raw(mc.pack(q), mc.pack(r), tasks, cap=64)
                assert out[0] == dev.BAD and _untouched(out), (bad, at)
    out = dev.raw(mc.pack([good] * 3), mc.pack([good] * 3), tasks, cap=64)
    assert out[0] == dev.OK and out[1][0] > 100 and out[8] >= 3


def test_bad_arguments_raise_before_the_device_is_touched(dev, monkeypatch):
    from kmerdb_amd import alignment, distance, minimizer

    def touched(*a, **kw):
        raise AssertionError("the device was asked")
    monkeypatch.setattr(alignment, "align_raw", touched)
    monkeypatch.setattr(alignment, "traceback_raw", touched)
    monkeypatch.setattr(minimizer, "minimizers_raw", touched)
    monkeypatch.setattr(distance, "_require_device", touched)
    good = dict(q_bases=b"ACGTACGTAC", q_offsets=[0, 10], r_bases=b"ACGTACGTACGT", r_offsets=[0, 12], task_q=[0], task_r=[0], task_diag=[0], task_strand=[0])
    for change, err in [(dict(band=0), ValueError), (dict(band=64), ValueError), (dict(band=True), TypeError), (dict(match=0), ValueError), (dict(mismatch=1), ValueError),
                        (dict(gap_extend=0.5), TypeError), (dict(q_bases="ACGT"), TypeError), (dict(q_offsets=[0, 9]), ValueError), (dict(r_offsets=[1, 12]), ValueError),
                        (dict(task_q=[1]), ValueError), (dict(task_strand=[2]), ValueError), (dict(task_diag=[0.5]), TypeError), (dict(task_q=[0, 0]), ValueError),
                        (dict(scratch_limit=0), ValueError), (dict(scratch_limit=-5), ValueError), (dict(scratch_limit=1.5), TypeError), (dict(scratch_limit=True), TypeError)]:
        with pytest.raises(err):
            alignment.align_tasks_cigar(**{**good, **change})
    for kw, err in [(dict(k=0), ValueError), (dict(band=64), ValueError), (dict(match=1.5), TypeError)]:
        with pytest.raises(err):
            list(alignment.align_file(CONTIGS, CONTIGS, cigar=True, **kw))
    with pytest.raises(AssertionError):
        alignment.align_tasks_cigar(**good)


def test_align_tasks_cigar(dev):
    """the Python call: size-then-fill from a guess that is too small, and the scratch limit"""
    from kmerdb_amd import alignment
    rng = np.random.Generator(np.random.PCG64(1900))
    x = mc.random_record(rng, 400)
    y = ac.mutate(rng, x, 0.15, 0.05)                                          # more runs than the first call has room for
    args = (x + x[:50], [0, 400, 450], y, [0, len(y)], [0, 1], [0, 0], [0, 0], [0, 0])
    want = tc.run_tasks([x, x[:50]], [y], [(0, 0, 0, 0), (1, 0, 0, 0)], 16, **CHEAP)
    assert len(want[1][0]) > alignment.RUNS_GUESS * 2
    for limit in (None, 1, 1 << 20):
        got = alignment.align_tasks_cigar(*args, band=16, scratch_limit=limit, **CHEAP)
        _same(got[:5], want[0], "align_tasks_cigar")
        assert got[5].dtype == np.uint64 and got[6].dtype == np.uint32 and _split(got[5], got[6]) == want[1]
    _same(alignment.align_tasks(*args, band=16, **CHEAP), want[0], "align_tasks")
    empty = alignment.align_tasks_cigar(*args[:4], [], [], [], [])
    assert all(a.size == 0 for a in empty) and len(empty) == 7


# ---- the pipeline ----

PIPELINE_SEED = 33


def _synthetic(seed):
    """three records of 20-30 kbp, the second holding 2 kbp of the first; 300 reads of 100-250 bp from both strands -- a third as they
    are, a third with substitutions, a third with one or two short indels --, ten that belong nowhere and twelve with 12 N before and 5 N
    behind a piece of 150 -> (refs, reads, the names and lengths of the error-free reads)"""
    rng = np.random.Generator(np.random.PCG64(seed))
    refs = [mc.random_record(rng, int(n)) for n in rng.integers(20000, 30001, size=3)]
    refs[1] = refs[1][:7000] + refs[0][3000:5000] + refs[1][9000:]
    reads, clean = [], {}
    for i in range(300):
        ref, n = int(rng.integers(0, 3)), int(rng.integers(100, 251))
        a = int(rng.integers(0, len(refs[ref]) - n))
        read = refs[ref][a:a + n]
        if i % 3 == 1:
            read = ac.mutate(rng, read, 0.03, 0.0)
        elif i % 3 == 2:
            for _ in range(int(rng.integers(1, 3))):
                p, g = int(rng.integers(20, len(read) - 20)), int(rng.integers(1, 4))
                read = read[:p] + (mc.random_record(rng, g) + read[p:] if rng.random() < 0.5 else read[p + g:])
        strand = int(rng.integers(0, 2))
        if i % 3 == 0:
            clean["read%d" % i] = n
        reads.append(("read%d" % i, ac.orient(read, strand)))
    reads += [("noise%d" % i, mc.random_record(rng, int(rng.integers(100, 251)))) for i in range(10)]
    for i in range(12):
        a = int(rng.integers(0, len(refs[i % 3]) - 150))
        reads.append(("clip%d" % i, ac.orient(b"N" * 12 + refs[i % 3][a:a + 150] + b"N" * 5, i & 1)))
    return [("ref%d" % i, s) for i, s in enumerate(refs)], reads, clean


def _write_fasta(path, records):
    with open(path, "w") as f:
        for name, s in records:
            f.write(">{0}\n".format(name))
            for a in range(0, len(s), 70):
                f.write(s[a:a + 70].decode() + "\n")


def _cigar(path, qstart, qend, m, eqx):
    """a SAM CIGAR written out on its own: clips from the oriented coordinates, = and X as they are or as M"""
    ops = [(qstart, "S")] + [(x >> 4, tc.CHAR[x & 15] if eqx or x & 15 in (tc.OP_I, tc.OP_D) else "M") for x in path] + [(m - qend, "S")]
    merged = []
    for n, ch in ops:
        if n == 0:
            continue
        if merged and merged[-1][1] == ch:
            merged[-1] = (merged[-1][0] + n, ch)
        else:
            merged.append((n, ch))
    return "".join("%d%s" % x for x in merged)


def _pipeline(refs, queries, k, w, order, band, eqx, **scores):
    """alignment_cases.pipeline with every candidate traced -> align_file's tuples with cigar=True"""
    table = ac.sketch([s for _, s in refs], k, w, order, 50)
    lines = []
    for qname, q in queries:
        cands = ac.seed(table, q, k, w, order, band)
        traced = [tc.trace(q, refs[ref][1], diag, band, rel, **scores) for ref, rel, diag, _ in cands]
        for found in ac.finish(len(q), cands, [five for five, _ in traced]):
            qs, qe, rel, ref, rs, re_, score, seeds, diag = found
            # the best-ranked candidate that gives this result
            five, path = next(t for c, t in zip(cands, traced) if c[:2] == (ref, rel) and t[0][0] == score and (t[0][3], t[0][4]) == (rs, re_) and
                              ((len(q) - t[0][2], len(q) - t[0][1]) if rel else (t[0][1], t[0][2])) == (qs, qe))
            nm = sum(x >> 4 for x in path if x & 15 != tc.OP_EQ)
            lines.append((qname, len(q), qs, qe, rel, refs[ref][0], len(refs[ref][1]), rs, re_, score, seeds, diag, _cigar(path, five[1], five[2], len(q), eqx), nm))
    return lines


def test_the_pipeline_with_cigars(dev, tmp_path):
    from kmerdb_amd import alignment
    refs, reads, clean = _synthetic(PIPELINE_SEED)
    _write_fasta(tmp_path / "ref.fa", refs)
    _write_fasta(tmp_path / "reads.fa", reads)
    ref, query = str(tmp_path / "ref.fa"), str(tmp_path / "reads.fa")
    k, w, band = 15, 10, 8
    scores = dict(match=3, mismatch=-3, gap_open=-4, gap_extend=-1)            # (a gap that pays: the reads with indels align across them)
    want = _pipeline(refs, reads, k, w, mc.HASHED, band, True, **scores)
    got = list(alignment.align_file(ref, query, k=k, w=w, order="hashed", band=band, cigar=True, eqx=True, **scores))
    assert got == want
    assert list(alignment.align_file(ref, query, k=k, w=w, order="hashed", band=band, cigar=True, eqx=True, batch_residues=5000, **scores)) == want
    plain = list(alignment.align_file(ref, query, k=k, w=w, order="hashed", band=band, cigar=True, **scores))
    assert plain == _pipeline(refs, reads, k, w, mc.HASHED, band, False, **scores)
    # without cigar nothing changes: the same tuples, two fields shorter
    assert list(alignment.align_file(ref, query, k=k, w=w, order="hashed", band=band, **scores)) == [x[:12] for x in want]
    best = {}
    for eq, m in zip(got, plain):
        best.setdefault(eq[0], (eq, m))
    assert len(clean) == 100
    for name, n in clean.items():                                             # an error-free read: its whole length, matched
        assert best[name][0][12:] == ("%d=" % n, 0) and best[name][1][12:] == ("%dM" % n, 0), name
    assert {x[4] for x in got} == {0, 1} and sum(1 for x in got if "I" in x[12]) > 20 and sum(1 for x in got if "D" in x[12]) > 20
    assert sum(1 for x in got if "X" in x[12]) > 80
    # what is no part of the alignment is clipped, along the oriented query: the 12 residues come first on either strand
    for i in range(12):
        eq, m = best["clip%d" % i]
        assert (eq[4], eq[12], eq[13], m[12], m[13]) == (i & 1, "12S150=5S", 0, "12S150M5S", 0), (i, eq)
    only = list(alignment.align_file(ref, query, k=k, w=w, order="hashed", band=band, best_only=True, cigar=True, eqx=True, **scores))
    assert only == [best[name][0] for name, _ in reads if name in best]


# ---- the subcommand ----

def _main(argv):
    from kmerdb_amd import profile
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        assert profile.main(argv) == 0
    return out.getvalue()


def test_the_subcommand_with_cigars(dev, tmp_path):
    from kmerdb_amd import alignment
    rng = np.random.Generator(np.random.PCG64(2100))
    contigs = [(rid, s.upper().encode()) for rid, s in mc.read_fasta(CONTIGS)]
    reads = []
    for i in range(40):
        rid, s = contigs[0] if i & 1 else contigs[3]
        a = int(rng.integers(0, len(s) - 200))
        read = ac.mutate(rng, s[a:a + int(rng.integers(90, 200))].replace(b"N", b"A"), 0.02 if i % 4 < 2 else 0.0, 0.004 if i % 4 < 2 else 0.0)
        reads.append(("r%d" % i, ac.orient(read, (i >> 1) & 1)))
    reads += [("nowhere%d" % i, mc.random_record(rng, 150)) for i in range(5)]
    _write_fasta(tmp_path / "reads.fa", reads)
    query = str(tmp_path / "reads.fa")
    kw = dict(k=13, w=8, order="hashed", band=12, gap_open=-6)
    argv = ["alignment", "-k", "13", "-w", "8", "--order", "hashed", "--band", "12", "--gap-open", "-6", CONTIGS, query]
    without = [alignment.format_line(x) for x in alignment.align_file(CONTIGS, query, **kw)]
    assert len({line.split("\t")[0] for line in without}) == 40 and all(len(line.rstrip("\n").split("\t")) == 12 for line in without)
    assert _main(argv) == "".join(without)                                    # without --cigar: what cigar=False gives, byte for byte
    for eqx in (False, True):
        lines = [alignment.format_line(x) for x in alignment.align_file(CONTIGS, query, cigar=True, eqx=eqx, **kw)]
        assert [line.rstrip("\n").rsplit("\t", 2)[0] + "\n" for line in lines] == without
        assert _main(argv[:1] + ["--cigar"] + (["--eqx"] if eqx else []) + argv[1:]) == "".join(lines)
        for line in lines:
            f = line.rstrip("\n").split("\t")
            ops = re.findall(r"(\d+)([MIDSX=])", f[12])
            assert "".join(a + b for a, b in ops) == f[12] and ("M" in f[12]) != eqx
            assert sum(int(a) for a, b in ops if b in "MIS=X") == int(f[1]) and sum(int(a) for a, b in ops if b in "MD=X") == int(f[8]) - int(f[7])
            assert sum(int(a) for a, b in ops if b in "MI=X") == int(f[3]) - int(f[2]) and int(f[13]) >= sum(int(a) for a, b in ops if b in "ID")
    out = tmp_path / "out.tsv"
    assert _main(argv[:1] + ["--cigar", "--eqx", "-o", str(out)] + argv[1:]) == "" and out.read_text() == "".join(lines)
