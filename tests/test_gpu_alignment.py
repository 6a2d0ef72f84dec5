"""GPU: kdb_align_banded -- banded local alignments with affine gaps, a wave per task (csrc/kdb_align.hip.h) -- against the restatement of
tests/alignment_cases.py, and the layers above it: kmerdb_amd.alignment and the `alignment` subcommand.

Every output is an integer and compared exactly, all five of them.  Every test here fails without kdb_align_banded: the library does not
export the symbol and the module is not there."""
import contextlib
import ctypes
import io
import os
import re

import numpy as np
import pytest

import alignment_cases as ac
import minimizer_cases as mc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONTIGS = os.path.join(ROOT, "tests", "golden", "inputs", "contigs.fa")


def _header_constant(name):
    text = open(os.path.join(ROOT, "include", "kdbhip.h")).read()
    return int(re.search(r"#define\s+%s\s+(\d+)" % name, text).group(1))


S, MAX_BAND, GRID_MAX = _header_constant("KDB_ALIGN_STAGE"), _header_constant("KDB_ALIGN_MAX_BAND"), _header_constant("KDB_ALIGN_GRID_MAX")
FILL32 = 2 ** 32 - 1
NAMES = ("score", "qstart", "qend", "rstart", "rend")
FREE = dict(match=1, mismatch=0, gap_open=0, gap_extend=0)


@pytest.fixture(scope="module")
def dev(gpu_engine_cls):
    from kmerdb_amd import _abi

    class Dev:
        lib = _abi.lib()
        OK, ARG, BAD = _abi.KDB_OK, _abi.KDB_ERR_ARG, _abi.KDB_ERR_BAD_RESIDUE

        @classmethod
        def raw(cls, q, r, tasks, band=4, match=3, mismatch=-1, gap_open=-10, gap_extend=-1, null=(), ntasks=None, nq=None, nr=None, q_nbytes=None, r_nbytes=None,
                ms=False):
            """kdb_align_banded with the arguments as given -- q, r: (bases, offsets); tasks: the four columns -- and every output filled
            with 0xFF -> (status, score, qstart, qend, rstart, rend)"""
            (qb, qo), (rb, ro), (tq, tr, td, ts) = q, r, tasks
            n = int(tq.size) if ntasks is None else ntasks
            outs = [np.full(max(int(tq.size), 1), -1, dtype=np.int32)] + [np.full(max(int(tq.size), 1), FILL32, dtype=np.uint32) for _ in range(4)]
            ptr = lambda name, a: None if name in null or a.size == 0 else a.ctypes.data
            t = ctypes.c_double(-1.0)
            rc = cls.lib.kdb_align_banded(0, ptr("q_bases", qb), qb.size if q_nbytes is None else q_nbytes, ptr("q_offsets", qo), len(qo) - 1 if nq is None else nq,
                                          ptr("r_bases", rb), rb.size if r_nbytes is None else r_nbytes, ptr("r_offsets", ro), len(ro) - 1 if nr is None else nr,
                                          ptr("task_q", tq), ptr("task_r", tr), ptr("task_diag", td), ptr("task_strand", ts), n, band, match, mismatch, gap_open,
                                          gap_extend, *(ptr(name, o) for name, o in zip(NAMES, outs)), ctypes.byref(t) if ms else None)
            if ms:
                assert t.value >= 0.0
            return (rc,) + tuple(outs)

        @classmethod
        def run(cls, queries, refs, tasks, band, **scores):
            """tasks: (q, r, d, strand) over the two lists of records -> the five arrays"""
            out = cls.raw(mc.pack(queries), mc.pack(refs), ac.task_arrays(tasks), band, **scores)
            assert out[0] == cls.OK, _abi.last_error()
            return out[1:]
    return Dev


def _same(got, want, where=""):
    for name, g, x in zip(NAMES, got, want):
        assert g.dtype == x.dtype and g.shape == x.shape, (where, name, g.dtype, x.dtype, g.shape, x.shape)
        bad = np.flatnonzero(g != x)
        assert bad.size == 0, (where, name, bad[:8].tolist(), g[bad[:8]].tolist(), x[bad[:8]].tolist())


def _check(dev, queries, refs, tasks, band, where="", **scores):
    got = dev.run(queries, refs, tasks, band, **scores)
    _same(got, ac.run_tasks(queries, refs, tasks, band, **scores), (where, band, scores))
    return got


# ---- every length at which the kernel takes another path ----

@pytest.mark.parametrize("strand", [0, 1])
@pytest.mark.parametrize("band", [1, 2, 16, MAX_BAND])
def test_length_ladder(dev, band, strand):
    rng = np.random.Generator(np.random.PCG64(100 * band + strand))
    lengths = [0, 1, 2, band, band + 1, 2 * band + 1, S - 1, S, S + 1, 2 * S + 7]
    queries = [mc.random_record(rng, n, 0.01) for n in lengths]
    refs = [ac.mutate(rng, ac.orient(q, strand), 0.03, 0.004) for q in queries]          # the partner: a mutated copy of what aligns
    tasks = [(i, i, 0, strand) for i in range(len(lengths))]
    tasks += [(i, j, d, strand) for i, j, d in [(9, 8, 3), (8, 9, -2), (6, 9, S - 1), (9, 6, -S), (3, 7, 0), (7, 3, 1), (1, 9, 2 * S), (9, 1, -5), (0, 9, 0), (9, 0, 0)]]
    got = _check(dev, queries, refs, tasks, band, "ladder")
    assert got[0][9] > 2 * S and got[0][0] == 0                               # (the longest pair aligns end to end, or nearly; the empty one not at all)


# ---- diagonals ----

@pytest.mark.parametrize("band", [1, 5, MAX_BAND])
def test_diagonals(dev, band):
    rng = np.random.Generator(np.random.PCG64(200 + band))
    m, n = 90, 150
    r = mc.random_record(rng, n, 0.01)
    tasks, queries = [], []
    ds = [0, 1, -1, band, -band, -(m - 1), n - 1, -(m - 1) - band, n - 1 + band, -(m - 1) - band - 1, n + band, -m, n, 10 ** 9, -10 ** 9, 2 ** 40, -2 ** 40,
          2 ** 63 - 1, -2 ** 63, 2 ** 31, -2 ** 31, 2 ** 32 - 70, 37, -41]
    for d in ds:
        for strand in (0, 1):
            # a query that matches the record along the diagonal d (where that meets it), with a few errors
            q = bytearray(mc.random_record(rng, m))
            for i in range(m):
                if 0 <= i + d < n and rng.random() < 0.9:
                    q[i] = r[i + d]
            queries.append(ac.orient(bytes(q), strand))
            tasks.append((len(queries) - 1, 0, d, strand))
    score = _check(dev, queries, [r], tasks, band, "diagonals")[0]
    by_d = dict(zip(ds, score[::2].tolist()))
    assert by_d[0] > 100 and by_d[37] > 100 and by_d[-41] > 50
    assert all(by_d[d] == 0 for d in (-(m - 1) - band - 1, n + band, 10 ** 9, -10 ** 9, 2 ** 40, -2 ** 40, 2 ** 63 - 1, -2 ** 63, 2 ** 31, -2 ** 31, 2 ** 32 - 70))
    # one cell in the band: the query's last residue against the record's first, the query's first against its last
    one = [(b"CCCCCCCG", b"GTTTTTTT", -7 - band), (b"GCCCCCCC", b"TTTTTTTG", 7 + band)]
    got = dev.run([q for q, _, _ in one], [x for _, x, _ in one], [(0, 0, one[0][2], 0), (1, 1, one[1][2], 0), (0, 0, one[0][2] - 1, 0), (1, 1, one[1][2] + 1, 0)], band)
    assert [g.tolist() for g in got] == [[3, 3, 0, 0], [7, 0, 0, 0], [8, 1, 0, 0], [0, 7, 0, 0], [1, 8, 0, 0]]


# ---- stage seams ----

def test_paths_across_a_stage_seam(dev):
    """The wave refills its residues every S steps; in step T lane l is on row T - l, so the lanes cross a seam on the rows S - 63 .. S.
    Around each of several such rows p: a gap that lies on p (in either sequence), the best cell on p, the origin on p - 1 and on p."""
    rng = np.random.Generator(np.random.PCG64(300))
    band = 16
    queries, refs, tasks = [], [], []

    def add(q, r, d=0):
        queries.append(q)
        refs.append(r)
        tasks.append((len(queries) - 1, len(refs) - 1, d, 0))
    for p in (S - 17, S - 9, S - 8, S - 7, S - 1, S, 2 * S - 8):
        q = mc.random_record(rng, p + 90)
        add(q, q[:p] + b"ACG" + q[p:])                                        # three reference residues without a partner, after row p - 1
        add(q, q[:p] + q[p + 2:])                                             # rows p and p + 1 without a partner
        add(q[:p + 1] + mc.random_record(rng, 60), q[:p + 1] + mc.random_record(rng, 60))       # the best cell is on row p
        add(mc.random_record(rng, p - 1) + q[p - 1:], mc.random_record(rng, p - 1) + q[p - 1:])  # the origin is on row p - 1
        add(mc.random_record(rng, p) + q[p:], mc.random_record(rng, p + 5) + q[p:], 5)          # ... on row p, five columns on
    got = _check(dev, queries, refs, tasks, band, "seams", match=3, mismatch=-4, gap_open=-10, gap_extend=-1)      # (-4: unrelated sequence does not align)
    for x, p in enumerate((S - 17, S - 9, S - 8, S - 7, S - 1, S, 2 * S - 8)):
        score, qstart, qend, rstart, rend = (g[5 * x:5 * x + 5].tolist() for g in got)
        assert score[0] == 3 * (p + 90) - 12 and score[1] == 3 * (p + 88) - 11 and (qend[0], rend[0]) == (p + 90, p + 93)
        assert p + 1 <= qend[2] <= p + 12 and qstart[2] == 0 and p - 12 <= qstart[3] <= p - 1 and qend[3] == p + 90
        assert p - 12 <= qstart[4] <= p and rstart[4] - qstart[4] == 5 and qend[4] == p + 90


def test_a_gap_of_exactly_the_band_and_one_more(dev):
    rng = np.random.Generator(np.random.PCG64(400))
    for band in (1, 2, 16, MAX_BAND):
        x, y = mc.random_record(rng, 120), mc.random_record(rng, 120)
        queries = [x + y, x + mc.random_record(rng, band) + y, x + mc.random_record(rng, band + 1) + y]
        tasks = [(0, 1, 0, 0), (0, 2, 0, 0), (1, 0, 0, 0), (2, 0, 0, 0), (0, 1, band, 0), (0, 2, band + 1, 0), (0, 2, 1, 0)]
        scores = dict(match=3, mismatch=-1, gap_open=-2, gap_extend=-1)
        score = _check(dev, queries, queries, tasks, band, "band edge", **scores)[0].tolist()
        whole = 3 * 240 - 2 - (band - 1)
        assert score[0] == whole and score[2] == whole and score[4] == whole  # band residues without a partner: the last diagonal of the band
        assert score[1] < whole - 1 and score[3] < whole - 1 and score[5] < whole - 1 and score[6] == whole - 1        # band + 1: out of reach around 0


# ---- ties ----

def test_ties(dev):
    queries = [b"A" * 70, b"AC" * 40, b"ACGTTTTTACG", b"ACGTACGTAAAAAAAAAAAAACGTACGT", b"AA", b"ACAC", b"AAAAAAAAAA", b"ACGNACG", b"N" * 9]
    refs = [b"A" * 75, b"AC" * 43, b"CA" * 40, b"ACGAAAAAACG", b"ACGTACGTCCCCCCCCCCCCACGTACGT", b"AAA", b"TAA", b"ACACAC", b"AAAA", b"ACGNACG", b"N" * 9]
    pairs = [(0, 0), (1, 1), (1, 2), (2, 3), (3, 4), (4, 5), (4, 6), (5, 7), (6, 8), (6, 0), (7, 9), (8, 10), (0, 8), (1, 7)]
    for band in (1, 3, 16, MAX_BAND):
        tasks = [(q, r, d, strand) for q, r in pairs for d in (0, 1, -2) for strand in (0, 1)]
        for scores in (ac.DEFAULT, FREE, dict(match=2, mismatch=-1, gap_open=-1, gap_extend=-1), dict(match=2, mismatch=-1, gap_open=-3, gap_extend=-1),
                       dict(match=2, mismatch=0, gap_open=-1, gap_extend=0), dict(match=127, mismatch=-127, gap_open=-127, gap_extend=-127),
                       dict(match=3, mismatch=-2, gap_open=0, gap_extend=-3)):
            got = _check(dev, queries, refs, tasks, band, "ties", **scores)
            if scores["match"] == 127:
                # two equal segments in one task, nothing worth having between them: the one with the smaller i
                at = tasks.index((3, 4, 0, 0))
                assert [int(g[at]) for g in got] == [8 * 127, 0, 8, 0, 8]
            if scores is ac.DEFAULT:
                at = tasks.index((0, 0, 0, 0))
                assert [int(g[at]) for g in got] == [210, 0, 70, 0, 70]


# ---- many tasks ----

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


def test_seventy_thousand_tasks(dev):
    """more tasks than the largest grid has waves, with empty records and missed bands among them"""
    n = 70000
    assert n > 4 * GRID_MAX
    q, r, tasks = _short_batch(np.random.Generator(np.random.PCG64(70000)), 5000, 3000, n)
    for band, scores in [(3, ac.DEFAULT), (2, dict(match=2, mismatch=-1, gap_open=-1, gap_extend=-1))]:
        out = dev.raw(q, r, tasks, band, **scores)
        assert out[0] == dev.OK
        want = ac.banded_batch(*q, *r, *tasks, band, **scores)
        _same(out[1:], want, "70000")
        assert 0.5 * n < np.count_nonzero(want[0]) < 0.9 * n
        records = lambda x: [x[0][int(a):int(b)].tobytes() for a, b in zip(x[1][:-1], x[1][1:])]
        queries, refs = records(q), records(r)
        for t in (0, 1, 4 * GRID_MAX - 1, 4 * GRID_MAX, 4 * GRID_MAX + 1, n - 1):  # (the restatement proper, on a few)
            assert tuple(int(o[t]) for o in out[1:]) == ac.banded(queries[tasks[0][t]], refs[tasks[1][t]], int(tasks[2][t]), band, int(tasks[3][t]), **scores), t


def test_a_long_task_among_many_short_ones(dev):
    rng = np.random.Generator(np.random.PCG64(500))
    band = 16
    long_q = mc.random_record(rng, 3 * S, 0.002)
    long_r = mc.random_record(rng, 200) + ac.mutate(rng, long_q, 0.02, 0.003) + mc.random_record(rng, 100)
    q, r, tasks = _short_batch(rng, 300, 200, 1200)
    records = lambda x: [x[0][int(a):int(b)].tobytes() for a, b in zip(x[1][:-1], x[1][1:])]
    queries, refs = records(q) + [long_q], records(r) + [long_r]
    short = list(zip(*(t.tolist() for t in tasks)))
    want_short = ac.banded_batch(*q, *r, *tasks, band)
    want_long = ac.banded(long_q, long_r, 200, band)
    assert want_long[0] > 7 * S
    for where in (0, 600, 1200):
        got = dev.run(queries, refs, short[:where] + [(300, 200, 200, 0)] + short[where:], band)
        assert tuple(int(g[where]) for g in got) == want_long, where
        _same([np.delete(g, where) for g in got], want_short, ("short around long", where))


def test_a_tasks_result_does_not_depend_on_the_batch(dev):
    rng = np.random.Generator(np.random.PCG64(600))
    band = 9
    q, r, tasks = _short_batch(rng, 50, 50, 90)
    records = lambda x: [x[0][int(a):int(b)].tobytes() for a, b in zip(x[1][:-1], x[1][1:])]
    queries, refs = records(q), records(r)
    others = list(zip(*(t.tolist() for t in tasks)))
    x = mc.random_record(rng, S + 100, 0.01)
    for mine_q, mine_r, d, strand in [(x, ac.mutate(rng, x, 0.05, 0.01), 0, 0), (ac.orient(x[:200], 1), x, 0, 1), (b"A" * 40, b"A" * 50, 3, 0)]:
        task = (len(queries), len(refs), d, strand)
        want = ac.banded(mine_q, mine_r, d, band, strand)
        assert want[0] > 0
        for place in (0, 17, len(others)):
            got = dev.run(queries + [mine_q], refs + [mine_r], others[:place] + [task] + others[place:], band)
            assert tuple(int(g[place]) for g in got) == want, place
        assert tuple(int(g[0]) for g in dev.run([mine_q], [mine_r], [(0, 0, d, strand)], band)) == want


# ---- the rows, scores and diagonals the packed origins and keys are sized for ----

MAX_QUERY = _header_constant("KDB_ALIGN_MAX_QUERY")
LETTERS = np.frombuffer(b"ACGT", dtype=np.uint8)


def _substitute(rng, rec, p):
    """a copy of rec with about p of its residues replaced by another letter (numpy: ac.mutate walks a megabase residue by residue)"""
    s = np.frombuffer(bytes(rec), dtype=np.uint8).copy()
    at = np.flatnonzero(rng.random(s.size) < p)
    s[at] = LETTERS[(np.searchsorted(LETTERS, s[at]) + rng.integers(1, 4, size=at.size)) % 4]
    return s.tobytes()


def _both_strands(dev, x, ref, d, band, where, before=(b"ACGTTGCAN", b"GATTACA"), **scores):
    """The task (x, ref, d) on strand 0, and on strand 1 with the query handed over as x's reverse complement: the oriented query is x both
    times (ac.banded turns the record round first and is the same computation from there on), so one run of ac.banded is the reference
    of both.  `before`: records ahead of the two in their buffers -> the reference's tuple"""
    assert ac.orient(ac.orient(x, 1), 1) == x
    want = ac.banded(x, ref, d, band, 0, **scores)
    got = dev.run([before[0], x, ac.orient(x, 1)], [before[1], ref], [(1, 1, d, 0), (2, 1, d, 1)], band, **scores)
    for strand in (0, 1):
        assert tuple(int(g[strand]) for g in got) == want, (where, strand)
    return want


def test_a_query_of_the_largest_length(dev):
    """m = KDB_ALIGN_MAX_QUERY: rows up to 2^20 - 1 in the origins and in the best cell's key, 2049 stages"""
    rng = np.random.Generator(np.random.PCG64(1 << 20))
    x = mc.random_record(rng, MAX_QUERY)
    ref = _substitute(rng, x, 0.02)                                           # substitutions alone: the path stays on the diagonal
    before = (mc.random_record(rng, 1001), mc.random_record(rng, 777))        # (the records begin at odd offsets, far into their buffers)
    score, qstart, qend, rstart, rend = _both_strands(dev, x, ref, 0, 1, "2^20 rows", before)
    assert score > 2 * MAX_QUERY and qend - qstart > MAX_QUERY - 1000 and (qend - qstart) == (rend - rstart)


def test_the_largest_score_there_is(dev):
    """127 x 2^20, above 2^26: the score's 27 bits beside the 27 of the best cell's place"""
    rng = np.random.Generator(np.random.PCG64(127 << 20))
    x = mc.random_record(rng, MAX_QUERY)
    before = (mc.random_record(rng, 1001), mc.random_record(rng, 777))
    scores = dict(match=127, mismatch=-127, gap_open=-127, gap_extend=-127)
    out = dev.raw(mc.pack([before[0], x]), mc.pack([before[1], x]), ac.task_arrays([(1, 1, 0, 0)]), 2, ms=True, **scores)
    want = ac.banded(x, x, 0, 2, 0, **scores)
    assert out[0] == dev.OK and tuple(int(o[0]) for o in out[1:]) == want == (127 * MAX_QUERY, 0, MAX_QUERY, 0, MAX_QUERY) and want[0] > 2 ** 26


FAR = (1 << 16) + 700


def _far_row_cases(rng, top):
    """three tasks of top + 700 rows whose origin or best cell lies beyond row `top` -> [(name, query, reference, d)]"""
    x = mc.random_record(rng, top + 700)
    tail, p = mc.random_record(rng, 650), top + 300
    return [("an indel of three after row top", x, _substitute(rng, x[:top + 100] + b"ACG" + x[top + 100:], 0.01), 0),
            ("the origin beyond row top", b"A" * (top + 50) + tail, b"C" * (top + 55) + tail, 5),
            ("the best cell beyond row top", x[:p] + mc.random_record(rng, 400), x[:p] + mc.random_record(rng, 400), 0)]


@pytest.mark.parametrize("case", [0, 1, 2])
def test_origins_and_best_cells_beyond_row_65536(dev, case):
    """rows that do not fit 16 bits in an origin (cases 0 and 1) and in the best cell (all three), on both strands"""
    name, x, ref, d = _far_row_cases(np.random.Generator(np.random.PCG64(65536)), 1 << 16)[case]
    assert len(x) == FAR
    score, qstart, qend, rstart, rend = _both_strands(dev, x, ref, d, 8, name, match=3, mismatch=-4, gap_open=-10, gap_extend=-1)
    if case == 0:
        assert (qstart, rstart, qend, rend) == (0, 0, FAR, FAR + 3) and score > 2 * FAR
    elif case == 1:
        assert (qstart, rstart, qend, rend, score) == ((1 << 16) + 50, (1 << 16) + 55, FAR, FAR + 5, 3 * 650)
    else:
        assert qstart == 0 and (1 << 16) + 300 <= qend < (1 << 16) + 320 and rend == qend and score >= 3 * ((1 << 16) + 300)


def test_an_origin_beyond_row_524288(dev):
    """bit 19 of the row is set in the origin and in the best cell"""
    top = 1 << 19
    name, x, ref, d = _far_row_cases(np.random.Generator(np.random.PCG64(524288)), top)[1]
    assert _both_strands(dev, x, ref, d, 1, name) == (3 * 650, top + 50, top + 700, top + 55, top + 705)


def test_the_tie_rule_between_row_0_and_row_524288(dev):
    """Two segments of one score, one at row 0 and one beyond row 2^19, nothing worth having between them: the smaller row wins, on one
    diagonal (one lane's own `>`) and on two (the wave's reduction of (score, -row, -diagonal)); the far one wins where it is one match
    longer."""
    n = 1 << 19
    seg = b"GCTGACTCGTGACCTGATCGTGCTAGTCGATGCGTCAGTC"
    assert len(seg) == 40 and 3 * len(seg) % 8 == 0
    q = seg + b"A" * n + seg
    one = ac.banded(q, seg + b"C" * n + seg, 0, 1)
    two = ac.banded(q, seg + b"C" * (n + 1) + seg, 0, 1)
    far = ac.banded(q + b"G", seg + b"C" * (n + 1) + seg + b"G", 0, 1)
    assert one == two == (120, 0, 40, 0, 40) and far == (123, 40 + n, 81 + n, 41 + n, 82 + n)
    got = dev.run([q, q + b"G"], [seg + b"C" * n + seg, seg + b"C" * (n + 1) + seg, seg + b"C" * (n + 1) + seg + b"G"], [(0, 0, 0, 0), (0, 1, 0, 0), (1, 2, 0, 0)], 1)
    assert [tuple(int(g[t]) for g in got) for t in range(3)] == [one, two, far]


def test_every_diagonal_of_the_widest_band_over_forty_stages(dev):
    """all 127 diagonals, 64 lanes, and a path that keeps changing lanes while the wave refills its residues forty times"""
    rng = np.random.Generator(np.random.PCG64(20000))
    x = mc.random_record(rng, 20000, 0.001)
    ref = ac.mutate(rng, x, 0.02, 0.01)                                       # indels: the path wanders from lane to lane
    assert 20000 + MAX_BAND > 39 * S and abs(len(ref) - len(x)) < MAX_BAND
    score, qstart, qend, rstart, rend = _both_strands(dev, x, ref, 0, MAX_BAND, "widest band", match=3, mismatch=-1, gap_open=-4, gap_extend=-1)
    assert qend - qstart > 19000 and score > 40000


def test_far_diagonals_in_a_record_of_sixteen_million_residues(dev):
    """jb = d - band up to 2^24 and beyond, in a record that is not the buffer's first"""
    rng = np.random.Generator(np.random.PCG64(1 << 24))
    n, band = (1 << 24) + 1000, 16
    big = LETTERS[rng.integers(0, 4, size=n)]
    big[rng.random(n) < 0.0005] = ord("N")
    big = big.tobytes()
    queries, tasks = [], []
    for a in (3, (1 << 16) - 150, (1 << 24) - 150, n - 300):
        piece = big[a:a + 300]
        queries.append(_substitute(rng, piece, 0.03) if a == n - 300 else ac.mutate(rng, piece, 0.03, 0.004))
        tasks += [(len(queries) - 1, 1, a, 0), (len(queries), 1, a, 1)]
        queries.append(ac.orient(queries[-1], 1))
    tasks += [(4, 1, (1 << 24) - 150 + band, 0), (4, 1, (1 << 24) - 150 - band, 0), (6, 1, n - 300 + band, 0), (0, 1, 3 - band, 0), (1, 1, 3 - band, 1)]
    m = len(queries[0])
    tasks += [(0, 1, n + band, 0), (0, 1, -(m - 1) - band - 1, 0), (0, 1, n - 1 + band, 0), (0, 1, -(m - 1) - band, 1), (0, 0, 0, 0)]
    got = _check(dev, queries, [b"ACGTACGTACGTA", big], tasks, band, "far diagonals")
    score, rend = got[0].tolist(), got[4].tolist()
    assert min(score[:8]) > 500 and rend[6] == rend[7] == n and score[13] == score[14] == 0 and rend[4] > 1 << 24


def test_a_task_of_65536_rows_while_its_neighbours_stride_on(dev):
    """more short tasks than the largest grid has waves, and among the first of them one that keeps its wave for 2^16 rows: the other
    three waves of its workgroup go on to their next tasks meanwhile"""
    rng = np.random.Generator(np.random.PCG64(65537))
    band, nshort = 4, 4 * GRID_MAX + 3000
    long_q = mc.random_record(rng, (1 << 16) + 200, 0.002)
    long_r = mc.random_record(rng, 90) + ac.mutate(rng, long_q, 0.02, 0.0005) + mc.random_record(rng, 100)
    q, r, tasks = _short_batch(rng, 3000, 2000, nshort)
    records = lambda x: [x[0][int(a):int(b)].tobytes() for a, b in zip(x[1][:-1], x[1][1:])]
    queries, refs = records(q) + [long_q], records(r) + [long_r]
    short = list(zip(*(t.tolist() for t in tasks)))
    want_short = ac.banded_batch(*q, *r, *tasks, band)
    want_long = ac.banded(long_q, long_r, 90, band)
    assert want_long[0] > 2 * (1 << 16) and want_long[2] > 1 << 16
    where = 5
    got = dev.run(queries, refs, short[:where] + [(3000, 2000, 90, 0)] + short[where:], band)
    assert tuple(int(g[where]) for g in got) == want_long
    _same([np.delete(g, where) for g in got], want_short, "short around 2^16 rows")
    assert tuple(int(g[0]) for g in dev.run([long_q], [long_r], [(0, 0, 90, 0)], band)) == want_long


# ---- refusals ----

def _untouched(out):
    return np.all(out[1] == -1) and all(np.all(o == FILL32) for o in out[2:])


def test_refusals_by_status(dev):
    q, r = mc.pack([b"ACGTACGTAC", b"ACGTNACGT"]), mc.pack([b"ACGTACGTACGGT"])
    tasks = ac.task_arrays([(0, 0, 0, 0), (1, 0, 1, 1)])
    ok = lambda **kw: dev.raw(q, r, tasks, **kw)
    assert ok()[0] == dev.OK and not _untouched(ok())
    for kw in (dict(band=0), dict(band=MAX_BAND + 1), dict(band=-1), dict(match=0), dict(match=128), dict(match=-3), dict(mismatch=1), dict(mismatch=-128),
               dict(gap_open=1), dict(gap_open=-128), dict(gap_extend=1), dict(gap_extend=-128)):
        out = ok(**kw)
        assert out[0] == dev.ARG and _untouched(out), kw
        assert ok(ntasks=0, **kw)[0] == dev.ARG, kw                            # (the scalars are checked even where there is nothing to do)
    assert ok(band=MAX_BAND, match=127, mismatch=-127, gap_open=-127, gap_extend=-127)[0] == dev.OK and ok(mismatch=0, gap_open=0, gap_extend=0)[0] == dev.OK
    for null in ("q_bases", "q_offsets", "r_bases", "r_offsets", "task_q", "task_r", "task_diag", "task_strand") + NAMES:
        out = ok(null=(null,))
        assert out[0] == dev.ARG and _untouched(out), null
    bad_offsets = lambda o: (q[0], np.array(o, dtype=np.uint64))
    for o in ([1, 10, 19], [0, 10, 18], [0, 12, 11, 19], [0, 25, 19]):
        assert dev.raw(bad_offsets(o), r, tasks)[0] == dev.ARG, o
        assert dev.raw(r, bad_offsets(o), ac.task_arrays([(0, 0, 0, 0)]))[0] == dev.ARG, o
    for bad in ([(2, 0, 0, 0)], [(0, 1, 0, 0)], [(0, 0, 0, 0), (0, 0, 0, 2)], [(0, 0, 0, 255)], [(2 ** 32 - 1, 0, 0, 0)]):
        out = dev.raw(q, r, ac.task_arrays(bad))
        assert out[0] == dev.ARG and _untouched(out), bad
    assert ok(q_nbytes=(1 << 30) + 1)[0] == dev.ARG and ok(r_nbytes=(1 << 30) + 1)[0] == dev.ARG and ok(ntasks=(1 << 26) + 1)[0] == dev.ARG
    assert ok(nq=0)[0] == dev.ARG and ok(nr=0)[0] == dev.ARG
    # nothing to do is no error, and nothing is written
    out = ok(ntasks=0)
    assert out[0] == dev.OK and _untouched(out)
    assert dev.raw(q, r, ac.task_arrays([]))[0] == dev.OK
    assert ok(ms=True)[0] == dev.OK
    # empty buffers may be NULL: every task then gives zeros
    empty = (np.zeros(0, dtype=np.uint8), np.zeros(3, dtype=np.uint64))
    out = dev.raw(empty, r, ac.task_arrays([(0, 0, 0, 0), (1, 0, 0, 1)]))
    assert out[0] == dev.OK and all(o.tolist() == [0, 0] for o in out[1:])
    out = dev.raw(q, empty, tasks)
    assert out[0] == dev.OK and all(o.tolist() == [0, 0] for o in out[1:])
    from kmerdb_amd import alignment
    with pytest.raises(ValueError):
        alignment.align_tasks(b"ACGTRACGT", [0, 9], b"ACGT", [0, 4], [0], [0], [0], [0])


def test_bad_residues_leave_the_outputs_untouched(dev):
    good = b"ACGTNACGTACGTTGCA" * 3
    tasks = ac.task_arrays([(0, 0, 0, 0), (2, 1, 0, 1), (1, 2, 2, 0)])
    for bad in (b"a", b"R", b"n", b"\x80", b"\x00"):
        for at in (0, 20, len(good) - 1):
            rec = good[:at] + bad + good[at + 1:]
            for q, r in [([good, good, rec], [good, good, good]), ([good, good, good], [rec, good, good]), ([good, rec, good], [good, good, rec])]:
                out = dev.raw(mc.pack(q), mc.pack(r), tasks)
                assert out[0] == dev.BAD and _untouched(out), (bad, at)
    out = dev.raw(mc.pack([good] * 3), mc.pack([good] * 3), tasks)
    assert out[0] == dev.OK and out[1][0] > 100


def test_bad_arguments_raise_before_the_device_is_touched(dev, monkeypatch):
    from kmerdb_amd import alignment, distance, minimizer

    def touched(*a, **kw):
        raise AssertionError("the device was asked")
    monkeypatch.setattr(alignment, "align_raw", touched)
    monkeypatch.setattr(minimizer, "minimizers_raw", touched)
    monkeypatch.setattr(distance, "_require_device", touched)
    good = dict(q_bases=b"ACGTACGTAC", q_offsets=[0, 10], r_bases=b"ACGTACGTACGT", r_offsets=[0, 12], task_q=[0], task_r=[0], task_diag=[0], task_strand=[0])
    for change, err in [(dict(band=0), ValueError), (dict(band=64), ValueError), (dict(band=1.0), TypeError), (dict(band=True), TypeError), (dict(match=0), ValueError),
                        (dict(match=128), ValueError), (dict(mismatch=1), ValueError), (dict(gap_open=-128), ValueError), (dict(gap_extend=0.5), TypeError),
                        (dict(q_bases="ACGT"), TypeError), (dict(r_bases=np.zeros(12, dtype=np.int32)), TypeError), (dict(q_offsets=[0, 9]), ValueError),
                        (dict(q_offsets=[]), ValueError), (dict(r_offsets=[1, 12]), ValueError), (dict(r_offsets=[0, 14, 12]), ValueError), (dict(task_q=[1]), ValueError),
                        (dict(task_r=[-1]), ValueError), (dict(task_strand=[2]), ValueError), (dict(task_diag=[0.5]), TypeError), (dict(task_q=[0, 0]), ValueError),
                        (dict(task_q=[[0]]), TypeError)]:
        with pytest.raises(err):
            alignment.align_tasks(**{**good, **change})
    long_query = np.full((1 << 20) + 1, ord("A"), dtype=np.uint8)
    with pytest.raises(ValueError, match="2\\^20"):
        alignment.align_tasks(**{**good, "q_bases": long_query, "q_offsets": [0, long_query.size]})
    for kw, err in [(dict(k=0), ValueError), (dict(w=257), ValueError), (dict(order="random"), ValueError), (dict(band=64), ValueError), (dict(min_seeds=0), ValueError),
                    (dict(max_occ=0), ValueError), (dict(max_candidates=0), ValueError), (dict(min_score=-1), ValueError), (dict(match=1.5), TypeError)]:
        with pytest.raises(err):
            list(alignment.align_file(CONTIGS, CONTIGS, **kw))
    with pytest.raises(TypeError):
        list(alignment.align_file(5, CONTIGS))
    with pytest.raises(AssertionError):
        alignment.align_tasks(**good)


# ---- the pipeline ----

# Checked on the CPU first: with this seed no error-free read touches the copied segment or its source (so none ties between the two), the
# restatement places every one of them at its locus with score 3 x length, and five other reads have more than one result.
PIPELINE_SEED = 33


def _synthetic(seed):
    """three records of 20-30 kbp, the second holding 2 kbp of the first; 300 reads of 100-250 bp from both strands -- a third as they
    are, a third with substitutions, a third with one or two short indels -- and ten that belong nowhere
    -> (refs, reads, truth: per error-free read (ref, start, strand))"""
    rng = np.random.Generator(np.random.PCG64(seed))
    refs = [mc.random_record(rng, int(n)) for n in rng.integers(20000, 30001, size=3)]
    refs[1] = refs[1][:7000] + refs[0][3000:5000] + refs[1][9000:]
    reads, truth = [], {}
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
            truth["read%d" % i] = (ref, a, n, strand)
        reads.append(("read%d" % i, ac.orient(read, strand)))
    reads += [("noise%d" % i, mc.random_record(rng, int(rng.integers(100, 251)))) for i in range(10)]
    return [("ref%d" % i, s) for i, s in enumerate(refs)], reads, truth


def _write_fasta(path, records):
    with open(path, "w") as f:
        for name, s in records:
            f.write(">{0}\n".format(name))
            for a in range(0, len(s), 70):
                f.write(s[a:a + 70].decode() + "\n")


def test_the_pipeline_on_a_synthetic_reference(dev, tmp_path):
    from kmerdb_amd import alignment
    refs, reads, truth = _synthetic(PIPELINE_SEED)
    _write_fasta(tmp_path / "ref.fa", refs)
    _write_fasta(tmp_path / "reads.fa", reads)
    k, w, band = 15, 10, 8
    want = ac.pipeline(refs, reads, k, w, mc.HASHED, band)
    got = list(alignment.align_file(str(tmp_path / "ref.fa"), str(tmp_path / "reads.fa"), k=k, w=w, order="hashed", band=band))
    assert got == want
    assert list(alignment.align_file(str(tmp_path / "ref.fa"), str(tmp_path / "reads.fa"), k=k, w=w, order="hashed", band=band, batch_residues=5000)) == want
    best = {}
    for line in got:
        best.setdefault(line[0], line)
    assert len(truth) == 100 and not any(name.startswith("noise") for name in best) and len(best) > 280
    # an error-free read: every run of w positions inside it is a run of the reference's, so all its minimizers hit on one diagonal, and the
    # alignment along that diagonal is the whole read
    for name, (ref, a, n, strand) in truth.items():
        assert best[name][:10] == (name, n, 0, n, strand, "ref%d" % ref, len(refs[ref][1]), a, a + n, 3 * n), name
    only = list(alignment.align_file(str(tmp_path / "ref.fa"), str(tmp_path / "reads.fa"), k=k, w=w, order="hashed", band=band, best_only=True))
    assert only == [best[name] for name, _ in reads if name in best]


# ---- the subcommand ----

def _main(argv):
    from kmerdb_amd import profile
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        assert profile.main(argv) == 0
    return out.getvalue()


def test_the_subcommand(dev, tmp_path):
    from kmerdb_amd import alignment
    rng = np.random.Generator(np.random.PCG64(700))
    contigs = [(rid, s.upper().encode()) for rid, s in mc.read_fasta(CONTIGS)]
    reads = []
    for i in range(40):
        rid, s = contigs[0] if i & 1 else contigs[3]
        a = int(rng.integers(0, len(s) - 200))
        read = ac.mutate(rng, s[a:a + int(rng.integers(90, 200))].replace(b"N", b"A"), 0.02 if i % 4 < 2 else 0.0, 0.0)
        reads.append(("r%d" % i, ac.orient(read, (i >> 1) & 1)))
    reads += [("nowhere%d" % i, mc.random_record(rng, 150)) for i in range(5)]
    _write_fasta(tmp_path / "reads.fa", reads)
    query = str(tmp_path / "reads.fa")
    lines = [alignment.format_line(x) for x in alignment.align_file(CONTIGS, query, k=13, w=8, order="hashed", band=12, gap_open=-6)]
    names = [line.split("\t")[0] for line in lines]
    assert len(set(names)) == 40 and not any(name.startswith("nowhere") for name in names)
    assert all(line.split("\t")[4] in "+-" and len(line.rstrip("\n").split("\t")) == 12 for line in lines) and {line.split("\t")[4] for line in lines} == {"+", "-"}
    argv = ["alignment", "-k", "13", "-w", "8", "--order", "hashed", "--band", "12", "--gap-open", "-6", CONTIGS, query]
    assert _main(argv) == "".join(lines)
    out = tmp_path / "out.tsv"
    assert _main(argv[:1] + ["-o", str(out)] + argv[1:]) == "" and out.read_text() == "".join(lines)
    first = []
    for line in lines:
        if line.split("\t")[0] not in [x.split("\t")[0] for x in first]:
            first.append(line)
    assert _main(argv[:1] + ["--best-only"] + argv[1:]) == "".join(first) and len(first) == 40
    strict = _main(argv[:1] + ["--min-score", "400", "-n", "3", "--max-candidates", "1", "--max-occ", "10", "--match-score", "3", "--mismatch-score", "-2",
                               "--gap-extend", "-2"] + argv[1:])
    assert 0 < len(strict.splitlines()) < 40 and all(int(line.split("\t")[9]) >= 400 and int(line.split("\t")[10]) >= 3 for line in strict.splitlines())
