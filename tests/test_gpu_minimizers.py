"""GPU: kdb_minimizers -- the (w,k)-minimizers of every record (csrc/kdb_minimizers.hip.h) -- against the run-form restatement of
tests/minimizer_cases.py and against kdb_window_ids, and the layers above it: kmerdb_amd.minimizer and the `minimizers` subcommand.

Every output is an integer and compared exactly.  Every test here fails without kdb_minimizers: the library does not export the symbol."""
import contextlib
import ctypes
import io
import os
import re

import numpy as np
import pytest

import minimizer_cases as mc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
CONTIGS = os.path.join(GOLDEN, "inputs", "contigs.fa")
SAMPLE = os.path.join(GOLDEN, "ref_data", "sample.fa")
RAGGED = os.path.join(GOLDEN, "inputs", "ragged_n.fq")


def _header_constant(name):
    text = open(os.path.join(ROOT, "include", "kdbhip.h")).read()
    return int(re.search(r"#define\s+%s\s+(\d+)" % name, text).group(1))


P = _header_constant("KDB_MINIMIZER_PIECE")
MAX_K, MAX_W = _header_constant("KDB_MINIMIZER_MAX_K"), _header_constant("KDB_MINIMIZER_MAX_W")
LADDER = [(1, 1), (3, 2), (8, 1), (15, 10), (16, 16), (17, 5), (21, 11), (31, 19), (12, 256)]
FILL64, FILL32, FILL8 = 2 ** 64 - 1, 2 ** 32 - 1, 0xFF


@pytest.fixture(scope="module")
def dev(gpu_engine_cls):
    from kmerdb_amd import _abi

    class Dev:
        lib = _abi.lib()
        OK, ARG, BAD = _abi.KDB_OK, _abi.KDB_ERR_ARG, _abi.KDB_ERR_BAD_RESIDUE

        @classmethod
        def raw(cls, bases, offsets, k, w, canonical=1, order=0, cap=None, nreads=None, nbytes=None, null=()):
            """kdb_minimizers with the arguments as given, the host output buffers filled with 0xFF
            -> (status, counts, ids, pos, strand, total); cap: the entries of the flat buffers (default: one per residue)"""
            m = max(len(offsets) - 1, 1)                                     # (the buffers follow the offsets given, not a claimed nreads)
            n = len(offsets) - 1 if nreads is None else nreads
            cap = int(bases.size) if cap is None else cap
            counts = np.full(m, FILL64, dtype=np.uint64)
            ids, pos, strand = np.full(max(cap, 1), FILL64, dtype=np.uint64), np.full(max(cap, 1), FILL32, dtype=np.uint32), np.full(max(cap, 1), FILL8, dtype=np.uint8)
            total = ctypes.c_uint64(FILL64)
            ptr = lambda name, a: None if name in null else a.ctypes.data
            rc = cls.lib.kdb_minimizers(0, k, w, canonical, order, None if "bases" in null or bases.size == 0 else bases.ctypes.data,
                                        bases.size if nbytes is None else nbytes, ptr("offsets", offsets), n, ptr("counts", counts),
                                        ptr("ids", ids), ptr("pos", pos), ptr("strand", strand), cap,
                                        None if "total" in null else ctypes.byref(total), None)
            return rc, counts, ids, pos, strand, int(total.value)

        @classmethod
        def run(cls, records, k, w, canonical=True, order=mc.LEX):
            """-> (counts, ids, pos, strand) of the batch, the lists cut to the total"""
            bases, offsets = mc.pack(records)
            rc, counts, ids, pos, strand, total = cls.raw(bases, offsets, k, w, 1 if canonical else 0, order)
            assert rc == cls.OK, _abi.last_error()
            assert total == int(counts.sum()) and total <= bases.size
            assert np.all(ids[total:] == FILL64) and np.all(pos[total:] == FILL32) and np.all(strand[total:] == FILL8)
            return counts, ids[:total], pos[:total], strand[:total]
    return Dev


def _same(got, want, where=""):
    for name, g, x in zip(("counts", "ids", "pos", "strand"), got, want):
        assert g.dtype == x.dtype and g.shape == x.shape, (where, name, g.shape, x.shape)
        assert g.tobytes() == x.tobytes(), (where, name, np.flatnonzero(g != x)[:8].tolist())


def _check(dev, records, k, w, canonical=True, order=mc.LEX, where=""):
    got = dev.run(records, k, w, canonical, order)
    _same(got, mc.batch_minimizers(records, k, w, canonical, order), (where, k, w, canonical, order))
    return got


def _split(got):
    """the per-record lists of a batch's output"""
    counts, ids, pos, strand = got
    ends = np.cumsum(counts.astype(np.int64))
    return [(pos[e - c:e].tolist(), ids[e - c:e].tolist(), strand[e - c:e].tolist()) for e, c in zip(ends.tolist(), counts.astype(np.int64).tolist())]


# ---- every parameter combination, at every edge of the kernel ----

@pytest.mark.parametrize("order", [mc.LEX, mc.HASHED])
@pytest.mark.parametrize("canonical", [False, True])
@pytest.mark.parametrize("k,w", LADDER)
def test_record_length_ladder(dev, k, w, canonical, order):
    records = mc.ladder_records(k, w, P, 1000 * k + w)
    assert sorted(len(r) for r in records) == sorted(mc.ladder_lengths(k, w, P))
    counts, ids, pos, strand = _check(dev, records, k, w, canonical, order)
    assert int(counts.sum()) > 0 and (canonical or not strand.any())


# ---- ties and seams ----

def test_poly_a_and_repeats_across_the_seams(dev):
    for k, w in [(5, 7), (1, 1), (16, 64), (31, 256)]:
        n = 2 * P + 7
        for canonical, order in [(False, mc.LEX), (True, mc.HASHED)]:
            counts, ids, pos, strand = _check(dev, [b"A" * mc.length_for(n, k), b"T" * mc.length_for(n, k)], k, w, canonical, order, "poly-A")
            assert counts.tolist() == [n - w + 1, n - w + 1] and pos[:n - w + 1].tolist() == list(range(n - w + 1))
    for k, w in [(4, 6), (7, 19), (2, 2)]:
        records = [b"AC" * (P + 9), b"CA" * (P + 9) + b"C", b"ACG" * P, b"AACCGGTT" * (P // 4 + 3)]
        for canonical in (False, True):
            for order in (mc.LEX, mc.HASHED):
                _check(dev, records, k, w, canonical, order, "repeats")


def test_minima_at_and_around_a_seam(dev):
    rng = np.random.Generator(np.random.PCG64(77))
    k = 4
    for w in (2, 10, 16, 200):
        n = 2 * P + 40
        cases = {"equal keys on both sides": [P - 3, P + 3], "unique at P - 1": [P - 1], "unique at P": [P],
                 "seen through the right halo": [P + w - 2], "seen through the left halo": [P - w + 1 if w > 5 else P - 6],
                 "both seams": [P - 1, 2 * P], "far from the seams": [100, P + 300]}
        records = [mc.record_with_keys_at(rng, n, k, low) for low in cases.values()]
        got = _split(_check(dev, records, k, w, False, mc.LEX, "seams"))
        for (name, low), (pos, ids, strand) in zip(cases.items(), got):
            for p in low:
                assert p in pos and ids[pos.index(p)] == 0, (name, w, p)
            # poly-A at p is the smallest key of every run that holds p: nothing else of those runs' positions is selected unless
            # another run selects it
            assert all(i != 0 or p in low for p, i in zip(pos, ids)), (name, w)


# ---- N ----

def test_n_layouts(dev):
    rng = np.random.Generator(np.random.PCG64(78))
    for k, w in [(3, 2), (15, 10), (21, 11), (9, 64)]:
        L = mc.length_for(2 * P + 50, k)
        base = bytearray(mc.random_record(rng, L))
        first_n, last_n, window_n, run_n, seam_n, seam2_n = (bytearray(base) for _ in range(6))
        first_n[0] = ord("N")
        last_n[L - 1] = ord("N")
        window_n[500:500 + k] = b"N" * k                                      # every residue of the window at 500
        run_n[700:700 + k + w + 3] = b"N" * (k + w + 3)
        seam_n[P - 2:P + 3] = b"N" * 5                                        # the keys P - k - 1 .. P + 2 are gone: both sides of the seam
        seam2_n[P + k - 3:P + k + 1] = b"N" * 4                               # ... and the residues at the first piece's end
        seam2_n[2 * P - w:2 * P - w + 2] = b"NN"
        records = [bytes(first_n), b"N" * 300, bytes(last_n), bytes(window_n), b"N" * (k - 1), bytes(run_n), b"N" * k, bytes(seam_n), bytes(seam2_n),
                   b"N" * L, mc.random_record(rng, L, 0.05), mc.random_record(rng, 700, 0.05), b"A" * 40 + b"N" + b"A" * 40]
        for canonical, order in [(True, mc.LEX), (False, mc.HASHED)]:
            counts, ids, pos, strand = _check(dev, records, k, w, canonical, order, "N layouts")
            assert counts[1] == 0 and counts[4] == 0 and counts[6] == 0 and counts[9] == 0 and counts[10] > 0


# ---- compaction ----

def test_seventy_thousand_records(dev):
    """more records than one scan block and one grid stride hold, with runs of records that have no minimizer"""
    n, k, w = 70000, 7, 5
    rng = np.random.Generator(np.random.PCG64(70000))
    lens = rng.integers(20, 41, size=n)
    kind = rng.integers(0, 10, size=n)
    lens[kind == 0] = 0                                                       # empty
    lens[5000:5000 + 4500] = 0                                                # more than two scan blocks in a row without a minimizer
    offsets = np.zeros(n + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum(lens)
    bases = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=int(offsets[-1]))].copy()
    bases[rng.random(bases.size) < 0.02] = ord("N")
    all_n = np.repeat(kind == 1, lens)                                        # all-N records
    bases[all_n] = ord("N")
    for canonical, order in [(True, mc.HASHED), (False, mc.LEX)]:
        rc, counts, ids, pos, strand, total = dev.raw(bases, offsets, k, w, 1 if canonical else 0, order)
        assert rc == dev.OK
        want = mc.batch_minimizers_flat(bases, offsets, k, w, canonical, order)
        assert total == int(want[0].sum()) > n
        _same((counts, ids[:total], pos[:total], strand[:total]), want, "70000")
        assert not counts[lens == 0].any() and not counts[kind == 1].any()
    raw = bases.tobytes()
    for r in (0, 1, 4999, 9500, 65535, 65536, n - 1):                         # (the restatement proper, on a few)
        a, b = int(offsets[r]), int(offsets[r + 1])
        p, i, s = mc.record_minimizers(raw[a:b], k, w, False, mc.LEX)
        e = int(counts[:r + 1].sum())
        assert (pos[e - p.size:e].tolist(), ids[e - p.size:e].tolist()) == (p.tolist(), i.tolist()) and int(counts[r]) == p.size


def test_a_long_record_before_many_short_ones(dev):
    rng = np.random.Generator(np.random.PCG64(79))
    k, w = 11, 8
    records = [mc.random_record(rng, mc.length_for(5 * P, k), 0.001)] + [mc.random_record(rng, int(n)) for n in rng.integers(0, 60, size=2500)]
    counts, ids, pos, strand = _check(dev, records, k, w, True, mc.HASHED, "long then short")
    assert counts[0] > 5 * P // w and np.all(np.diff(pos[:int(counts[0])].astype(np.int64)) > 0)
    _check(dev, records[1:400] + records[:1] + records[400:800], k, w, False, mc.LEX, "short, long, short")


# ---- the piece counts of whole read sets and contigs ----

# scan_top_kernel takes the sums of the scan blocks SCAN_TPB at a time and carries the running sum from one trip to the next: a second
# trip needs more than SCAN_TOP pieces in one call
_SCAN = re.search(r"constexpr int SCAN_TPB = (\d+), SCAN_ITEMS = (\d+);", open(os.path.join(ROOT, "kmerdb_amd", "csrc", "kdb_minimizers.hip.h")).read())
SCAN_TPB, SCAN_ITEMS = int(_SCAN.group(1)), int(_SCAN.group(2))
SCAN_BLOCK = SCAN_TPB * SCAN_ITEMS
SCAN_TOP = SCAN_TPB * SCAN_BLOCK
SHORT_K, SHORT_W = 5, 4                                                       # a record of 8 residues has w start positions


def _short_records(n, seed, quiet=()):
    """n records of 8 .. 20 residues, a tenth of them empty, a twentieth all N, and none with a minimizer in the ranges `quiet`
    -> (bases, offsets, lens, all_n)"""
    rng = np.random.Generator(np.random.PCG64(seed))
    lens = rng.integers(8, 21, size=n)
    kind = rng.integers(0, 20, size=n)
    lens[kind < 2] = 0
    for a, b in quiet:
        lens[a:b:2] = 0                                                       # empty and all N by turns
        kind[a:b] = 2
    offsets = np.zeros(n + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum(lens)
    bases = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=int(offsets[-1]))].copy()
    bases[rng.random(bases.size) < 0.02] = ord("N")
    all_n = kind == 2
    bases[np.repeat(all_n, lens)] = ord("N")
    return bases, offsets, lens, all_n


def _spot_check(bases, offsets, got, rows, k, w, canonical, order):
    """the restatement proper on the records `rows` of a batch's output"""
    counts, ids, pos, strand = got
    ends = np.cumsum(counts.astype(np.int64))
    raw = bases.tobytes()
    for r in rows:
        p, i, s = mc.record_minimizers(raw[int(offsets[r]):int(offsets[r + 1])], k, w, canonical, order)
        e = int(ends[r])
        assert int(counts[r]) == p.size and (pos[e - p.size:e].tolist(), ids[e - p.size:e].tolist(), strand[e - p.size:e].tolist()) == (p.tolist(), i.tolist(), s.tolist()), r


@pytest.mark.parametrize("canonical,order", [(True, mc.HASHED), (False, mc.LEX)])
@pytest.mark.parametrize("n", [SCAN_TOP, SCAN_TOP + 1, 2 * SCAN_TOP + 3])
def test_one_two_and_three_trips_of_the_top_scan(dev, n, canonical, order):
    """one piece per record: one trip exactly, a second trip of one block sum, three trips; more than a scan block of records without a
    minimizer lies across piece SCAN_TOP (up to it where the call ends there)"""
    quiet = (SCAN_TOP - SCAN_BLOCK - 100, min(n, SCAN_TOP + SCAN_BLOCK // 2 + 100))
    bases, offsets, lens, all_n = _short_records(n, n, [quiet])
    assert quiet[1] - quiet[0] > SCAN_BLOCK
    rc, counts, ids, pos, strand, total = dev.raw(bases, offsets, SHORT_K, SHORT_W, 1 if canonical else 0, order)
    assert rc == dev.OK
    want = mc.batch_minimizers_flat(bases, offsets, SHORT_K, SHORT_W, canonical, order)
    assert total == int(want[0].sum()) > n and total <= bases.size
    got = (counts, ids[:total], pos[:total], strand[:total])
    _same(got, want, ("top scan", n))
    assert np.all(ids[total:] == FILL64) and np.all(pos[total:] == FILL32) and np.all(strand[total:] == FILL8)
    assert not counts[lens == 0].any() and not counts[all_n].any() and not counts[quiet[0]:quiet[1]].any()
    assert counts[quiet[0] - 50:quiet[0]].any() and (quiet[1] == n or counts[quiet[1]:quiet[1] + 50].any())
    rows = [0, SCAN_BLOCK - 1, SCAN_BLOCK, quiet[0] - 1, SCAN_TOP - 2, SCAN_TOP - 1, SCAN_TOP, SCAN_TOP + 1, quiet[1], 2 * SCAN_TOP - 1, 2 * SCAN_TOP, n - 1]
    _spot_check(bases, offsets, got, [r for r in rows if r < n], SHORT_K, SHORT_W, canonical, order)


@pytest.mark.parametrize("canonical,order", [(True, mc.HASHED), (False, mc.LEX)])
def test_records_of_several_pieces_in_a_call_of_two_trips(dev, canonical, order):
    """piece_rec is there: a record of five pieces first, one whose four pieces are SCAN_TOP - 2 .. SCAN_TOP + 1, one of four last"""
    k, w = SHORT_K, SHORT_W
    rng = np.random.Generator(np.random.PCG64(2 * SCAN_TOP))
    long = [np.frombuffer(mc.random_record(rng, mc.length_for(nwin, k), 0.001), dtype=np.uint8) for nwin in (5 * P, 3 * P + 1, 3 * P + 17)]
    between, after = SCAN_TOP - 2 - 5, 1000
    b1, o1, l1, _ = _short_records(between, 11)
    b2, o2, l2, _ = _short_records(after, 12)
    bases = np.concatenate([long[0], b1, long[1], b2, long[2]])
    lens = np.concatenate([[long[0].size], l1, [long[1].size], l2, [long[2].size]])
    offsets = np.concatenate(([0], np.cumsum(lens))).astype(np.uint64)
    nwin = np.maximum(lens - k + 1, 0)
    first_piece = np.concatenate(([0], np.cumsum(np.maximum(1, -(-nwin // P)))))
    at = between + 1                                                          # the record across piece SCAN_TOP
    assert int(first_piece[at]) == SCAN_TOP - 2 and int(first_piece[at + 1]) == SCAN_TOP + 2 and int(first_piece[-1]) > SCAN_TOP + after
    rc, counts, ids, pos, strand, total = dev.raw(bases, offsets, k, w, 1 if canonical else 0, order)
    assert rc == dev.OK
    want = mc.batch_minimizers_flat(bases, offsets, k, w, canonical, order)
    assert total == int(want[0].sum())
    got = (counts, ids[:total], pos[:total], strand[:total])
    _same(got, want, "several pieces, two trips")
    assert all(int(counts[r]) > nw // w for r, nw in ((0, 5 * P), (at, 3 * P + 1), (lens.size - 1, 3 * P + 17)))
    _spot_check(bases, offsets, got, [0, 1, at - 1, at, at + 1, lens.size - 2, lens.size - 1], k, w, canonical, order)


@pytest.mark.parametrize("k,w,pieces", [(15, 10, 2100), (31, 256, 300)])
def test_one_record_of_more_pieces_than_a_scan_block(dev, k, w, pieces):
    """a record's count is the difference of two prefix sums SCAN_BLOCK and more pieces apart (k = 15: over four megabases), and its
    positions do not fit 22 bits; at w = 256 every piece reads a halo of 255 keys on either side"""
    rng = np.random.Generator(np.random.PCG64(pieces))
    nwin = pieces * P + 301
    contig = bytearray(mc.random_record(rng, mc.length_for(nwin, k)))
    for at in rng.integers(0, len(contig), size=9).tolist():
        contig[at] = ord("N")
    shorts = [mc.random_record(rng, int(n), 0.01) for n in rng.integers(0, 90, size=60)]
    records = shorts[:35] + [bytes(contig)] + shorts[35:]
    counts, ids, pos, strand = _check(dev, records, k, w, True, mc.HASHED, "a contig")
    e = int(counts[:36].sum())
    mine = pos[e - int(counts[35]):e].astype(np.int64)
    assert (pieces <= SCAN_BLOCK or int(mine.max()) > 2 ** 22) and int(counts[35]) > nwin // w and np.all(np.diff(mine) > 0) and int(mine[-1]) >= nwin - w


@pytest.mark.parametrize("order", [mc.LEX, mc.HASHED])
@pytest.mark.parametrize("canonical", [False, True])
def test_whole_pieces_without_a_key_inside_a_record(dev, canonical, order):
    """Eight pieces: N from the record's start past its first two pieces, N over two pieces in its middle, and N from w - 1 positions
    before the last piece to the end -- that piece selects nothing (emit_kernel leaves at once) and its left neighbour's halo is all
    +infinity."""
    rng = np.random.Generator(np.random.PCG64(88))
    for k, w in [(15, 10), (5, 200), (31, 256)]:
        L = mc.length_for(8 * P, k)
        rec = bytearray(mc.random_record(rng, L))
        rec[:2 * P + w + 5] = b"N" * (2 * P + w + 5)
        rec[4 * P - 30:6 * P + w + 40] = b"N" * (2 * P + w + 70)
        rec[7 * P - w:] = b"N" * (L - (7 * P - w))
        middle = bytearray(mc.random_record(rng, mc.length_for(3 * P + 9, k)))   # only its middle piece has no key
        middle[P - k + 1:2 * P + k - 1] = b"N" * (P + 2 * k - 2)
        records = [mc.random_record(rng, 200), bytes(rec), b"N" * (2 * P + 50), mc.random_record(rng, 64), bytes(middle), b"", bytes(rec), mc.random_record(rng, 30)]
        counts, ids, pos, strand = _check(dev, records, k, w, canonical, order, "pieces of N")
        mine = pos[int(counts[0]):int(counts[:2].sum())].astype(np.int64)
        assert int(counts[2]) == 0 and int(counts[1]) == int(counts[6]) > 0
        assert sorted(set((mine // P).tolist())) == [2, 3, 6] and int(mine[0]) == 2 * P + w + 5 and int(mine[-1]) == 7 * P - w - k


# ---- capacity ----

def test_capacity(dev):
    rng = np.random.Generator(np.random.PCG64(80))
    records = [mc.random_record(rng, n, 0.01) for n in (300, 0, P + 500, 40, 2 * P + 100)]
    bases, offsets = mc.pack(records)
    k, w = 13, 9
    want = mc.batch_minimizers(records, k, w, True, mc.HASHED)
    total = int(want[0].sum())
    rc, counts, ids, pos, strand, got_total = dev.raw(bases, offsets, k, w, 1, mc.HASHED, cap=total)
    assert rc == dev.OK and got_total == total
    _same((counts, ids, pos, strand), want, "cap = total")
    rc, counts, ids, pos, strand, got_total = dev.raw(bases, offsets, k, w, 1, mc.HASHED, cap=total, null=("strand",))
    assert rc == dev.OK and np.all(strand == FILL8)
    _same((counts, ids, pos), want[:3], "no strand list")
    for cap, null in [(total - 1, ()), (0, ("ids", "pos", "strand")), (0, ()), (1, ("strand",))]:
        rc, counts, ids, pos, strand, got_total = dev.raw(bases, offsets, k, w, 1, mc.HASHED, cap=cap, null=null)
        assert rc == dev.OK and got_total == total and counts.tolist() == want[0].tolist(), (cap, null)
        assert np.all(ids == FILL64) and np.all(pos == FILL32) and np.all(strand == FILL8), (cap, null)


# ---- refusals ----

def test_refusals_by_status(dev):
    bases, offsets = mc.pack([b"ACGTACGTAC", b"ACGTNACGT"])
    ok = lambda **kw: dev.raw(bases, offsets, **{"k": 3, "w": 2, **kw})[0]
    assert ok() == dev.OK
    for k in (0, MAX_K + 1, -1, 64):
        assert ok(k=k) == dev.ARG, k
    assert ok(k=MAX_K) == dev.OK and ok(w=MAX_W) == dev.OK
    for w in (0, MAX_W + 1, -1):
        assert ok(w=w) == dev.ARG, w
    for order in (2, -1, 7):
        assert ok(order=order) == dev.ARG, order
    for null in ("counts", "total", "offsets", "bases"):
        assert ok(null=(null,)) == dev.ARG, null
    for null in (("ids",), ("pos",), ("ids", "pos", "strand")):
        assert ok(null=null) == dev.ARG, null
    assert ok(null=("strand",)) == dev.OK
    for bad in ([1, 10, 19], [0, 10, 18], [0, 12, 11, 19], [0, 25, 19]):
        assert dev.raw(bases, np.array(bad, dtype=np.uint64), 3, 2)[0] == dev.ARG, bad
    assert dev.raw(bases, offsets, 3, 2, nbytes=(1 << 30) + 1)[0] == dev.ARG
    assert dev.raw(bases, offsets, 3, 2, nreads=(1 << 30) + 1)[0] == dev.ARG
    assert dev.raw(bases, offsets, 3, 2, nreads=0)[0] == dev.ARG              # residues but no records
    rc, counts, ids, pos, strand, total = dev.raw(bases[:0], offsets[:1], 3, 2)                 # nothing at all
    assert rc == dev.OK and total == 0
    rc, counts, ids, pos, strand, total = dev.raw(bases[:0], np.zeros(4, dtype=np.uint64), 3, 2)  # three empty records
    assert rc == dev.OK and total == 0 and counts.tolist() == [0, 0, 0]
    from kmerdb_amd import minimizer
    with pytest.raises(ValueError):
        minimizer.minimizers(b"ACGTRACGT", [0, 9], 3, 2)


def test_bad_residues_leave_the_outputs_untouched(dev):
    good = b"ACGTNACGTACGTTGCA" * 3
    for bad in (b"a", b"R", b"n", b"\x80", b"\x00"):
        for at in (0, 20, len(good) - 1):
            rec = good[:at] + bad + good[at + 1:]
            rc, counts, ids, pos, strand, total = dev.raw(*mc.pack([good, good, rec]), 4, 3)
            assert rc == dev.BAD and total == FILL64, (bad, at)
            assert np.all(counts == FILL64) and np.all(ids == FILL64) and np.all(pos == FILL32) and np.all(strand == FILL8), (bad, at)
    rc, counts, ids, pos, strand, total = dev.raw(*mc.pack([good, good, good]), 4, 3)
    assert rc == dev.OK and total == int(counts.sum()) > 0


# ---- against kdb_window_ids ----

@pytest.mark.parametrize("k,w,canonical", [(3, 4, True), (12, 10, False), (15, 19, True), (17, 5, True), (17, 31, False)])
def test_against_window_ids(dev, k, w, canonical):
    """the ids at the selected positions are kdb_window_ids', and the selected set is the run minimum over that array"""
    from kmerdb_amd.engine import IdsEngine, NO_WINDOW
    rng = np.random.Generator(np.random.PCG64(81))
    records = [mc.random_record(rng, n, 0.004) for n in (k, 150, k + w - 1, P + 333, 3 * P, 64)] + [b"N" * 90, b"ACGT" * 200]
    bases, offsets = mc.pack(records)
    eng = IdsEngine(k, canonicalize=canonical)
    try:
        window = eng.window_ids(bases, offsets)
    finally:
        eng.close()
    got = _split(dev.run(records, k, w, canonical, mc.LEX))
    hashed = _split(dev.run(records, k, w, canonical, mc.HASHED))
    for r, rec in enumerate(records):
        nwin = len(rec) - k + 1
        keys = window[int(offsets[r]):int(offsets[r]) + nwin]
        assert NO_WINDOW == mc.INF
        want = mc.select_runs(keys, w)
        assert got[r][0] == want.tolist() and got[r][1] == keys[want].tolist(), r
        assert hashed[r][1] == keys[np.array(hashed[r][0], dtype=np.int64)].tolist(), r
        assert hashed[r][0] == mc.select_runs(np.where(keys != mc.INF, mc.h_array(keys, k), mc.INF), w).tolist(), r


# ---- independence ----

def test_a_records_list_does_not_depend_on_the_batch(dev):
    rng = np.random.Generator(np.random.PCG64(82))
    k, w = 14, 12
    others = [mc.random_record(rng, int(n), 0.01) for n in rng.integers(0, 300, size=40)] + [mc.random_record(rng, 2 * P + 77)]
    for rec in (mc.random_record(rng, 3 * P + 100, 0.002), mc.random_record(rng, 151), b"A" * (P + 50)):
        alone = _split(_check(dev, [rec], k, w, True, mc.HASHED))[0]
        assert len(alone[0]) > 0
        first = _split(dev.run([rec] + others, k, w, True, mc.HASHED))[0]
        last = _split(dev.run(others + [rec], k, w, True, mc.HASHED))[-1]
        middle = _split(dev.run(others[:17] + [rec] + others[17:], k, w, True, mc.HASHED))[17]
        assert alone == first == last == middle


# ---- files and the subcommand ----

def _main(argv):
    from kmerdb_amd import profile
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        assert profile.main(argv) == 0
    return out.getvalue()


def _file_lists(path, k, w, **kw):
    from kmerdb_amd import minimizer
    return [(rid, length, pos.tolist(), ids.tolist(), strand.tolist()) for rid, length, pos, ids, strand in minimizer.minimizers_file(path, k, w, **kw)]


@pytest.mark.parametrize("path,k,w,order,small", [(CONTIGS, 11, 8, "lexicographic", 4096), (SAMPLE, 15, 10, "hashed", 40000), (SAMPLE, 21, 200, "lexicographic", 50000)])
def test_files_through_every_layer(dev, path, k, w, order, small, tmp_path):
    from kmerdb_amd import minimizer
    recs = [(rid, s.upper().encode()) for rid, s in mc.read_fasta(path)]
    assert max(len(s) for _, s in recs) > 2 * small                            # (a record of three reader pieces and more)
    direct = _split(dev.run([s for _, s in recs], k, w, True, minimizer.ORDERS[order]))
    want = [(rid, len(s)) + mc_lists for (rid, s), mc_lists in zip(recs, direct)]
    for (rid, s), (pos, ids, strand) in zip(recs, direct):
        p, i, st = mc.record_minimizers(s, k, w, True, minimizer.ORDERS[order])
        assert (pos, ids, strand) == (p.tolist(), i.tolist(), st.tolist()), rid
    assert _file_lists(path, k, w, order=order) == want
    assert _file_lists(path, k, w, order=order, block_bytes=small) == want
    lines = _main(["minimizers", "-k", str(k), "-w", str(w), "--order", order, path]).splitlines()
    assert lines == ["{0}\t{1}\t{2}\t{3}".format(rid, p, i, "-" if s else "+") for rid, _, pos, ids, strand in want for p, i, s in zip(pos, ids, strand)]
    if path == CONTIGS:
        out = tmp_path / "contigs.kdbi.1"
        assert _main(["minimizers", "-k", str(k), "-w", str(w), "--do-not-canonicalize", "-o", str(out), path]) == ""
        forward = _split(dev.run([s for _, s in recs], k, w, False, mc.LEX))
        assert out.read_text().splitlines() == ["{0}\t{1}\t{2}\t+".format(rid, p, i) for (rid, _), (pos, ids, _) in zip(recs, forward) for p, i in zip(pos, ids)]


def test_fastq_input(dev):
    recs = mc.read_fastq(RAGGED)
    assert len(recs) == 125 and any("N" in s for _, s in recs)
    got = _file_lists(RAGGED, 9, 6, canonical=False, order="hashed")
    assert [(g[0], g[1]) for g in got] == [(rid, len(s)) for rid, s in recs]
    for g, (rid, s) in zip(got, recs):
        p, i, st = mc.record_minimizers(s.encode(), 9, 6, False, mc.HASHED)
        assert g[2:] == (p.tolist(), i.tolist(), st.tolist()), rid


def test_the_lists_are_sized_by_an_estimate_and_one_more_call(dev, monkeypatch):
    from kmerdb_amd import minimizer
    calls = []
    raw = minimizer.minimizers_raw
    monkeypatch.setattr(minimizer, "minimizers_raw", lambda *a, **kw: calls.append(a[6]) or raw(*a, **kw))
    monkeypatch.setattr(minimizer, "SMALL_BATCH", 16)                         # (a batch of more residues than this gets an estimate)
    rng = np.random.Generator(np.random.PCG64(83))
    k, w = 12, 10
    random, dense = [mc.random_record(rng, 20000), mc.random_record(rng, 9000)], [b"A" * 20000, mc.random_record(rng, 500), b"C" * 9000]
    for records, ncalls in [(random, 1), (dense, 2)]:
        del calls[:]
        bases, offsets = mc.pack(records)
        got = minimizer.minimizers(bases, offsets, k, w, canonical=True, order="hashed")
        _same(got, mc.batch_minimizers(records, k, w, True, mc.HASHED), "estimate")
        total = int(got[0].sum())
        assert len(calls) == ncalls and calls[0] == minimizer.list_capacity(bases.size, w) < bases.size
        assert (calls[0] >= total) if ncalls == 1 else (calls[0] < total == calls[1])


def test_bad_arguments_raise_before_the_device_is_touched(dev, monkeypatch):
    from kmerdb_amd import distance, minimizer

    def touched(*a, **kw):
        raise AssertionError("the device was asked")
    monkeypatch.setattr(minimizer, "minimizers_raw", touched)
    monkeypatch.setattr(distance, "_require_device", touched)
    bases, offsets = b"ACGTACGTAC", [0, 10]
    for k, w, order, err in [(0, 2, "hashed", ValueError), (32, 2, "hashed", ValueError), (3, 0, "hashed", ValueError), (3, 257, "hashed", ValueError),
                             (3.0, 2, "hashed", TypeError), (3, True, "hashed", TypeError), (3, 2, "random", ValueError), (3, 2, 1, TypeError)]:
        with pytest.raises(err):
            minimizer.minimizers(bases, offsets, k, w, order=order)
        with pytest.raises(err):
            list(minimizer.minimizers_file(CONTIGS, k, w, order=order))
    for bad_bases, bad_offsets, err in [("ACGT", [0, 4], TypeError), (np.zeros(4, dtype=np.int32), [0, 4], TypeError), (bases, [0, 9], ValueError),
                                        (bases, [1, 10], ValueError), (bases, [0, 7, 5, 10], ValueError), (bases, [], ValueError)]:
        with pytest.raises(err):
            minimizer.minimizers(bad_bases, bad_offsets, 3, 2)
    with pytest.raises(TypeError):
        list(minimizer.minimizers_file(5, 3, 2))
    with pytest.raises(ValueError):
        list(minimizer.minimizers_file(CONTIGS, 15, 10, block_bytes=99))
    with pytest.raises(AssertionError):
        minimizer.minimizers(bases, offsets, 3, 2)
