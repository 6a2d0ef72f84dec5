"""GPU: kdb_record_tables -- one k-mer table per record (csrc/kdb_tables.hip.h) -- against the numpy restatement of tests/tables_cases.py,
and the layers above it: kmerdb_amd.composition, kmerdb_amd.codons and the `composition`, `codons` and `CUB` subcommands.

Every output is an integer and compared exactly.  Every test here fails without kdb_record_tables: the library does not export the symbol."""
import contextlib
import ctypes
import io
import json
import math
import os
import re

import numpy as np
import pytest

import tables_cases as tc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
CDS = os.path.join(GOLDEN, "inputs", "cds.fa")


def _header_constant(name):
    text = open(os.path.join(ROOT, "include", "kdbhip.h")).read()
    return int(re.search(r"#define\s+%s\s+(\d+)" % name, text).group(1))


PIECE, CONTINUES = _header_constant("KDB_TABLES_PIECE"), _header_constant("KDB_TABLES_CONTINUES")
COMBINATIONS = sorted({(k, s) for k in range(1, 7) for s in (1, k)} | {(6, 3), (4, 2)})


@pytest.fixture(scope="module")
def dev(gpu_engine_cls):
    from kmerdb_amd import _abi

    class Dev:
        lib = _abi.lib()
        OK, ARG, BAD = _abi.KDB_OK, _abi.KDB_ERR_ARG, _abi.KDB_ERR_BAD_RESIDUE

        @classmethod
        def raw(cls, bases, offsets, k, stride, canonical=0, phase=0, flags=0, nreads=None, nbytes=None, null=(), rows=None):
            """kdb_record_tables with the arguments as given, the host output buffers filled with 0xFF -> (status, the five buffers)"""
            m = max(len(offsets) - 1, 1)                                     # (the buffers follow the offsets given, not a claimed nreads)
            n = len(offsets) - 1 if nreads is None else nreads
            outs = [np.full((m if rows is None else rows, 4 ** min(max(k, 1), 6)), 0xFFFFFFFF, dtype=np.uint32), np.full(m, 2 ** 64 - 1, dtype=np.uint64),
                    np.full(m, 2 ** 64 - 1, dtype=np.uint64), np.full(m, -1431655766, dtype=np.int32), np.full(m, -1431655766, dtype=np.int32)]
            po = [None if i in null else o.ctypes.data for i, o in enumerate(outs)]
            rc = cls.lib.kdb_record_tables(0, k, stride, canonical, phase, None if "bases" in null or bases.size == 0 else bases.ctypes.data,
                                           bases.size if nbytes is None else nbytes, None if "offsets" in null else offsets.ctypes.data, n, flags,
                                           po[0], po[1], po[2], po[3], po[4], None)
            return rc, outs

        @classmethod
        def tables(cls, records, k, stride=1, canonical=False, phase=0, continues=False):
            bases, offsets = tc.pack(records)
            rc, outs = cls.raw(bases, offsets, k, stride, 1 if canonical else 0, phase, CONTINUES if continues else 0)
            assert rc == cls.OK, _abi.last_error()
            return outs
    return Dev


def _untouched(outs):
    return bool(np.all(outs[0] == 0xFFFFFFFF) and np.all(outs[1] == 2 ** 64 - 1) and np.all(outs[2] == 2 ** 64 - 1)
                and np.all(outs[3] == -1431655766) and np.all(outs[4] == -1431655766))


def _check(dev, records, k, stride, canonical, phase=0, continues=False, name=""):
    got = dev.tables(records, k, stride, canonical, phase, continues)
    want = tc.batch_tables(records, k, stride, canonical, phase, continues)
    for r in range(len(records)):
        where = (name, k, stride, canonical, r, len(records[r]))
        assert tuple(int(g[r]) for g in got[1:]) == tuple(int(w[r]) for w in want[1:]), where
        assert got[0][r].tobytes() == want[0][r].tobytes(), where + (np.flatnonzero(got[0][r] != want[0][r])[:8].tolist(),)
    return got


# ---- every parameter combination, at every edge of the kernel ----

@pytest.mark.parametrize("canonical", [False, True])
@pytest.mark.parametrize("k,stride", COMBINATIONS)
def test_every_parameter_combination_at_the_kernels_edges(dev, k, stride, canonical):
    records = tc.ladder_records(k, stride, PIECE, 100 * k + stride)
    tables, windows, skipped, first, last = _check(dev, records, k, stride, canonical)
    npieces = [max(1, -(-int(w + s) // PIECE)) for w, s in zip(windows, skipped)]
    assert sorted(set(npieces)) == [1, 2, 3] and npieces.count(3) == 2 and int(skipped.sum()) > 0
    assert [len(r) for r in records[:5]] == [0, 1, k - 1, k, k + 1] and (int(first[0]), int(last[0])) == (-1, -1)
    assert int(tables.sum(dtype=np.uint64)) == int(windows.sum())


# ---- N layouts, one bin, the smallest table ----

def test_n_layouts_and_single_bin_records(dev):
    rng = np.random.Generator(np.random.PCG64(5))
    for k, stride in [(3, 3), (4, 1), (6, 3), (1, 1)]:
        L = tc.length_for(2 * PIECE + 1, k, stride)
        base = bytearray(tc.random_record(rng, L))
        first_n, last_n, across = bytearray(base), bytearray(base), bytearray(base)
        first_n[k - 1] = ord("N")                                            # the first window only (and its neighbours at stride < k)
        last_n[L - 1] = ord("N")
        at = PIECE * stride                                                   # the first residue of piece 1's first window
        across[at - 1:at + 1] = b"NN"                                         # the last window of piece 0 and the first of piece 1
        records = [bytes(first_n), b"N" * 100, bytes(last_n), b"ACGT" * 5, bytes(across), b"N" * (k - 1), b"A" * L, b"N" * k, b"T" * (PIECE // 2)]
        tables, windows, skipped, first, last = _check(dev, records, k, stride, k % 2 == 0, name="n layouts")
        assert (int(windows[1]), int(first[1]), int(last[1])) == (0, -1, -1) and int(skipped[1]) == len(tc.window_starts(100, k, stride))
        assert int(skipped[0]) >= 1 and int(skipped[2]) >= 1 and int(skipped[4]) >= (2 if k > 1 else 1)
        # poly-A over three pieces: one bin, through the atomic row path; poly-T in one piece: one bin, through the stored row
        assert int(tables[6][0]) == 2 * PIECE + 1 == int(tables[6].sum()) and int(np.count_nonzero(tables[8])) == 1
    _check(dev, [b"ACGT" * 16, b"A" * 64, b"ACGTNACG" * 8, b"C" * 63 + b"G"], 1, 1, False, name="k = 1, 64 residues")


def test_seventy_thousand_records(dev):
    """more records, pieces and workgroups than 16 bits count"""
    n, L, k = 70000, 12, 3
    rng = np.random.Generator(np.random.PCG64(70000))
    bases = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=n * L)].copy()
    bases[rng.random(n * L) < 0.01] = ord("N")
    offsets = np.arange(n + 1, dtype=np.uint64) * np.uint64(L)
    rc, (tables, windows, skipped, first, last) = dev.raw(bases, offsets, k, 3)
    assert rc == dev.OK
    codes = tc.CODE[bases].reshape(n, L // 3, 3)
    ok = np.all(codes >= 0, axis=2)
    ids = (np.where(codes >= 0, codes, 0) * np.array([16, 4, 1])).sum(axis=2)
    want = np.zeros((n, 64), dtype=np.uint32)
    rows, cols = np.nonzero(ok)
    np.add.at(want, (rows, ids[rows, cols]), 1)
    assert tables.tobytes() == want.tobytes()
    assert windows.tolist() == ok.sum(axis=1).tolist() and skipped.tolist() == (~ok).sum(axis=1).tolist()
    has = ok.any(axis=1)
    f = np.where(has, ids[np.arange(n), np.argmax(ok, axis=1)], -1)
    l = np.where(has, ids[np.arange(n), L // 3 - 1 - np.argmax(ok[:, ::-1], axis=1)], -1)
    assert first.tolist() == f.tolist() and last.tolist() == l.tolist()
    for r in (0, 1, 65535, 65536, 65537, n - 1):                             # (the restatement proper, on a few)
        row, w, s, fi, la = tc.record_table(bases[r * L:(r + 1) * L].tobytes(), k, 3)
        assert (tables[r].tolist(), int(windows[r]), int(skipped[r]), int(first[r]), int(last[r])) == (row.tolist(), w, s, fi, la)


# ---- the piece and record counts of whole genomes ----

def test_more_multi_piece_records_than_the_zeroing_grid_has_workgroups(dev):
    """tables_zero_kernel is launched with at most 4096 workgroups and strides through the records of more than one piece: 4113 of them,
    two pieces each, with single-piece and empty records in between so that they are no contiguous range of rows"""
    nmulti, k = 4096 + 17, 2
    L = tc.length_for(PIECE + 3, k, 1)
    rng = np.random.Generator(np.random.PCG64(4113))
    block = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=(nmulti, L))].copy()
    block[rng.random((nmulti, L)) < 0.001] = ord("N")
    block[5, :PIECE + 1] = ord("N")                                           # a first piece without a counted window
    block[6, PIECE:] = ord("N")                                               # ... and a second one
    block[7, :] = ord("N")
    small = {i: np.frombuffer(tc.random_record(rng, int(rng.integers(k, 60)), 0.02), dtype=np.uint8) for i in range(0, nmulti, 3)}
    empty = set(range(0, nmulti, 7))
    parts, lens, rows_multi, rows_small = [], [], [], []
    for i in range(nmulti):
        rows_multi.append(len(lens))
        parts.append(block[i])
        lens.append(L)
        if i in small:
            rows_small.append(len(lens))
            parts.append(small[i])
            lens.append(small[i].size)
        if i in empty:
            lens.append(0)
    offsets = np.concatenate(([0], np.cumsum(lens))).astype(np.uint64)
    bases = np.concatenate(parts)
    n = len(lens)
    assert bases.size == int(offsets[-1]) and nmulti > 4096 and rows_multi[-1] - rows_multi[0] + 1 > nmulti
    want = [np.zeros((n, 4 ** k), dtype=np.uint32), np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint64), np.full(n, -1, dtype=np.int32), np.full(n, -1, dtype=np.int32)]
    for w, u in zip(want, tc.uniform_tables(block, k)):
        w[rows_multi] = u
    for w, u in zip(want, tc.batch_tables([small[i].tobytes() for i in sorted(small)], k)):
        w[rows_small] = u
    # The same shapes first as poly-T: where the allocator hands the second call the first one's block, the rows that have to be zeroed hold
    # PIECE + 3 in their last entry then.  Best effort: nothing here can tell whether the block was reused, and nothing asserts it.
    stale = np.where(bases == ord("N"), bases, np.uint8(ord("T")))
    rc, (tables, windows, skipped, first, last) = dev.raw(stale, offsets, k, 1)
    assert rc == dev.OK and int(tables[rows_multi[0]][15]) == PIECE + 3 - int(skipped[rows_multi[0]]) and not tables[:, :15].any()
    rc, got = dev.raw(bases, offsets, k, 1)
    assert rc == dev.OK
    for name, g, w in zip(("tables", "windows", "skipped", "first_id", "last_id"), got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, name
        assert g.tobytes() == w.tobytes(), (name, np.argwhere(g != w)[:8].tolist())
    assert 0 < int(got[1][rows_multi[5]]) <= 2 and int(got[3][rows_multi[5]]) >= 0 and int(got[4][rows_multi[6]]) >= 0
    assert [int(g[rows_multi[7]]) for g in got[1:]] == [0, PIECE + 3, -1, -1] and not got[0][rows_multi[7]].any()
    for r in (rows_multi[0], rows_multi[5], rows_multi[6], rows_multi[7], rows_multi[4095], rows_multi[4096], rows_multi[4097], rows_multi[-1], n - 1):
        row, w, s, fi, la = tc.record_table(bases[int(offsets[r]):int(offsets[r + 1])].tobytes(), k)       # (the restatement proper, on a few)
        assert (got[0][r].tolist(), int(got[1][r]), int(got[2][r]), int(got[3][r]), int(got[4][r])) == (row.tolist(), w, s, fi, la), r


@pytest.mark.parametrize("canonical", [False, True])
@pytest.mark.parametrize("k,stride", [(1, 1), (3, 3), (6, 1), (6, 6)])
def test_a_record_of_a_hundred_and_fifty_pieces(dev, k, stride, canonical):
    """a contig of more than a megabase: every entry of its row is added to by the waves of 150 pieces"""
    rng = np.random.Generator(np.random.PCG64(150 * k + stride))
    nwin = 150 * PIECE + 77
    contig = bytearray(tc.random_record(rng, tc.length_for(nwin, k, stride) + stride - 1))
    for at in rng.integers(0, len(contig), size=12).tolist():
        contig[at] = ord("N")
    records = [tc.random_record(rng, 50, 0.02), b"", bytes(contig), tc.random_record(rng, k), tc.random_record(rng, tc.length_for(PIECE + 1, k, stride)), b"N" * 40]
    tables, windows, skipped, first, last = _check(dev, records, k, stride, canonical, name="150 pieces")
    assert int(windows[2] + skipped[2]) == nwin > 150 * PIECE and 0 < int(skipped[2]) <= 12 * k
    assert int(tables[2].sum(dtype=np.uint64)) == int(windows[2]) and int(tables.sum(dtype=np.uint64)) == int(windows.sum())


@pytest.mark.parametrize("k,stride,canonical", [(3, 3, True), (4, 1, False), (6, 3, True), (1, 1, False), (2, 1, True)])
def test_pieces_without_a_counted_window_at_a_records_ends(dev, k, stride, canonical):
    """tables_record_kernel joins the pieces' first and last ids in piece order and passes over a piece that reports -1: a record whose
    pieces 0, 1 and 4 of five are all N has both from its interior, and one that is N over three pieces has neither"""
    rng = np.random.Generator(np.random.PCG64(31 * k + stride))
    L = tc.length_for(5 * PIECE, k, stride)
    rec = bytearray(tc.random_record(rng, L))
    rec[:2 * PIECE * stride] = b"N" * (2 * PIECE * stride)                   # the windows 0 .. 2 PIECE - 1 begin with an N
    rec[4 * PIECE * stride:] = b"N" * (L - 4 * PIECE * stride)                # ... and so do those from 4 PIECE on
    inner = bytearray(tc.random_record(rng, L))                               # the mirror: only the pieces 0 and 4 count anything
    inner[PIECE * stride:4 * PIECE * stride] = b"N" * (3 * PIECE * stride)
    all_n = b"N" * tc.length_for(2 * PIECE + 5, k, stride)
    records = [tc.random_record(rng, 70), bytes(rec), all_n, b"", bytes(inner), tc.random_record(rng, 33, 0.1), all_n, bytes(rec)]
    tables, windows, skipped, first, last = _check(dev, records, k, stride, canonical, name="pieces of N")
    assert int(windows[1] + skipped[1]) == 5 * PIECE and 2 * PIECE - k < int(windows[1]) <= 2 * PIECE and int(first[1]) >= 0 and int(last[1]) >= 0
    assert (int(windows[2]), int(skipped[2]), int(first[2]), int(last[2])) == (0, 2 * PIECE + 5, -1, -1) and not tables[2].any()
    assert int(skipped[4]) >= 3 * PIECE and int(first[4]) >= 0 and int(last[4]) >= 0
    for r in (1, 4):                                                          # the ids are those of the first and last window without an N
        s = records[r]
        starts = [p for p in tc.window_starts(len(s), k, stride).tolist() if b"N" not in s[p:p + k]]
        ids = [int(tc.record_table(s[p:p + k], k, 1, canonical)[3]) for p in (starts[0], starts[-1])]
        assert (int(first[r]), int(last[r])) == tuple(ids), r
        assert (2 * PIECE <= starts[0] // stride < 3 * PIECE and starts[-1] // stride < 4 * PIECE) if r == 1 else (starts[0] == 0 and starts[-1] // stride >= 4 * PIECE)


def test_a_records_row_does_not_depend_on_the_batch(dev):
    k, stride = 5, 2
    records = tc.ladder_records(k, stride, PIECE, 9)
    whole = dev.tables(records, k, stride, True)
    back = dev.tables(records[::-1], k, stride, True)
    again = dev.tables(records, k, stride, True)
    for a, b, c in zip(whole, back, again):
        assert a.tobytes() == b[::-1].tobytes() == c.tobytes()
    for r in (1, 6, len(records) - 2):                                       # alone: a multi-piece record among them
        alone = dev.tables([records[r]], k, stride, True)
        assert all(a[0].tobytes() == w[r].tobytes() for a, w in zip(alone, whole))
    assert any(len(tc.window_starts(len(records[r]), k, stride)) > PIECE for r in (1, 6, len(records) - 2))


# ---- continuation ----

def test_a_record_cut_at_every_position_adds_up(dev):
    k, stride = 6, 3
    rng = np.random.Generator(np.random.PCG64(40))
    rec = bytearray(tc.random_record(rng, 40))
    rec[17] = ord("N")
    rec = bytes(rec)
    other = tc.random_record(rng, 33)
    whole = [x[0] for x in dev.tables([rec], k, stride, True)]
    phases = set()
    for cut in range(1, 40):
        begin, phase = tc.split_phase(cut, k, stride)
        assert 0 <= phase < stride
        phases.add(phase)
        a = [x[-1] for x in dev.tables([other, rec[:cut]], k, stride, True)]
        b = [x[0] for x in _check(dev, [rec[begin:], other], k, stride, True, phase=phase, continues=True, name="cut %d" % cut)]
        assert (a[0].astype(np.uint64) + b[0]).tolist() == whole[0].tolist(), cut
        assert (int(a[1] + b[1]), int(a[2] + b[2])) == (int(whole[1]), int(whole[2])), cut
        assert (int(a[3]) if a[3] >= 0 else int(b[3])) == int(whole[3]) and (int(b[4]) if b[4] >= 0 else int(a[4])) == int(whole[4]), cut
    assert phases == {0, 1, 2}


def test_tables_file_joins_the_pieces_of_streamed_records(dev, tmp_path):
    from kmerdb_amd import composition
    rng = np.random.Generator(np.random.PCG64(41))
    recs = [("r%d" % i, tc.random_record(rng, n, 0.01).decode()) for i, n in enumerate([40, 1000, 7, 333, 2 * PIECE + 50, 5])]
    path = tc.write_fasta(tmp_path / "wrapped.fa", recs, 50)
    for k, stride, bb in [(6, 3, 128), (3, 3, 200), (4, 1, 1000), (4, 1, None)]:
        got = list(composition.tables_file(path, k, stride=stride, canonical=True, block_bytes=bb))
        assert [g[0] for g in got] == [r[0] for r in recs]
        for g, (rid, s) in zip(got, recs):
            row, windows, skipped, first_id, last_id = tc.record_table(s.encode(), k, stride, True)
            assert g[1:6] == (len(s), windows, skipped, first_id, last_id), (k, stride, bb, rid)
            assert g[6].dtype == np.uint64 and g[6].tolist() == row.tolist(), (k, stride, bb, rid)


def test_call_entries_cap_splits_a_block(dev, tmp_path, monkeypatch):
    from kmerdb_amd import composition
    rng = np.random.Generator(np.random.PCG64(42))
    recs = [("r%d" % i, tc.random_record(rng, 30 + i).decode()) for i in range(11)]
    path = tc.write_fasta(tmp_path / "many.fa", recs)
    monkeypatch.setattr(composition, "MAX_CALL_ENTRIES", 3 * 4 ** 4)          # three records of k = 4 per call
    got = list(composition.tables_file(path, 4, canonical=False))
    assert [(g[0], g[6].tolist()) for g in got] == [(rid, tc.record_table(s.encode(), 4)[0].tolist()) for rid, s in recs]


# ---- refusals ----

def test_refusals_by_status(dev):
    bases, offsets = tc.pack([b"ACGTACGTAC", b"ACGTNACGT"])
    ok = lambda **kw: dev.raw(bases, offsets, **{"k": 3, "stride": 3, **kw})[0]
    assert ok() == dev.OK
    for k in (0, 7, -1, 17):
        assert ok(k=k, stride=1) == dev.ARG
    for stride in (0, 4, -1):
        assert ok(stride=stride) == dev.ARG
    assert ok(phase=3, flags=CONTINUES) == dev.ARG and ok(phase=1) == dev.ARG and ok(phase=2, flags=CONTINUES) == dev.OK
    assert ok(flags=2) == dev.ARG and ok(flags=3) == dev.ARG
    for null in ("bases", "offsets", 0, 1, 2, 3, 4):
        assert ok(null=(null,)) == dev.ARG, null
    for bad in ([1, 10, 19], [0, 10, 18], [0, 12, 11, 19], [0, 25, 19]):
        assert dev.raw(bases, np.array(bad, dtype=np.uint64), 3, 3)[0] == dev.ARG, bad
    assert dev.raw(bases, offsets, 3, 3, nbytes=(1 << 30) + 1)[0] == dev.ARG
    assert dev.raw(bases, offsets, 3, 3, nreads=(1 << 30) + 1)[0] == dev.ARG
    assert dev.raw(bases, offsets, 3, 3, nreads=0)[0] == dev.ARG              # residues but no records
    assert dev.raw(bases[:0], offsets[:1], 3, 3)[0] == dev.OK                 # nothing at all
    # 524 289 empty records at k = 6: one row above 2^31 entries; 524 288 are allowed, but nothing of that size is asked for here
    assert dev.raw(bases[:0], np.zeros(524289 + 1, dtype=np.uint64), 6, 1, rows=1)[0] == dev.ARG
    from kmerdb_amd import composition
    with pytest.raises(ValueError):
        composition.record_tables(b"ACGTRACGT", [0, 9], 3)


def test_bad_residues_leave_the_outputs_untouched(dev):
    good = b"ACGTNACGTACGTTGCA" * 3
    for bad in (b"R", b"a", b"n", b"\x80", b"\xff", b"\x00", b" "):
        for at in (0, 20, len(good) - 1):
            rec = good[:at] + bad + good[at + 1:]
            bases, offsets = tc.pack([good, rec, good])
            rc, outs = dev.raw(bases, offsets, 4, 1)
            assert rc == dev.BAD and _untouched(outs), (bad, at)
    rc, outs = dev.raw(*tc.pack([good, b"ANRNA"]), 3, 3)                     # an IUPAC letter that only shares windows with an N: refused too
    assert rc == dev.BAD and _untouched(outs)
    rc, outs = dev.raw(*tc.pack([good]), 4, 1)
    assert rc == dev.OK and not _untouched(outs)


# ---- files and subcommands ----

@pytest.fixture(scope="module")
def golden():
    return json.load(open(os.path.join(GOLDEN, "codons.json")))


@pytest.fixture(scope="module")
def sequences():
    return dict(tc.read_fasta(CDS))


def _main(argv):
    from kmerdb_amd import profile
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        assert profile.main(argv) == 0
    return out.getvalue()


def test_codons_as_reference_equals_the_reference(dev, golden, sequences, tmp_path):
    from kmerdb_amd import codons, kmer
    ok = [c for c in golden["records"] if not c["codon_frequency_table"][0]["raises"]]
    path = tc.write_fasta(tmp_path / "ok.fa", [(c["id"], sequences[c["id"]]) for c in ok])
    for f, (start, stop) in enumerate(golden["flags"]):
        ids, counts, flags = codons.codon_tables(path, include_start_codons=start, include_stop_codons=stop, include_noncanonicals=True, as_reference=True)
        assert ids == [c["id"] for c in ok]
        assert counts.tolist() == [c["codon_frequency_table"][f]["value"][1] for c in ok]
        assert flags.tolist() == [c["get_codons_in_order"]["value"][1] for c in ok]
    # cds.fa itself: the length refusals can be ignored, three triplets with an N cannot
    with pytest.raises(ValueError, match="n_three"):
        codons.codon_tables(CDS, include_noncanonicals=True, ignore_invalid_cds=True, as_reference=True)
    with pytest.raises(ValueError, match="non-canonical"):
        codons.codon_tables(CDS, as_reference=True)
    # the subcommand's text
    text = _main(["codons", "--as-reference", "--include-noncanonicals", path]).splitlines()
    assert text[0].split("\t") == [""] + [kmer.id_to_kmer(i, 3) for i in range(64)]
    assert [line.split("\t") for line in text[1:]] == [[c["id"]] + [str(x) for x in c["codon_frequency_table"][0]["value"][1]] for c in ok]
    # one sequence, the reference's tuple
    for c in ok[:4] + ok[-2:]:
        ids, counts, wrt_length, in_family = codons.codon_frequency_table(sequences[c["id"]], c["id"], as_reference=True)
        want = c["codon_frequency_table"][0]["value"]
        assert ids == want[0] and counts.tolist() == want[1]
        assert np.array_equal(np.array(wrt_length), np.array(want[2]), equal_nan=True) and np.array_equal(np.array(in_family), np.array(want[3]), equal_nan=True)
        assert codons.is_sequence_cds(sequences[c["id"]], as_reference=True) is bool(c["is_sequence_cds"][0]["value"])


def test_codons_by_default_count_forward_ids(dev, sequences, tmp_path):
    from kmerdb_amd import codons
    names = [i for i, s in sequences.items() if len(s) % 3 == 0 and "N" not in s and len(s) >= 9]
    path = tc.write_fasta(tmp_path / "genes.fa", [(i, sequences[i]) for i in names])
    ids, counts, flags = codons.codon_tables(path, include_noncanonicals=True)
    assert ids == names
    for i, row, flag in zip(ids, counts, flags):
        s = sequences[i].encode()
        want, _, _, first_id, last_id = tc.record_table(s, 3, 3)
        assert row.tolist() == tc.record_table(s[3:-3], 3, 3)[0].tolist(), i
        assert bool(flag) == (first_id not in (14, 46, 62) or last_id not in (48, 50, 56)), i
    assert flags.tolist() == [i in ("start_ccc", "stop_ccc") for i in ids]   # TAG, TGA and GTG are what they are under forward ids


def test_composition_of_contigs(dev):
    from kmerdb_amd import kmer
    path = os.path.join(GOLDEN, "inputs", "contigs.fa")
    recs = tc.read_fasta(path)
    lines = [line.split("\t") for line in _main(["composition", "-k", "4", path]).splitlines()]
    cols = [i for i in range(256) if i <= int(tc.rc_ids([i], 4)[0])]
    assert len(cols) == 136 and lines[0] == ["id", "length", "windows"] + [kmer.id_to_kmer(i, 4) for i in cols] and len(lines) == len(recs) + 1
    for line, (rid, s) in zip(lines[1:], recs):
        row, windows, _, _, _ = tc.record_table(s.upper().encode(), 4, 1, True)
        assert line == [rid, str(len(s)), str(windows)] + [str(int(c)) for c in row[cols]], rid
    freq = [line.split("\t") for line in _main(["composition", "-k", "2", "--do-not-canonicalize", "--as-frequencies", path]).splitlines()]
    for line, (rid, s) in zip(freq[1:], recs):
        row, windows, _, _, _ = tc.record_table(s.upper().encode(), 2, 1, False)
        assert line[3:] == [repr(int(c) / windows) for c in row], rid


def test_cub_end_to_end(dev, golden, sequences, tmp_path):
    genes = tc.write_fasta(tmp_path / "genes.fa", [(i, sequences[i]) for i in golden["table_ids"]])
    table = tmp_path / "table.tsv"
    table.write_text(_main(["codons", "--include-noncanonicals", genes]))
    lines = [line.split("\t") for line in _main(["CUB", "--sequences", genes, str(table)]).splitlines()]
    want = [c for c in golden["cub"] if c["chisq"] is not None]
    assert lines[0] == ["", "chisq", "pval"] and [line[0] for line in lines[1:]] == [c["id"] for c in want]
    for line, c in zip(lines[1:], want):
        chisq = float(line[1])
        assert line[2] == "nan"
        assert math.isnan(chisq) if math.isnan(c["chisq"]) else abs(chisq - c["chisq"]) <= 64 * 2.0 ** -53 * c["chisq"], c["id"]
