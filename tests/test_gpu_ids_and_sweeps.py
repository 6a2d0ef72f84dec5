"""GPU: the kernels beside the counting paths, against the oracle or a closed-form expectation (exact integers throughout).

The ids path -- lens_kernel, hibit_check_kernel, mark_reads_kernel, shred_kernel, resolve_suspects_kernel behind
kdb_window_ids / kdb_shred -- on batches of several tiles whose record starts, N's and ends lie on every side of a tile
(16 384 residues) and chunk (16) edge; inputs and expected values come from tests/ids_cases.py.
The sweeps over the count vector -- stats_kernel, null_count / null_scan / null_write_kernel, reduce_slice_kernel -- on
vectors written through table_tensor(), which counting random reads never produces.
"""
import ctypes
from collections import Counter

import numpy as np
import pytest

import ids_cases as ic
from ids_cases import T

pytestmark = pytest.mark.gpu

ALL_K = list(range(1, 18))
SUSPECTS_CAP = 1 << 16              # kdb_engine.hip: suspects_cap, the length of the list resolve_suspects_kernel reads


def _assert_ids(got, want, offsets, *what):
    msg = ic.describe_mismatch(got, want, offsets)
    assert msg == "", what + (msg,)


def _window_ids_rc(eng, bases, offsets):
    """kdb_window_ids with its status: -> (rc, ids)."""
    bases = np.ascontiguousarray(bases, dtype=np.uint8)
    offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
    ids = np.empty(bases.size, dtype=np.uint64)
    rc = eng._lib.kdb_window_ids(eng._h, bases.ctypes.data, bases.size, offsets.ctypes.data, len(offsets) - 1, ids.ctypes.data)
    return rc, ids


# ---------------------------------------------------------------------------------------------------------------
# C. the ids path
# ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", ALL_K)
def test_ragged_window_ids_at_tile_and_chunk_edges(gpu_engine_cls, k):
    """kdb_window_ids on ragged batches of three tiles and a partial last chunk: lens_kernel (max != min length),
    mark_reads_kernel's bit-7 marks at -17 .. +17 of a tile edge and at every chunk offset, shred_kernel's halo chunk,
    its window_crosses / vwin test (records of exactly k residues across an edge, N's at -17 .. +17 of one) and its
    `p0 + i >= nbytes` cut; buffers that end at T - 1, T and T + 1."""
    from kmerdb_amd.engine import ids_engine
    for lay in ic.ragged_family(k):
        for canon in (True, False):
            want = ic.expected_window_ids(lay.bases, lay.offsets, k, canon)
            got = ids_engine(k, canon).window_ids(lay.bases, lay.offsets)
            _assert_ids(got, want, lay.offsets, lay.name, canon)


@pytest.mark.parametrize("k", ALL_K)
def test_uniform_window_ids_and_the_same_residues_with_marks(gpu_engine_cls, k):
    """Records of one length L (batch_uniform_len != 0: UniformStarts / uniform_starts compute the record starts, its loop
    for L < 16 and its single-start form for L >= 16, L around a tile's size) and the same residues with one record a
    residue longer (the marks branch): both equal the oracle."""
    from kmerdb_amd.engine import ids_engine
    for L in ic.uniform_lengths(k):
        lay = ic.uniform_layout(k, L)
        re = ic.rebatch_ragged(lay, k)
        for canon in (True, False):
            eng = ids_engine(k, canon)
            for form in (lay, re):
                want = ic.expected_window_ids(form.bases, form.offsets, k, canon)
                _assert_ids(eng.window_ids(form.bases, form.offsets), want, form.offsets, form.name, canon)


@pytest.mark.parametrize("k", ALL_K)
def test_single_record_shred_and_its_scratch(gpu_engine_cls, oracle, k):
    """kdb_shred (no offsets: resolve_suspects_kernel's one-record form, no lens / mark kernels) on records of k .. 2 T + 9
    residues with N's; one engine takes a large record, a small one, then a larger one: the scratch of window_ids_run (kdb_engine.hip) is
    reused, then grown."""
    from kmerdb_amd.engine import IdsEngine
    rest = [L for L in ic.single_lengths(k) if L not in (T, k, 2 * T + 9)]
    for canon in (True, False):
        with IdsEngine(k, canon) as eng:                       # a fresh engine: no scratch yet
            for L in [T, k, 2 * T + 9] + rest:
                rec = ic.single_record(k, L)
                want_ids, want_pos = oracle.c_shred(rec, k, canon, oracle.N_DROP)
                ids, pos = eng.shred(rec)
                assert np.array_equal(pos, want_pos) and np.array_equal(ids, want_ids), (k, canon, L)
            ids, pos = eng.shred(b"N" * k)                     # a record without any window
            assert ids.size == 0 and pos.size == 0 and oracle.c_shred(b"N" * k, k, canon, oracle.N_DROP)[0].size == 0


def _error_layouts(k):
    """[(layout, tile edge, record edge)]: a ragged and a uniform batch of two tiles; the tile edge lies inside a record,
    the record edge far from a tile edge."""
    rng = np.random.Generator(np.random.PCG64(8086 + k))
    total, B = 2 * T + 100, 4999
    points = [0, B, T - 120, T + 130, total]
    starts = []
    for lo, hi in zip(points[:-1], points[1:]):
        starts += ic.cut_records(rng, lo, hi, k)
    ragged = ic.Layout("ragged", ic.random_bases(rng, total), np.array(starts + [total], dtype=np.uint64))
    nrec = 2 * T // 150 + 1
    uniform = ic.Layout("uniform", ic.random_bases(rng, nrec * 150), np.arange(nrec + 1, dtype=np.uint64) * np.uint64(150))
    return [(ragged, T, B), (uniform, T, 40 * 150)]


@pytest.mark.parametrize("k", [2, 9, 17])
def test_window_ids_errors_agree_with_the_oracle(gpu_engine_cls, oracle, k):
    """What the reference refuses, at -1, 0, +1 of a tile edge and of a record edge: an IUPAC code that no N shields
    (resolve_suspects_kernel finds its record by binary search in the offsets), a lowercase letter, a byte with bit 7 set
    (hibit_check_kernel; in a ragged batch the byte may sit where mark_reads_kernel puts a mark) -> KDB_ERR_BAD_RESIDUE; a shielded code -> the oracle's ids; a record of k - 1
    residues behind a tile edge -> KDB_ERR_SHORT_READ (lens_kernel); offsets that do not tile the buffer -> KDB_ERR_ARG
    (host check, and lens_kernel's bad_layout)."""
    from kmerdb_amd import _abi
    from kmerdb_amd.engine import IdsEngine
    canon = k != 9
    with IdsEngine(k, canon) as eng:
        for lay, tile_edge, rec_edge in _error_layouts(k):
            offs = lay.offsets.astype(np.int64)
            clean = ic.expected_window_ids(lay.bases, lay.offsets, k, canon)
            for p in [e + d for e in (tile_edge, rec_edge) for d in (-1, 0, 1)]:
                r = int(np.searchsorted(offs, p, side="right")) - 1
                s, e = int(offs[r]), int(offs[r + 1])
                for name, byte in (("unshielded R", ord("R")), ("lowercase", ord("a")), ("bit 7", 0xC1)):
                    b = lay.bases.copy()
                    b[p] = byte
                    with pytest.raises(oracle.OracleError) as ei:
                        oracle.c_shred(b[s:e].tobytes(), k, canon, oracle.N_DROP)
                    assert ei.value.status == oracle.BAD_RESIDUE
                    rc, _ = _window_ids_rc(eng, b, lay.offsets)
                    assert rc == _abi.KDB_ERR_BAD_RESIDUE, (lay.name, name, p, rc, _abi.last_error())
                b = lay.bases.copy()
                b[p] = ord("R")
                for q in (p - 1, p + 1):                       # an N on either side, inside the record: no window holds the R alone
                    if s <= q < e:
                        b[q] = ord("N")
                want = ic.expected_window_ids(b, lay.offsets, k, canon)
                assert np.all(want[max(s, p - k + 1):p + 1] == ic.NO_WINDOW) and not np.array_equal(want, clean)
                rc, got = _window_ids_rc(eng, b, lay.offsets)
                assert rc == _abi.KDB_OK, (lay.name, "shielded R", p, rc, _abi.last_error())
                _assert_ids(got, want, lay.offsets, lay.name, "shielded R", p)
            # offsets that do not tile the buffer
            for at, delta in ((-1, -1), (-1, 1), (0, 1)):
                bad = lay.offsets.copy()
                bad[at] = np.uint64(int(bad[at]) + delta)
                rc, _ = _window_ids_rc(eng, lay.bases, bad)
                assert rc == _abi.KDB_ERR_ARG, (lay.name, at, delta, rc)
            bad = lay.offsets.copy()
            bad[[7, 8]] = bad[[8, 7]]                          # record 7 ends before it starts
            rc, _ = _window_ids_rc(eng, lay.bases, bad)
            assert rc == _abi.KDB_ERR_ARG, (lay.name, "decreasing offsets", rc)
            # the engine is none the worse for any of it
            _assert_ids(eng.window_ids(lay.bases, lay.offsets), clean, lay.offsets, lay.name, "clean batch after the errors")
        # a record of k - 1 residues right behind a tile edge
        rng = np.random.Generator(np.random.PCG64(31 + k))
        total = 2 * T + 100
        starts = ic.cut_records(rng, 0, T, k) + [T] + ic.cut_records(rng, T + k - 1, total, k)
        offsets = np.array(starts + [total], dtype=np.uint64)
        bases = ic.random_bases(rng, total)
        with pytest.raises(oracle.OracleError) as ei:
            ic.expected_window_ids(bases, offsets, k, canon)
        assert ei.value.status == oracle.SHORT_READ
        rc, _ = _window_ids_rc(eng, bases, offsets)
        assert rc == _abi.KDB_ERR_SHORT_READ, (rc, _abi.last_error())


@pytest.mark.parametrize("k", [2, 9, 17])
def test_window_ids_with_more_shielded_codes_than_the_suspects_list_holds(gpu_engine_cls, oracle, k):
    """More IUPAC codes between N's than suspects_cap in one ragged batch: sus_count runs past the list and
    resolve_suspects_kernel takes its overflow branch -- every residue judged in place, the buffer's partial last chunk by
    one lane, the record of each found by binary search.  Ids equal the oracle's; one code that no N shields still raises."""
    from kmerdb_amd import _abi
    from kmerdb_amd.engine import IdsEngine
    rng = np.random.Generator(np.random.PCG64(6502 + k))
    codes = np.frombuffer(b"RYSWKMBDHV", dtype=np.uint8)
    recs = []
    for i in range(760):
        masked = np.full(270, ord("N"), dtype=np.uint8)
        masked[1::3] = codes[rng.integers(0, 10, size=90)]                     # N?N N?N ...: every window with a code holds an N
        recs.append(np.concatenate([ic.random_bases(rng, 30 + i % 16), masked]))
    if sum(len(r) for r in recs) % 16 < 2:                                     # the last code lies in a partial last chunk
        recs[0] = np.concatenate([ic.random_bases(rng, 2), recs[0]])
    bases = np.concatenate(recs)
    offsets = np.concatenate([[0], np.cumsum([len(r) for r in recs])]).astype(np.uint64)
    assert int(np.isin(bases, codes).sum()) > SUSPECTS_CAP + 1000 and bases.size % 16 >= 2 and bases[-2] in codes
    for canon in (True, False):
        want = ic.expected_window_ids(bases, offsets, k, canon)
        assert int(np.sum(want != ic.NO_WINDOW)) == sum(len(r) - 270 - k + 1 for r in recs)
        with IdsEngine(k, canon) as eng:
            rc, got = _window_ids_rc(eng, bases, offsets)
            assert rc == _abi.KDB_OK, (rc, _abi.last_error())
            _assert_ids(got, want, offsets, "overflowing suspects list", canon)
            bad = bases.copy()
            at = int(offsets[380]) + 15                                        # in the N-free head of a record: k residues without N around it
            bad[at] = ord("R")
            with pytest.raises(oracle.OracleError) as ei:
                ic.expected_window_ids(bad, offsets, k, canon)
            assert ei.value.status == oracle.BAD_RESIDUE
            rc, _ = _window_ids_rc(eng, bad, offsets)
            assert rc == _abi.KDB_ERR_BAD_RESIDUE, (rc, _abi.last_error())


@pytest.fixture(scope="module")
def graph_files(tmp_path_factory):
    """{kind: (path, [(seq_id, seq)])}: FASTQ of equal-length reads, FASTQ of ragged reads, FASTA of three records longer than a tile."""
    d = tmp_path_factory.mktemp("graph_inputs")
    out = {}
    for kind, writer, suffix in (("uniform", ic.write_fastq, ".fq"), ("ragged", ic.write_fastq, ".fq"), ("long", ic.write_fasta, ".fa")):
        recs = ic.graph_records(kind)
        path = str(d / (kind + suffix))
        writer(path, recs)
        out[kind] = (path, recs)
    return out


@pytest.mark.parametrize("k", [9, 13])
@pytest.mark.parametrize("kind", ["uniform", "ragged", "long"])
def test_graph_rows_over_several_tiles_and_blocks(gpu_engine_cls, oracle, graph_files, monkeypatch, kind, k):
    """graph.make_edges_from_fasta (window_ids on blocks of several tiles: the uniform branch, the marks branch, records
    longer than a tile) == oracle.py_make_edges, row for row; a FASTQ that arrives in blocks of 8 KiB gives the same rows,
    seq_ids and metadata; edge_counts + weighted_edges == the Counter of the rows."""
    from kmerdb_amd import graph
    path, recs = graph_files[kind]
    lens = [len(s) for _, s in recs]
    bases, offsets = oracle.pack_records([s for _, s in recs])
    for canon in (True, False):
        want_rows = oracle.py_make_edges(recs, k, canonicalize=canon)
        assert len(want_rows) == sum(n - k for n in lens)
        want_counts, want_total = oracle.c_count(bases, offsets, k, canon, oracle.N_DROP)
        rows, meta, counts = graph.make_edges_from_fasta(path, k, canonicalize=canon)
        assert len(rows) == len(want_rows)
        assert rows == want_rows, next((i, a, b) for i, (a, b) in enumerate(zip(rows, want_rows)) if a != b)
        assert np.array_equal(counts, want_counts)
        unique = int(np.count_nonzero(want_counts))
        assert {x: meta[x] for x in ("filename", "total_reads", "num_reads", "total_kmers", "unique_kmers", "nullomers", "min_read_length",
                                     "max_read_length", "avg_read_length")} == {
            "filename": path, "total_reads": len(recs), "num_reads": len(recs), "total_kmers": want_total, "unique_kmers": unique,
            "nullomers": 4 ** k - unique if not canon else int(4 ** k / 2 - unique), "min_read_length": min(lens),
            "max_read_length": max(lens), "avg_read_length": int(np.mean(lens))}
        if kind != "long":
            real, blocks = graph.reader.iter_blocks, []

            def small_blocks(p, want_ids=False, block_bytes=None, pinned=False):
                for blk in real(p, want_ids=want_ids, block_bytes=8192, pinned=pinned):
                    blocks.append(len(blk[1]) - 1)
                    yield blk

            with monkeypatch.context() as m:
                m.setattr(graph.reader, "iter_blocks", small_blocks)
                rows2, meta2, counts2 = graph.make_edges_from_fasta(path, k, canonicalize=canon)
            assert len(blocks) > 5 and sum(blocks) == len(recs)
            assert rows2 == want_rows and meta2 == meta and np.array_equal(counts2, want_counts)
        ev, ecounts, n_edges = graph.edge_counts(path, k, canonicalize=canon)
        assert n_edges == len(want_rows) == int(ev.sum()) and np.array_equal(ecounts, want_counts)
        id1, id2, w = graph.weighted_edges(ev, k, canonicalize=canon)
        assert {(int(a), int(b)): int(x) for a, b, x in zip(id1, id2, w)} == dict(Counter((r[2], r[4]) for r in want_rows))


# ---------------------------------------------------------------------------------------------------------------
# D. the sweeps over the count vector
# ---------------------------------------------------------------------------------------------------------------

def _write_vector(eng, values):
    """values: uint64[4^k] on the host -> the engine's vector."""
    import torch
    t = eng.table_tensor()                                     # from here on the vector is the caller's (kdb_table: table_escaped)
    t.copy_(torch.from_numpy(np.ascontiguousarray(values, dtype=np.uint64).view(np.int64)))
    torch.cuda.synchronize()                                   # (the engine's streams do not wait for torch's)


def _nullomer_count(eng):
    n = ctypes.c_uint64(0)
    assert eng._lib.kdb_nullomers(eng._h, 0, None, 0, ctypes.byref(n)) == 0
    return n.value


NULL_LANE, NULL_WAVE, NULL_TILE, NULL_RANGE = 8, 512, 2048, 1 << 25       # bins per lane, wave, tile and range of the null_* kernels


def _edge_bins(r, rng):
    """bins of range r: the first and last bin of the first, second, a middle and the last lane group, wave and tile of
    the range (the range's own first and last bin among them), and a few hundred random ones."""
    base = r * NULL_RANGE
    bins = set(int(x) for x in base + rng.integers(0, NULL_RANGE, size=300))
    for unit in (NULL_LANE, NULL_WAVE, NULL_TILE):
        for j in (0, 1, int(rng.integers(2, NULL_RANGE // unit - 1)), NULL_RANGE // unit - 1):
            bins |= {base + j * unit, base + j * unit + unit - 1}
    return bins


@pytest.mark.parametrize("k,range_sets", [(13, [(0, 1), (0,), (1,)]), (14, [tuple(range(8)), (1, 2, 4, 6), (3,), (0, 7)])])
def test_nullomers_of_a_written_vector_closed_form(gpu_engine_cls, k, range_sets):
    """kdb_nullomers on a vector of ones with a known set of zeros: bin 0 and the last bin, the first and last bin of a lane's
    group of 8, of a wave, of a tile and of a range of 2^25 bins; ranges without any zero before, between and behind ranges
    that have some (the `continue` of the write loop, the two output buffers taken by r & 1, also twice in a row).
    null_count_kernel, null_scan_kernel and null_write_kernel must give exactly the sorted set, and its size when only
    counted."""
    import torch
    nranges = 4 ** k // NULL_RANGE
    assert nranges == (2 if k == 13 else 8)
    with gpu_engine_cls(k) as eng:
        t = eng.table_tensor()
        for n_set, ranges in enumerate(range_sets):
            rng = np.random.Generator(np.random.PCG64(1300 * k + n_set))
            bins = set()
            for r in ranges:
                bins |= _edge_bins(r, rng)
            want = np.array(sorted(bins), dtype=np.uint64)
            if ranges[0] == 0 and ranges[-1] == nranges - 1:
                assert want[0] == 0 and want[-1] == 4 ** k - 1
            assert set(int(x) for x in want // np.uint64(NULL_RANGE)) == set(ranges)
            t.fill_(1)
            t[torch.from_numpy(want.astype(np.int64)).to(t.device)] = 0
            torch.cuda.synchronize()
            assert _nullomer_count(eng) == want.size, (k, ranges)
            got = eng.nullomers()
            assert got.dtype == np.uint64 and np.array_equal(got, want), (k, ranges, ic.describe_mismatch(got, want, [0, want.size]) if got.size == want.size else got.size)
            _, s, u = eng.table_stats(copy=False)
            assert (s, u) == (4 ** k - want.size, 4 ** k - want.size)


@pytest.mark.parametrize("pattern", ["alternating", "range 0 all zero", "range 1 all zero"])
def test_nullomers_of_dense_zero_patterns_k13(gpu_engine_cls, pattern):
    """2^25 nullomers: every second bin (every lane's mask is 0x55), or one whole range of 2^25 bins beside a range
    without any (null_scan_kernel's totals at their largest, 256 MiB of ids through one output buffer)."""
    import torch
    k = 13
    with gpu_engine_cls(k) as eng:
        t = eng.table_tensor()
        t.fill_(3)
        if pattern == "alternating":
            t[0::2] = 0
        elif pattern == "range 0 all zero":
            t[:NULL_RANGE] = 0
        else:
            t[NULL_RANGE:] = 0
        torch.cuda.synchronize()
        want = np.flatnonzero(t.cpu().numpy() == 0).astype(np.uint64)
        assert want.size == 1 << 25
        assert _nullomer_count(eng) == want.size
        assert np.array_equal(eng.nullomers(), want)


@pytest.mark.parametrize("k", [1, 2, 3])
def test_nullomers_of_vectors_smaller_than_a_tile(gpu_engine_cls, k):
    """4, 16 and 64 bins: fewer than one lane's group (null_mask8's bounds-checked form) or than one tile; every subset of
    the four bins of k = 1, and a few dozen random masks (all-zero and all-non-zero among them) of the others."""
    nbins = 4 ** k
    rng = np.random.Generator(np.random.PCG64(17 + k))
    if k == 1:
        masks = [np.array([(m >> i) & 1 for i in range(4)], dtype=bool) for m in range(16)]
    else:
        masks = [np.zeros(nbins, dtype=bool), np.ones(nbins, dtype=bool)] + [rng.random(nbins) < p for p in (0.05, 0.3, 0.5, 0.9) for _ in range(12)]
    with gpu_engine_cls(k) as eng:
        for zero in masks:
            vec = np.where(zero, 0, rng.integers(1, 1 << 40, size=nbins)).astype(np.uint64)
            _write_vector(eng, vec)
            want = np.flatnonzero(zero).astype(np.uint64)
            assert _nullomer_count(eng) == want.size
            assert np.array_equal(eng.nullomers(), want), (k, zero)
            assert np.array_equal(eng.nullomers(n=want.size), want)


@pytest.mark.parametrize("k", [1, 6, 13])
def test_table_stats_of_counts_beyond_32_bits(gpu_engine_cls, k):
    """stats_kernel: Sum and count_nonzero of a vector with values up to 2^40 at scattered bins (the first and the last
    among them), and of a vector without any zero whose every value is above 2^32 -- exactly numpy's."""
    import torch
    nbins = 4 ** k
    rng = np.random.Generator(np.random.PCG64(40 + k))
    idx = np.unique(np.concatenate([[0, nbins - 1], rng.integers(0, nbins, size=min(nbins, 3000))])).astype(np.int64)
    vals = rng.integers(1, (1 << 40) + 1, size=idx.size).astype(np.uint64)
    vals[:2] = (1 << 40, (1 << 32) + 1)
    if idx.size > 3:
        vals[2:4] = (1 << 32, (1 << 32) - 1)
    with gpu_engine_cls(k) as eng:
        t = eng.table_tensor()
        t.zero_()
        t[torch.from_numpy(idx).to(t.device)] = torch.from_numpy(vals.view(np.int64)).to(t.device)
        torch.cuda.synchronize()
        counts, s, u = eng.table_stats()
        assert s == sum(int(v) for v in vals) and u == idx.size
        assert np.array_equal(np.flatnonzero(counts), idx) and np.array_equal(counts[idx], vals)
        if k <= 6:
            dense = (np.uint64(1 << 33) + np.arange(nbins, dtype=np.uint64) * np.uint64(0x10001))
            _write_vector(eng, dense)
            counts, s, u = eng.table_stats()
            assert np.array_equal(counts, dense) and s == sum(int(v) for v in dense) and u == nbins
            assert eng.table_stats(copy=False) == (None, s, u)


def _reduce_pattern(j, nbins):
    """engine j's vector: (j + 1) << s with s up to 33, another s in every bin and engine."""
    i = np.arange(nbins, dtype=np.uint64)
    return np.uint64(j + 1) << ((np.uint64(7) * i + np.uint64(5 * j)) % np.uint64(34))


@pytest.mark.parametrize("k,n,root", [(1, 3, 0), (1, 3, 2), (2, 16, 0), (2, 16, 1), (2, 16, 15), (7, 16, 0), (7, 16, 9)])
def test_kdb_reduce_with_empty_slices_and_sixteen_engines(gpu_engine_cls, k, n, root):
    """kdb_reduce where bound[j] = (nbins * j / n) & ~1 leaves slices empty (k = 1, n = 3: engine 0's; k = 2, n = 16: every
    even engine's, the root's own with roots 0) and at KDB_REDUCE_MAX engines (reduce_slice_kernel with 15 peers): the
    root's vector == the numpy sum of distinct written vectors."""
    from kmerdb_amd.engine import reduce_engines
    nbins = 4 ** k
    bound = [(nbins * j // n) & ~1 for j in range(n)] + [nbins]
    empty = [j for j in range(n) if bound[j + 1] <= bound[j]]
    assert empty == {(1, 3): [0], (2, 16): list(range(0, 16, 2)), (7, 16): []}[(k, n)]
    vecs = [_reduce_pattern(j, nbins) for j in range(n)]
    want = np.sum(vecs, axis=0, dtype=np.uint64)
    engines = [gpu_engine_cls(k) for _ in range(n)]
    try:
        for e, v in zip(engines, vecs):
            _write_vector(e, v)
        reduce_engines(engines, root=root)
        got, s, u = engines[root].table_stats()
        assert np.array_equal(got, want), (k, n, root, np.flatnonzero(got != want)[:8])
        assert s == sum(int(x) for x in want) and u == nbins
    finally:
        for e in engines:
            e.close()


def test_kdb_reduce_refuses_seventeen_engines(gpu_engine_cls):
    from kmerdb_amd import _abi
    engines = [gpu_engine_cls(1) for _ in range(17)]
    try:
        for j, e in enumerate(engines):
            _write_vector(e, _reduce_pattern(j, 4))
        arr = (ctypes.c_void_p * 17)(*[e._h for e in engines])
        assert _abi.lib().kdb_reduce(arr, 17, 0) == _abi.KDB_ERR_ARG
        for j, e in enumerate(engines):                         # nothing was summed
            assert np.array_equal(e.table_stats()[0], _reduce_pattern(j, 4))
    finally:
        for e in engines:
            e.close()
