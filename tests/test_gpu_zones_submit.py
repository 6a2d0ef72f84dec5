"""GPU: what a submit may touch of the caller's residues and offsets, and when the caller may have them back.

Device-resident input (kdb_submit_device, kdb_submit_device_const): the residues are a payload of exactly nbytes inside 1 MiB zones
(tests/zones.py), the offsets a payload of nreads + 1 words with all ones behind it.  Every case runs three times with the zones around
the residues filled with 'A', with 'N' and with 0xFF: a kernel that takes a byte from beside the buffer for a residue counts a window
too many, one too few, or a bad residue -- the counts, the totals and the status must be the oracle's all three times.  After the sync
both payloads and all four zones are bit-identical: the direct-atomics kernel's record marks (bit 7 of a record's first byte) are off
again and none was set outside.

Host input (kdb_submit, kdb_submit_ex, kdb_submit_pinned): the header promises that kdb_submit's buffers "may be reused as soon as it
returns" and that a pinned buffer is free "until two further kdb_submit_pinned calls have returned", its offsets at once.  The drivers of
tests/zones.py overwrite what the engine said it was done with -- residues with 0xFF, offsets with all ones -- at the first moment the
contract allows, and the result must still be the oracle's.  What the two prove: a correct engine must pass.  An engine that reads the
caller's memory late fails whenever the overwrite wins the race against the late read; with 4-8 MB per submit, whose last pieces are
still on their way to the device when the call returns, that is likely but not certain (tests/test_zones_cpu.py shows the drivers
failing stand-in engines that lose the race every time)."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import zones  # noqa: E402

pytestmark = pytest.mark.gpu

LET = np.frombuffer(b"ACGTN", dtype=np.uint8)
ALL_ONES = np.uint64(0xFFFFFFFFFFFFFFFF)
Q = 9                                                  # 16 q + 1 = 145 = 5 x 29, 16 q + 15 = 159 = 3 x 53, 4096 + 7 = 11 x 373
FILLS = (ord("A"), ord("N"), 0xFF)


def _residues(rng, n, p_n=0.01):
    return LET[rng.choice(5, size=n, p=[(1 - p_n) / 4] * 4 + [p_n])].copy()


def _sizes(k):
    return (k, k + 1, 16 * Q + 1, 16 * Q + 15, 4096 + 7)


def _uniform_lengths(k, nbytes):
    """records of one length that fill nbytes exactly: the smallest divisor of nbytes that is at least k"""
    L = next(d for d in range(k, nbytes + 1) if nbytes % d == 0)
    return [L] * (nbytes // L)


def _ragged_lengths(rng, k, nbytes):
    """records of k .. 3 k residues; the last one ends exactly at nbytes"""
    lens, left = [], nbytes
    while left:
        L = int(rng.integers(k, 3 * k + 1))
        if left - L < k:
            L = left
        lens.append(L)
        left -= L
    return lens


def _sparse(oracle, bases, offsets, k):
    """the oracle's ids of every record -> (ids ascending, counts, total)"""
    ids = [oracle.c_shred(bytes(bases[int(s):int(e)]), k, True, oracle.N_DROP)[0] for s, e in zip(offsets[:-1], offsets[1:]) if e - s >= k]
    ids = np.concatenate(ids) if ids else np.zeros(0, dtype=np.uint64)
    u, c = np.unique(ids, return_counts=True)
    return u.astype(np.uint64), c.astype(np.uint64), int(ids.size)


def _vector_at(eng, u):
    import torch
    t = eng.table_tensor()
    return t[torch.as_tensor(u.astype(np.int64), device=t.device)].cpu().numpy().view(np.uint64)


def _error_counts(eng):
    n_short, n_bad = ctypes.c_uint64(0), ctypes.c_uint64(0)
    assert eng._lib.kdb_error_counts(eng._h, ctypes.byref(n_short), ctypes.byref(n_bad)) == 0
    return n_short.value, n_bad.value


# ---- residues and offsets in HBM ----

@pytest.mark.parametrize("algo", [1, 2])
@pytest.mark.parametrize("k", [3, 8, 11, 14])
def test_device_submits_read_their_buffers_alone_and_leave_them_as_they_were(gpu_engine_cls, oracle, k, algo):
    from kmerdb_amd import _abi
    rng = np.random.default_rng(300 + 10 * k + algo)
    with gpu_engine_cls(k, algo=algo) as eng:
        for nbytes in _sizes(k):
            bases = _residues(rng, nbytes)
            bases[0], bases[-1] = ord("C"), ord("G")                          # a first and a last window that count, whatever was drawn
            zb = zones.Zoned(nbytes).write(bases)
            assert zb.ptr % 16 == 0
            shapes = [("uniform", _uniform_lengths(k, nbytes), False), ("ragged", _ragged_lengths(rng, k, nbytes), False),
                      ("ragged, empty last record", _ragged_lengths(rng, k, nbytes) + [0], True)]
            for shape, lens, short in shapes:
                offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
                assert int(offsets[-1]) == nbytes
                zo = zones.Zoned(offsets.size * 8, fill=0xFF).write(offsets)
                u, c, total = _sparse(oracle, bases, offsets, k)
                ragged = len(set(lens)) > 1
                for const in (False, True):
                    for fill in FILLS:
                        tag = "k=%d algo=%d nbytes=%d %s const=%d zones 0x%02X" % (k, algo, nbytes, shape, const, fill)
                        zb.refill_zones(fill)
                        zb.sync()
                        (eng.submit_device_const if const else eng.submit_device)(zb.ptr, nbytes, zo.ptr, len(lens))
                        rc = eng._lib.kdb_sync(eng._h)
                        zb.assert_clean(tag + ": residues")
                        zo.assert_clean(tag + ": offsets")
                        if short:
                            # "min_len" 0 means k: an empty record is the reference's "shorter than k" (kmer.py:461-463) and the sync says so
                            # (that error comes first); what lies beside the buffer must still not show: one short record, no bad residue
                            assert rc == _abi.KDB_ERR_SHORT_READ and _error_counts(eng) == (1, 0), tag
                        elif const and ragged and algo == 1:                    # documented: that kernel would have to mark the buffer
                            assert rc == _abi.KDB_ERR_ARG and "kdb_submit_device_const" in _abi.last_error(), tag
                        else:
                            assert rc == _abi.KDB_OK, tag + ": " + _abi.last_error()
                            assert _error_counts(eng) == (0, 0), tag
                            _, got_total, got_unique = eng.finish(copy=False)
                            assert (got_total, got_unique) == (total, u.size), tag
                            assert np.array_equal(_vector_at(eng, u), c), tag
                        eng.reset()


# ---- kdb_submit and kdb_submit_ex: the caller's arrays overwritten the moment the call is back ----

HOST_K = (6, 11, 14)
HOST_OPTS = [{"stage_bytes": sb, "accum_bytes": ab, "copy_threads": ct} for sb in (4096, None) for ab in (0, 1 << 20) for ct in (1, 8)]
_opts_id = lambda o: "stage%s-accum%d-threads%d" % (o["stage_bytes"] or "default", o["accum_bytes"], o["copy_threads"])


def _reads(rng, nbytes):
    """reads of 100-150 bp, about nbytes of them -> (bases, offsets)"""
    lens = rng.integers(100, 151, size=nbytes // 125)
    return _residues(rng, int(lens.sum()), 0.002), np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)


def _expected(oracle, batches, k):
    """the oracle over the batches (a continuation piece joins the record before it) -> (ids, counts, total): dense counting, then
    the bins that are not zero"""
    dense = np.zeros(4 ** k, dtype=np.uint64)
    total = sum(oracle.c_count(b, o, k, True, oracle.N_DROP, counts=dense)[1] for b, o in batches)
    u = np.flatnonzero(dense).astype(np.uint64)
    return u, dense[u], total


@pytest.fixture(scope="module")
def host_jobs(oracle):
    """per k: the submits of one job -- two of reads (4 MB and 5 MB) and one record of 9 MB handed over in two pieces, the second a
    KDB_SUBMIT_CONTINUES piece that starts with the last k - 1 residues of the first -- and the oracle's answer, computed once"""
    jobs = {}
    for k in HOST_K:
        rng = np.random.default_rng(500 + k)
        a, b = _reads(rng, 4 << 20), _reads(rng, 5 << 20)
        long_record = _residues(rng, 9 << 20, 0.0005)
        cut = (9 << 20) // 2 + 7
        whole = (long_record, np.array([0, long_record.size], dtype=np.uint64))
        pieces = [(long_record[:cut], np.array([0, cut], dtype=np.uint64)),
                  (long_record[cut - (k - 1):], np.array([0, long_record.size - cut + k - 1], dtype=np.uint64))]
        jobs[k] = ([a, b] + pieces, [False, False, False, True], _expected(oracle, [a, b, whole], k))
    return jobs


def _engine(cls, k, opts):
    eng = cls(k)
    for name, value in opts.items():
        if value is not None:
            eng.set_option(name, value)
    return eng


def _check(eng, want):
    u, c, total = want
    _, got_total, got_unique = eng.finish(copy=False)         # (raises on any error status)
    assert (got_total, got_unique) == (total, u.size)
    assert np.array_equal(_vector_at(eng, u), c)


@pytest.mark.parametrize("opts", HOST_OPTS, ids=_opts_id)
@pytest.mark.parametrize("k", HOST_K)
def test_submit_has_let_go_of_the_callers_arrays_when_it_returns(gpu_engine_cls, host_jobs, k, opts):
    batches, continues, want = host_jobs[k]
    with _engine(gpu_engine_cls, k, opts) as eng:
        zones.drive_submit_poisoned(eng, batches, continues)
        _check(eng, want)


# ---- kdb_submit_pinned: three buffers in a ring ----

PINNED_CALLS = 9


@pytest.fixture(scope="module")
def pinned_jobs(oracle, gpu_engine_cls):
    """per k: nine calls of different sizes and contents (0.5-1.5 MB of reads each) and the oracle's answer; one ring of three pinned
    buffers for all of them"""
    from kmerdb_amd.engine import pinned_empty
    jobs = {}
    for k in HOST_K:
        rng = np.random.default_rng(700 + k)
        batches = [_reads(rng, int(rng.integers(1 << 19, 3 << 19))) for _ in range(PINNED_CALLS)]
        jobs[k] = (batches, _expected(oracle, batches, k))
    size = max(b.size for batches, _ in jobs.values() for b, _ in batches)
    return jobs, [pinned_empty(size) for _ in range(3)]


@pytest.mark.parametrize("opts", HOST_OPTS, ids=_opts_id)
@pytest.mark.parametrize("k", HOST_K)
def test_a_ring_of_three_pinned_buffers_is_enough(gpu_engine_cls, pinned_jobs, k, opts):
    jobs, ring = pinned_jobs
    batches, want = jobs[k]
    with _engine(gpu_engine_cls, k, opts) as eng:
        zones.drive_pinned_ring_poisoned(eng, batches, ring)
        _check(eng, want)


def test_parsefile_feeds_a_fastq_of_a_dozen_blocks_through_its_ring(gpu_engine_cls, oracle, tmp_path, monkeypatch):
    """the product's own pinned feed, parse._feed_file over the reader's ring of three, with blocks of 64 KiB instead of 128 MiB"""
    from kmerdb_amd import parse, reader
    k = 11
    rng = np.random.default_rng(900)
    bases, offsets = _reads(rng, 12 * 65536 // 2)                              # (a FASTQ record is twice its residues and a little more)
    path = tmp_path / "dozen.fastq"
    with open(path, "wb") as f:
        for r, (s, e) in enumerate(zip(offsets[:-1], offsets[1:])):
            seq = bytes(bases[int(s):int(e)])
            f.write(b"@r%d\n%s\n+\n%s\n" % (r, seq, b"I" * len(seq)))
    monkeypatch.setattr(reader, "BLOCK_BYTES", 65536)
    nblocks = sum(1 for _ in reader.BlockReader(str(path)))
    assert nblocks >= 12
    counts, metadata, nullomers = parse.parsefile(str(path), k, replace_with_none=True)
    want, total = oracle.c_count(bases, offsets, k, True, oracle.N_DROP)
    assert np.array_equal(counts, want) and metadata["total_kmers"] == total and metadata["total_reads"] == offsets.size - 1
    assert np.array_equal(nullomers, np.flatnonzero(want == 0))
