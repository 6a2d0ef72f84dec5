"""GPU: what the engine may touch of a count vector that the caller owns.  The vector handed to kdb_create (and the two of
kdb_strand_merge, and the n of kdb_reduce) is the payload of a tests/zones.py allocation: exactly 4^k words with 1 MiB of 0xA5 on either
side.  After every step of an engine's life -- create, each submit, sync, finish, table_stats, nullomers, fold_file, reset, destroy --
both zones must still hold the poison, and after the sync the vector must be the oracle's.  Every counting path is taken at the smallest
k that reaches it: count vectors go down to 32 bytes at k = 1, the paged paths cut the vector into buckets and runs, the two-level path
sweeps it in a deferred pass, the direct path and the hot-id shortcuts add to single bins (the first and the last one here: poly-A and
poly-T reads of 70 000 windows).

Alignment (DESIGN, "What a call may touch"): the histogram pass of the paged paths moves the vector in 16-byte pieces, so kdb_create
refuses a vector that is not 16-byte aligned, whatever k; the refusal is tested and no engine runs on such a vector.  kdb_strand_merge's
two kernels touch both vectors 8 bytes at a time, as its comment says: it runs at shift 8 too."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import zones  # noqa: E402
from test_gpu_strand_merge import rc_ids  # noqa: E402

pytestmark = pytest.mark.gpu

DROP, EXPAND = 0, 1
SPARSE_FROM_K = 13                                     # as tests/fuzz_gpu.py: the oracle's ids instead of its dense vector
LONG = 70000                                           # windows of each single-bin read: wrap notes (16-bit counters) and the hot-id shortcut
LET = np.frombuffer(b"ACGTN", dtype=np.uint8)
STAGE = {"stage_bytes": 1 << 20, "stage_reads": 1 << 14, "accum_bytes": 0}     # small host staging: every submit is one batch, engines are cheap


def _batches(k, canon):
    """two submits: ragged reads of 35-150 bp with a little N (a few thousand in all), each followed by one read that loads a single bin
    LONG times -- forward: poly-A (bin 0) and poly-T (the last bin); canonical: poly-A and (AC)n"""
    rng = np.random.default_rng(1000 + k)
    out = []
    for long_read in ((b"A", b"T") if not canon else (b"A", b"AC")):
        lens = rng.integers(35, 151, size=1500)
        ragged = LET[rng.choice(5, size=int(lens.sum()), p=[0.2495] * 4 + [0.002])]
        tail = np.frombuffer((long_read * (LONG + k))[:LONG + k - 1], dtype=np.uint8)
        bases = np.concatenate([ragged, tail])
        offsets = np.concatenate([[0], np.cumsum(np.concatenate([lens, [tail.size]]))]).astype(np.uint64)
        out.append((bases, offsets))
    return out


_WANT = {}


def _want(oracle, k, canon, mode):
    """-> (batches, per batch and for both: dense vector (k < 13) or (ids, counts), total, unique); computed once per (k, canon, mode)"""
    key = (k, canon, mode)
    if key not in _WANT:
        batches = _batches(k, canon)
        omode = oracle.N_EXPAND if mode == EXPAND else oracle.N_DROP

        shredded = {}

        def ids_of(i):
            if i not in shredded:
                b, o = batches[i]
                shredded[i] = np.concatenate([oracle.c_shred(bytes(b[int(s):int(e)]), k, canon, omode)[0] for s, e in zip(o[:-1], o[1:])])
            return shredded[i]

        def count(which):
            if k < SPARSE_FROM_K:
                dense = np.zeros(4 ** k, dtype=np.uint64)
                total = sum(oracle.c_count(*batches[i], k, canon, omode, counts=dense)[1] for i in which)
                return dense, total, int(np.count_nonzero(dense))
            ids = np.concatenate([ids_of(i) for i in which])
            u, c = np.unique(ids, return_counts=True)
            return (u, c.astype(np.uint64)), int(ids.size), int(u.size)
        _WANT[key] = (batches, count((0, 1)), count((0,)))
    return _WANT[key]


def _vector_is(z, want, k):
    import torch
    if k < SPARSE_FROM_K:
        return np.array_equal(z.read(np.uint64), want)
    u, c = want
    t = z.view(torch.int64)
    got = t[torch.as_tensor(u.astype(np.int64), device=t.device)].cpu().numpy().view(np.uint64)
    return np.array_equal(got, c)                     # (with Sum and count_nonzero equal, as the caller checks, every other bin is zero)


def _is_zero(z):
    import torch
    return not bool(z.view(torch.int64).any())


def _life(cls, z, oracle, k, canon, mode, algo, opts):
    """one engine's life on the zoned vector `z`, the zones checked after every step"""
    import torch
    from kmerdb_amd import _abi
    batches, (want, want_total, want_unique), (want0, want0_total, want0_unique) = _want(oracle, k, canon, mode)
    tag = "k=%d canonical=%d n_mode=%d algo=%s %s: " % (k, canon, mode, algo, opts)
    nbins = 4 ** k
    z.view(torch.int64).fill_(-1)                     # create must zero the vector: start from ones
    z.sync()
    eng = cls(k, canonicalize=bool(canon), n_mode=mode, table_ptr=z.ptr, algo=algo)
    try:
        z.assert_zones(tag + "kdb_create")
        assert _is_zero(z), tag + "kdb_create zeroes the vector"
        for name, value in dict(STAGE, **opts).items():
            eng.set_option(name, value)
        for i, (b, o) in enumerate(batches):
            eng.submit(b, o)
            z.assert_zones(tag + "submit %d" % i)
        eng.sync()
        z.assert_zones(tag + "kdb_sync")
        assert _vector_is(z, want, k), tag + "the vector after the sync"
        counts, total, unique = eng.finish(copy=k < SPARSE_FROM_K)
        z.assert_zones(tag + "kdb_finish")
        assert (total, unique) == (want_total, want_unique), tag + "totals"
        assert counts is None or np.array_equal(counts, want)
        _, s, u = eng.table_stats(copy=False)
        z.assert_zones(tag + "kdb_table_stats")
        assert (s, u) == (want_total, want_unique)
        if k < SPARSE_FROM_K:
            assert np.array_equal(eng.nullomers(nbins - want_unique), np.flatnonzero(want == 0).astype(np.uint64))
        else:
            n = ctypes.c_uint64(0)
            _abi.check(eng._lib.kdb_nullomers(eng._h, 0, None, 0, ctypes.byref(n)))
            assert n.value == nbins - want_unique
        z.assert_zones(tag + "kdb_nullomers")
        assert _vector_is(z, want, k), tag + "the readers left the vector alone"
        assert eng.fold_file() == (want_total, want_unique)
        z.assert_zones(tag + "kdb_fold_file")
        assert _is_zero(z), tag + "the fold clears the file's vector"
        eng.submit(*batches[0])                        # the next file, then a reset with its counts in the vector
        eng.sync()
        z.assert_zones(tag + "the second file")
        assert _vector_is(z, want0, k) and eng.finish(copy=False)[1:] == (want0_total, want0_unique)
        eng.reset()
        z.assert_zones(tag + "kdb_reset")
        assert _is_zero(z), tag + "kdb_reset zeroes the vector"
    finally:
        eng.close()
    z.sync()
    z.assert_zones(tag + "kdb_destroy")
    assert _is_zero(z)


ALL4 = [(0, DROP), (1, DROP), (0, EXPAND), (1, EXPAND)]
TWO = [(0, DROP), (1, EXPAND)]


def _cases():
    out = []
    add = lambda path, k, algo, opts, modes: out.extend(pytest.param(k, c, m, algo, opts, id="%s-k%d-c%d-m%d-%s" % (path, k, c, m, "_".join("%s%d" % kv for kv in opts.items()) or "default"))
                                                        for c, m in modes)
    for k in (1, 2, 3, 4, 8):                                                  # count_smallk_kernel
        add("smallk", k, None, {}, ALL4 if k in (3, 8) else TWO)
    for k in (3, 8):                                                           # count_lds_kernel; k = 8 through the paged scatter
        add("smallk_old", k, None, {"smallk_old": 1}, TWO)
    for k in (9, 11):                                                          # one scatter level + page_hist_kernel
        add("one_level", k, None, {}, ALL4)
        for opts in ({"one_level_defer": 0}, {"sc_wide_lines": 0}, {"one_level_defer": 0, "sc_wide_lines": 0}):
            add("one_level", k, None, opts, TWO)
    add("ring1024", 13, None, {}, ALL4)                                        # 1024 rings + the pass over 16-bit bins
    add("direct", 3, 1, {}, ALL4)                                              # global atomics
    add("direct", 11, 1, {}, ALL4)
    add("staging", 9, None, {"strand_merge": 1}, [(1, DROP)])                  # canonical engines: forward ids staged, merged at the sync
    add("staging", 9, None, {"strand_merge": 0}, [(1, DROP)])
    add("staging", 12, None, {"strand_merge": 1}, [(1, DROP)])
    add("staging", 12, None, {"strand_merge": 0}, [(1, DROP)])
    return out


@pytest.mark.parametrize("k,canon,mode,algo,opts", _cases())
def test_an_engines_life_on_a_zoned_vector(gpu_engine_cls, oracle, k, canon, mode, algo, opts):
    _life(gpu_engine_cls, zones.Zoned(4 ** k * 8), oracle, k, canon, mode, algo, opts)


@pytest.fixture(scope="module")
def two_gib():
    """the 4^14 words of k = 14, allocated once"""
    import torch
    z = zones.Zoned(4 ** 14 * 8)
    yield z
    del z
    torch.cuda.empty_cache()


@pytest.mark.parametrize("canon,mode,opts", [pytest.param(c, m, {"defer_flush": 1}, id="defer1-c%d-m%d" % (c, m)) for c, m in ALL4]
                         + [pytest.param(c, m, {"defer_flush": 0}, id="defer0-c%d-m%d" % (c, m)) for c, m in TWO])
def test_the_two_level_path_on_a_zoned_vector_of_2_gib(gpu_engine_cls, oracle, two_gib, canon, mode, opts):
    _life(gpu_engine_cls, two_gib, oracle, 14, canon, mode, None, opts)


@pytest.mark.parametrize("k", [1, 3, 9])
def test_a_vector_that_is_not_16_byte_aligned_is_refused_untouched(gpu_engine_cls, k):
    """the finding of the alignment review: kdb_create refuses such a vector at every k, and neither zeroes it nor keeps the pointer"""
    from kmerdb_amd import _abi
    z = zones.zoned_words(np.full(4 ** k, 7, dtype=np.uint64), shift=8)
    z.sync()
    h = ctypes.c_void_p(1)
    assert _abi.lib().kdb_create(k, 1, DROP, 0, ctypes.c_void_p(z.ptr), ctypes.byref(h)) == _abi.KDB_ERR_ARG
    assert "16-byte aligned" in _abi.last_error() and not h.value
    with pytest.raises(ValueError, match="16-byte aligned"):
        gpu_engine_cls(k, table_ptr=z.ptr, algo=1)
    z.sync()
    z.assert_clean("kdb_create refused")


# ---- kdb_strand_merge on two vectors of the caller's ----

@pytest.mark.parametrize("shift", [0, 8])
@pytest.mark.parametrize("k", [1, 2, 3, 8, 9, 12])
def test_strand_merge_touches_the_canonical_bins_of_two_zoned_vectors(gpu_engine_cls, k, shift):
    """d_fwd is all zero afterwards; the bins of d_table with i > rc(i) keep a sentinel; the rest is the definition; no zone changes.
    Both kernels (one thread per id up to k = 8, pairs of 64 x 64 tiles from k = 9) read and write single words: 8-byte alignment is
    all the entry point asks, so shift 8 runs."""
    from kmerdb_amd import _abi
    n = 4 ** k
    rng = np.random.default_rng(50 + k)
    fwd = (rng.poisson(2.0, n) * rng.integers(0, 2, n)).astype(np.uint64)
    fwd[0], fwd[-1] = 70000, 2 ** 33 + 1                                       # AA..A and TT..T: each other's reverse complement, the first and the last word
    table = rng.integers(0, 1000, n).astype(np.uint64)
    ids = np.arange(n, dtype=np.uint64)
    upper = ids > rc_ids(ids, k)                                              # the bins the call may not touch
    sentinel = np.uint64(0xDEADBEEFCAFEF00D)
    table[upper] = sentinel
    rc = rc_ids(ids, k)
    want = table + np.where(ids < rc, fwd + fwd[rc], np.where(ids == rc, fwd, np.uint64(0)))         # the header's definition
    assert np.all(want[upper] == sentinel)
    zf, zt = zones.zoned_words(fwd, shift=shift), zones.zoned_words(table, shift=shift)
    zf.sync()
    _abi.check(_abi.lib().kdb_strand_merge(0, ctypes.c_void_p(zf.ptr), ctypes.c_void_p(zt.ptr), k))
    zf.assert_zones("kdb_strand_merge's d_fwd, k=%d shift=%d" % (k, shift))
    zt.assert_zones("kdb_strand_merge's d_table, k=%d shift=%d" % (k, shift))
    assert not zf.read(np.uint64).any()
    got = zt.read(np.uint64)
    assert np.all(got[upper] == sentinel)
    assert np.array_equal(got, want)


# ---- kdb_reduce over adopted vectors ----

@pytest.mark.parametrize("k,n", [(1, 3), (2, 16), (5, 3)])
def test_reduce_sums_into_every_root_inside_the_zones(gpu_engine_cls, oracle, k, n):
    """the slices are cut with & ~1: at k = 1 and n = 3 they are [0, 0), [0, 2), [2, 4); at k = 2 and n = 16 every other one is empty.
    The root's vector is the sum; the other payloads may change (the header says so), no zone may."""
    from kmerdb_amd.engine import reduce_engines
    rng = np.random.default_rng(70 + k)
    reads = []
    for j in range(n):
        lens = rng.integers(k, k + 40, size=5 + j)
        reads.append((LET[rng.integers(0, 4, int(lens.sum()))].copy(), np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)))
    want = np.zeros(4 ** k, dtype=np.uint64)
    want_total = sum(oracle.c_count(b, o, k, True, oracle.N_DROP, counts=want)[1] for b, o in reads)
    zs = [zones.Zoned(4 ** k * 8) for _ in range(n)]
    engines = [gpu_engine_cls(k, table_ptr=z.ptr) for z in zs]
    try:
        for eng in engines:
            for name, value in STAGE.items():
                eng.set_option(name, value)
        for root in range(n):
            for eng, (b, o) in zip(engines, reads):
                eng.reset()
                eng.submit(b, o)
            reduce_engines(engines, root)
            for j, z in enumerate(zs):
                z.assert_zones("kdb_reduce k=%d n=%d root=%d, vector %d" % (k, n, root, j))
            assert np.array_equal(zs[root].read(np.uint64), want), root
            counts, total, unique = engines[root].finish()
            assert np.array_equal(counts, want) and total == want_total and unique == np.count_nonzero(want)
    finally:
        for eng in engines:
            eng.close()
    for j, z in enumerate(zs):
        z.sync()
        z.assert_zones("kdb_destroy after kdb_reduce, vector %d" % j)
