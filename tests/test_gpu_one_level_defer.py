"""GPU: the one-level count step with its page sort and histogram pass deferred (engine option one_level_defer = N, k = 9 .. 12 and k = 13
in one level; csrc/kdb_scatter_host.hip.h: OneLevelPending).

Every vector is compared with the oracle's and, bit for bit over all 4^k bins, with the vector of an engine that runs the immediate path
(one_level_defer = 0) over the same batches; the flush counters are compared with what the rules of tests/defer_model.py give.
References (oracle and immediate engine) are computed once per input and not changed."""
import numpy as np
import pytest

from tests import defer_model as dm

pytestmark = pytest.mark.gpu

LET = np.frombuffer(b"ACGT", dtype=np.uint8)
DROP, EXPAND = 0, 1
MODES = {"forward": (False, DROP, 0.0), "canonical": (True, DROP, 0.0), "expand": (True, EXPAND, 0.005)}
BYTES_PER_PAGE = 1024 + 4 + 8          # a page of the arena, its tag, its list entry


def ragged_batch(seed, n_reads, p_n=0.0, lo=35, hi=150):
    rng = np.random.Generator(np.random.PCG64(seed))
    lens = rng.integers(lo, hi + 1, size=n_reads)
    bases = LET[rng.integers(0, 4, size=int(lens.sum()))].copy()
    if p_n:
        bases[rng.random(bases.size) < p_n] = ord("N")
    offsets = np.zeros(n_reads + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum(lens)
    return bases, offsets


class References:
    """per (k, mode, batches): the oracle's vector and total, checked once against the immediate path's vector"""

    def __init__(self, oracle, engine_cls):
        self.oracle, self.engine_cls, self.memo = oracle, engine_cls, {}

    def want(self, key, k, mode, batches, base=None):
        if key not in self.memo:
            canon, n_mode, _ = MODES[mode]
            counts, total = (None if base is None else base.copy()), 0
            for b, o in batches:
                counts, t = self.oracle.c_count(b, o, k, canon, n_mode, counts=counts)
                total += t
            if base is None:
                with self.engine_cls(k, canonicalize=canon, n_mode=n_mode) as eng:
                    eng.set_option("one_level_defer", 0)
                    for b, o in batches:
                        eng.submit(b, o)
                    got, got_total, _ = eng.finish()
                    assert eng.get_option("hist_flushes") == 0 and eng.get_option("arena_pages") == 0
                assert got_total == total and np.array_equal(got, counts), "the immediate path differs from the oracle"
            counts.setflags(write=False)
            self.memo[key] = (counts, total)
        return self.memo[key]

    def prefix(self, k, mode, batches, n):
        """the first n of `batches` (the module's four): the oracle's vector after each batch and the immediate path's, one run of each"""
        if (k, mode, 1) not in self.memo:
            canon, n_mode, _ = MODES[mode]
            counts, total = None, 0
            with self.engine_cls(k, canonicalize=canon, n_mode=n_mode) as eng:
                eng.set_option("one_level_defer", 0)
                for i, (b, o) in enumerate(batches):
                    counts, t = self.oracle.c_count(b, o, k, canon, n_mode, counts=counts)
                    total += t
                    eng.submit(b, o)
                    got, got_total, _ = eng.table_stats()
                    assert got_total == total and np.array_equal(got, counts), "the immediate path differs from the oracle"
                    got.setflags(write=False)
                    self.memo[(k, mode, i + 1)] = (got, total)
                assert eng.get_option("hist_flushes") == 0 and eng.get_option("arena_pages") == 0
        return self.memo[(k, mode, n)]


@pytest.fixture(scope="module")
def refs(oracle, gpu_engine_cls):
    return References(oracle, gpu_engine_cls)


@pytest.fixture(scope="module")
def batches4():
    """four batches of 50 000 reads of 35..150 bases, with and without 0.5 % N"""
    return {p_n: [ragged_batch(9100 + 10 * i + (1 if p_n else 0), 50_000, p_n) for i in range(4)] for p_n in (0.0, 0.005)}


def flush_counters(eng):
    return tuple(eng.get_option(n) for n in ("one_level_pending", "hist_flushes", "flushed_batches", "full_flushes"))


def check_vector(eng, want, what):
    counts, total = want
    got, got_total, got_unique = eng.finish()
    assert got_total == total, (what, got_total, total)
    bad = np.flatnonzero(got != counts)
    assert bad.size == 0, "%s: %d bins differ, first id %d: got %d, want %d" % (what, bad.size, bad[0], got[bad[0]], counts[bad[0]])
    assert got_unique == int(np.count_nonzero(counts))


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("k", [9, 12])
def test_depth_edges(gpu_engine_cls, refs, batches4, k, mode):
    """depth 3; 2, 3 and 4 batches, then a sync: 1, 1 and 2 flushes, and every batch in one of them"""
    canon, n_mode, p_n = MODES[mode]
    D = 3
    with gpu_engine_cls(k, canonicalize=canon, n_mode=n_mode) as eng:
        eng.set_option("one_level_defer", D)
        for n, want_flushes in ((D - 1, 1), (D, 1), (D + 1, 2)):
            eng.reset()
            f0 = flush_counters(eng)
            for i, (b, o) in enumerate(batches4[p_n][:n]):
                eng.submit(b, o)
                assert eng.get_option("one_level_pending") == (i + 1) % D
            eng.sync()
            f1 = flush_counters(eng)
            assert (f1[0], f1[1] - f0[1], f1[2] - f0[2], f1[3] - f0[3]) == (0, want_flushes, n, 0), (n, f0, f1)
            check_vector(eng, refs.prefix(k, mode, batches4[p_n], n), "k=%d %s, %d batches" % (k, mode, n))
        assert eng.get_option("oom_fallbacks") == 0


def test_batches_of_different_sizes_in_one_flush(gpu_engine_cls, refs):
    """three batches in one flush: 70 000 reads, a single read, 3 000 reads no longer than 40 bases; their regions begin at different pages"""
    k, mode = 12, "canonical"
    bs = [ragged_batch(9201, 70_000), ragged_batch(9202, 1, lo=97, hi=97), ragged_batch(9203, 3_000, lo=12, hi=40)]
    with gpu_engine_cls(k, canonicalize=True, n_mode=DROP) as eng:
        eng.set_option("one_level_defer", 4)
        bases_seen = []
        for b, o in bs:
            bases_seen.append(eng.get_option("arena_region_base"))
            eng.submit(b, o)
        end = eng.get_option("arena_region_base")
        sizes = np.diff(bases_seen + [end])
        assert bases_seen[0] == 0 and len(set(bases_seen)) == 3 and (sizes > 0).all() and len(set(sizes.tolist())) == 3, (bases_seen, end)
        assert flush_counters(eng)[:2] == (3, 0)
        eng.sync()
        assert flush_counters(eng) == (0, 1, 3, 0) and eng.get_option("arena_region_base") == 0
        check_vector(eng, refs.want("sizes", k, mode, bs), "three sizes")


@pytest.mark.parametrize("read", ["finish", "table_stats"])
def test_reads_of_the_vector_between_submits(gpu_engine_cls, refs, batches4, read):
    k, mode = 12, "canonical"
    with gpu_engine_cls(k, canonicalize=True, n_mode=DROP) as eng:
        eng.set_option("one_level_defer", 8)
        b, o = batches4[0.0][0]
        eng.submit(b, o)
        assert flush_counters(eng)[:2] == (1, 0)
        counts, total = refs.prefix(k, mode, batches4[0.0], 1)
        if read == "finish":
            _, got_total, got_unique = eng.finish(copy=False)
        else:
            _, got_total, got_unique = eng.table_stats(copy=False)
        assert (got_total, got_unique) == (total, int(np.count_nonzero(counts)))
        assert flush_counters(eng) == (0, 1, 1, 0)
        eng.submit(*batches4[0.0][1])
        check_vector(eng, refs.prefix(k, mode, batches4[0.0], 2), "a read between two submits")


def test_reset_with_batches_pending(gpu_engine_cls, refs, batches4):
    k, mode = 12, "canonical"
    with gpu_engine_cls(k, canonicalize=True, n_mode=DROP) as eng:
        eng.set_option("one_level_defer", 4)
        eng.submit(*batches4[0.0][1])
        eng.submit(*batches4[0.0][2])
        assert flush_counters(eng)[:2] == (2, 0)
        eng.reset()
        assert flush_counters(eng) == (0, 0, 0, 0)
        eng.submit(*batches4[0.0][0])
        check_vector(eng, refs.prefix(k, mode, batches4[0.0], 1), "one batch behind a reset")
        assert flush_counters(eng) == (0, 1, 1, 0)


def test_adopted_vector_keeps_what_it_held(gpu_engine_cls, refs, batches4):
    import torch
    k, mode = 10, "forward"
    rng = np.random.Generator(np.random.PCG64(9300))
    before = rng.integers(1, 1 << 40, size=4 ** k, dtype=np.uint64)
    table = torch.zeros(4 ** k, dtype=torch.int64, device="cuda")
    bs = batches4[0.0][:3]
    counts, _ = refs.want((k, mode, "adopted"), k, mode, bs, base=before)
    with gpu_engine_cls(k, canonicalize=False, n_mode=DROP, table_ptr=table.data_ptr()) as eng:
        eng.set_option("one_level_defer", 2)
        table.copy_(torch.from_numpy(before.view(np.int64)))        # (an engine clears the vector it adopts: the caller writes it afterwards)
        torch.cuda.synchronize()
        for b, o in bs:
            eng.submit(b, o)
        eng.sync()
        assert flush_counters(eng) == (0, 2, 3, 0)
    torch.cuda.synchronize()
    assert np.array_equal(table.cpu().numpy().view(np.uint64), counts)


def test_arena_too_small(gpu_engine_cls, refs, batches4):
    """a budget of two and a half regions: the third batch does not fit and forces a flush; a budget of one and a half: the immediate path"""
    k, mode = 12, "canonical"
    bs = batches4[0.0]
    with gpu_engine_cls(k, canonicalize=True, n_mode=DROP) as eng:
        eng.set_option("one_level_defer", 8)
        eng.submit(*bs[0])
        region = eng.get_option("arena_region_base")
        eng.sync()
        assert region > 0 and eng.get_option("arena_pages") == 8 * region
    want = refs.prefix(k, mode, batches4[0.0], 4)
    with gpu_engine_cls(k, canonicalize=True, n_mode=DROP) as eng:
        eng.set_option("one_level_defer", 8)
        eng.set_option("pending_budget", region * BYTES_PER_PAGE * 5 // 2)
        seen = []
        for b, o in bs:
            eng.submit(b, o)
            seen.append(flush_counters(eng))
        assert seen == [(1, 0, 0, 0), (2, 0, 0, 0), (1, 1, 2, 1), (2, 1, 2, 1)], seen
        assert 2 * region <= eng.get_option("arena_pages") < 3 * region
        check_vector(eng, want, "a budget of 2.5 regions")
        assert flush_counters(eng) == (0, 2, 4, 1) and eng.get_option("oom_fallbacks") == 0
    with gpu_engine_cls(k, canonicalize=True, n_mode=DROP) as eng:
        eng.set_option("one_level_defer", 8)
        eng.set_option("pending_budget", region * BYTES_PER_PAGE * 3 // 2)
        for b, o in bs:
            eng.submit(b, o)
            assert flush_counters(eng) == (0, 0, 0, 0)
        check_vector(eng, want, "a budget of 1.5 regions")
        assert eng.get_option("arena_pages") == 0 and eng.get_option("oom_fallbacks") == 0


def period17_batch(seed, n_reads):
    unit = b"ACGTTGCAAGGCTCATC"
    assert len(unit) == 17
    rng = np.random.Generator(np.random.PCG64(seed))
    lens = rng.integers(35, 151, size=n_reads)
    starts = rng.integers(0, 17, size=n_reads)
    long_ = np.frombuffer(unit * 12, dtype=np.uint8)
    offsets = np.zeros(n_reads + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum(lens)
    # residue j of a read that starts at phase s is residue s + j of the repeat
    pos = np.arange(int(offsets[-1]), dtype=np.int64) - np.repeat(offsets[:-1].astype(np.int64), lens) + np.repeat(starts, lens)
    return long_[pos].copy(), offsets


def test_bucket_past_one_slice_across_pending_batches(gpu_engine_cls, refs, oracle):
    """17 ids, each too rare in a wave for the hot-id shortcut, fill a handful of buckets with far more than a slice's 128 pages: the pass
    runs several workgroups per bucket and they add to the vector with atomics -- over the pages of three pending batches"""
    k, mode = 12, "canonical"
    bs = [period17_batch(9400 + i, 60_000) for i in range(3)]
    fwd, total = None, 0
    for b, o in bs:
        fwd, t = oracle.c_count(b, o, k, False, DROP, counts=fwd)
        total += t
    ids = np.flatnonzero(fwd)
    assert ids.size == 17 and int(fwd.max()) * 64 < 16 * total       # 17 ids, none on 16 lanes of a wave's 64: not degenerate
    buckets = (ids >> 9) & 511                                        # the bucket field of the one-level path at k = 12
    per_bucket = np.bincount(buckets, weights=fwd[ids].astype(np.float64), minlength=512)
    assert per_bucket.max() > 4 * 128 * 512                           # several slices of 128 pages of 512 elements
    with gpu_engine_cls(k, canonicalize=True, n_mode=DROP) as eng:
        eng.set_option("one_level_defer", 4)
        for b, o in bs:
            eng.submit(b, o)
        assert flush_counters(eng)[:2] == (3, 0)
        check_vector(eng, refs.want("period17", k, mode, bs), "period-17 repeats")
        assert flush_counters(eng) == (0, 1, 3, 0)


def test_option_changes_with_batches_pending(gpu_engine_cls, refs, batches4):
    """one_level_defer 3 -> 0 -> 3 and the bucket field moved, each with batches pending: what is pending is added under the old value"""
    k, mode = 12, "canonical"
    bs = batches4[0.0]
    with gpu_engine_cls(k, canonicalize=True, n_mode=DROP) as eng:
        eng.set_option("one_level_defer", 3)
        eng.submit(*bs[0])
        assert flush_counters(eng)[:2] == (1, 0)
        eng.set_option("one_level_defer", 0)
        assert flush_counters(eng) == (0, 1, 1, 0)
        eng.submit(*bs[1])                                            # the immediate path
        assert flush_counters(eng) == (0, 1, 1, 0)
        eng.set_option("one_level_defer", 3)
        eng.submit(*bs[2])
        assert flush_counters(eng)[:2] == (1, 1)
        eng.set_option("sc_lo_bits", 15)                              # another bucket geometry under a pending batch
        assert flush_counters(eng) == (0, 2, 2, 0)
        eng.submit(*bs[3])
        assert flush_counters(eng)[:2] == (1, 2)
        check_vector(eng, refs.prefix(k, mode, batches4[0.0], 4), "option changes")
        assert flush_counters(eng) == (0, 3, 3, 0)


def test_k13_in_one_level(gpu_engine_cls, refs, batches4):
    k, mode = 13, "canonical"
    bs = batches4[0.0][:3]
    with gpu_engine_cls(k, canonicalize=True, n_mode=DROP) as eng:
        assert eng.get_option("one_level_max_k") == 13
        eng.set_option("one_level_defer", 2)
        eng.set_option("accum_bytes", 0)                              # (k >= 13 gathers host submits into batches of 1 GiB otherwise: one batch at the sync)
        for b, o in bs:
            eng.submit(b, o)
        assert flush_counters(eng) == (1, 1, 2, 0)
        check_vector(eng, refs.want("k13", k, mode, bs), "k = 13")


@pytest.mark.parametrize("depth,room", [(3, None), (4, 2)])
def test_bookkeeping_follows_the_model(gpu_engine_cls, oracle, depth, room):
    """a random sequence of submit, sync and reset: the engine's counters after every operation, and the vector at the end, are the model's"""
    k = 9
    ops = dm.fixed_ops(21, 40) + ["sync"]
    _, seen, holds = dm.run_model(ops, depth, room)
    small = [ragged_batch(9500 + i, 2_000, lo=90, hi=90) for i in range(sum(op == "submit" for op in ops))]      # (one size: every region is as large as the first)
    with gpu_engine_cls(k, canonicalize=False, n_mode=DROP) as eng:
        eng.set_option("one_level_defer", depth)
        if room is not None:
            with gpu_engine_cls(k, canonicalize=False, n_mode=DROP) as probe:
                probe.set_option("one_level_defer", depth)
                probe.submit(*small[0])
                region = probe.get_option("arena_region_base")
            eng.set_option("pending_budget", region * BYTES_PER_PAGE * (2 * room + 1) // 2)
        nb = 0
        for i, op in enumerate(ops):
            if op == "submit":
                eng.submit(*small[nb])
                nb += 1
            elif op == "sync":
                eng.sync()
            else:
                eng.reset()
            # (a reset clears the engine's counters of nothing: flushes are counted over the engine's life, like the model's)
            assert flush_counters(eng) == seen[i], (i, op, flush_counters(eng), seen[i])
        want, total = None, 0
        for j in holds[-1]:
            want, t = oracle.c_count(*small[j], k, False, DROP, counts=want)
            total += t
        if want is None:
            want = np.zeros(4 ** k, dtype=np.uint64)
        check_vector(eng, (want, total), "the batches since the last reset")


def test_defaults(gpu_engine_cls, refs, batches4):
    """as created: depth 4 at k = 12, the immediate path at k = 13"""
    k, mode = 12, "canonical"
    with gpu_engine_cls(k, canonicalize=True, n_mode=DROP) as eng:
        assert eng.get_option("one_level_defer") == -1
        seen = []
        for b, o in batches4[0.0]:
            eng.submit(b, o)
            seen.append(flush_counters(eng))
        assert seen == [(1, 0, 0, 0), (2, 0, 0, 0), (3, 0, 0, 0), (0, 1, 4, 0)], seen
        check_vector(eng, refs.prefix(k, mode, batches4[0.0], 4), "the default depth")
    with gpu_engine_cls(13, canonicalize=True, n_mode=DROP) as eng:
        eng.set_option("accum_bytes", 0)
        eng.submit(*batches4[0.0][0])
        assert flush_counters(eng) == (0, 0, 0, 0) and eng.get_option("arena_pages") == 0
        eng.sync()
