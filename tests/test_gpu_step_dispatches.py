"""GPU: the small dispatches around the one-level count step's two kernels.

The per-batch words of the device counters, which lens_kernel (csrc/kdb_kernels.hip.h) fills with a batch's record geometry, are put back to zero by
the batch's last kernel (resolve_suspects_kernel's last-arriving workgroup) instead of by a memset in front of every batch, and the page sort
(csrc/kdb_scatter.hip.h: pages_count / pages_scan / pages_place) leaves the tags and the bucket counts as the next sort wants to find them, so that
the memsets in front of it run only for what is not known to be clean (csrc/kdb_scatter_host.hip.h: ScatterState::tags_dirty, bkt_zero_nb).  What would show a leftover: a length or a count of the batch before
in this batch's geometry, a tag of an earlier cycle counted again (the engine's own Sum(counts) == windows emitted check fails at the read).

Every vector is compared with the oracle's over all 4^k bins; finish() applies the engine's Sum check at every read.  Oracle vectors are
computed once per input and not changed."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LET = np.frombuffer(b"ACGT", dtype=np.uint8)
DROP, EXPAND = 0, 1


def batch_of(lens, seed, letters=LET, p_n=0.0):
    rng = np.random.Generator(np.random.PCG64(seed))
    lens = np.asarray(lens, dtype=np.int64)
    bases = letters[rng.integers(0, len(letters), size=int(lens.sum()))].copy()
    if p_n:
        bases[rng.random(bases.size) < p_n] = ord("N")
    offsets = np.zeros(len(lens) + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum(lens)
    return bases, offsets


def uniform(n, L, seed, **kw):
    return batch_of(np.full(n, L), seed, **kw)


def ragged(n, lo, hi, seed, **kw):
    rng = np.random.Generator(np.random.PCG64(seed + 77))
    return batch_of(rng.integers(lo, hi + 1, size=n), seed, **kw)


def edge_lens(n, k):
    """reads of k .. k + 2 bases whose shortest and longest sit where a lost partial result would hide them: all k + 1 but the last
    (k + 2) and the middle one (k) -- a batch that looks uniform to a kernel that misses either"""
    lens = np.full(n, k + 1)
    lens[-1] = k + 2
    if n >= 3:
        lens[n // 2] = k
    return lens


class Device:
    """device-resident copies; the offsets at an address that is 8 but not 16 bytes aligned where asked"""

    def __init__(self):
        import torch
        self.torch, self.keep = torch, []

    def submit(self, eng, bases, offsets, odd=True, nbytes=None):
        t = self.torch
        d_b = t.from_numpy(bases.copy()).cuda()
        o = offsets.view(np.int64)
        d_all = t.from_numpy(np.concatenate([np.zeros(1, np.int64), o]) if odd else o.copy()).cuda()
        d_o = d_all[1:] if odd else d_all
        assert d_o.data_ptr() % 16 == (8 if odd else 0)
        self.keep.append((d_b, d_all))                     # (asynchronous: the buffers live until the read)
        eng.submit_device(d_b.data_ptr(), bases.size if nbytes is None else nbytes, d_o.data_ptr(), len(offsets) - 1)


class Want:
    """the oracle's running vector over the batches submitted so far"""

    def __init__(self, oracle, k, canon, n_mode=DROP):
        self.oracle, self.k, self.canon, self.n_mode, self.counts, self.total = oracle, k, canon, n_mode, None, 0

    def add(self, bases, offsets, times=1):
        one, t = self.oracle.c_count(bases, offsets, self.k, self.canon, self.n_mode)
        one *= np.uint64(times)
        self.counts = one if self.counts is None else self.counts + one
        self.total += t * times

    def check(self, eng, what):
        got, got_total, got_unique = eng.finish()
        assert got_total == self.total, (what, got_total, self.total)
        bad = np.flatnonzero(got != self.counts)
        assert bad.size == 0, "%s: %d bins differ, first id %d: got %d, want %d" % (what, bad.size, bad[0], got[bad[0]], self.counts[bad[0]])
        assert got_unique == int(np.count_nonzero(self.counts)), what


# ---------------------------------------------------------------------------------------------------------------------------------
# record geometry
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [9, 12])
def test_geometry_does_not_leak_from_batch_to_batch(gpu_engine_cls, oracle, k):
    """uniform L = 40, ragged, uniform L = 25, a batch with one read shorter than k (the error comes at its sync, not before), reset, uniform again --
    one engine, nothing clears the per-batch words between the batches but the batch's own last kernel"""
    want = Want(oracle, k, True)
    with gpu_engine_cls(k, canonicalize=True, n_mode=DROP) as eng:
        for what, (b, o) in (("uniform 40", uniform(3000, 40, 1)), ("ragged", ragged(2500, 20, 90, 2)), ("uniform 25", uniform(3000, 25, 3))):
            eng.submit(b, o)
            want.add(b, o)
            want.check(eng, what)
        lens = np.full(2000, 30)
        lens[1234] = k - 1
        b, o = batch_of(lens, 4)
        eng.submit(b, o)                                   # (no error yet)
        with pytest.raises(ValueError, match="shorter than k"):
            eng.sync()
        eng.reset()
        b, o = uniform(3000, 31, 5)
        want = Want(oracle, k, True)
        for i in range(5):                                 # (past one flush cycle of the default depth: the last kernel's ticket is back at zero every time)
            eng.submit(b, o)
        want.add(b, o, times=5)
        want.check(eng, "uniform 31 after the reset")


def test_geometry_read_counts(gpu_engine_cls, oracle):
    """1, 2 and the counts at the edges of a wave, of a workgroup of 256 lanes and of two and four of them, host-fed and device-resident with the
    offsets at an address that is 8 but not 16 bytes aligned; every batch's shortest and longest read hide in the middle and at the end"""
    k = 9
    want, dev = Want(oracle, k, False), Device()
    with gpu_engine_cls(k, canonicalize=False, n_mode=DROP) as eng:
        for n in (1, 2, 3, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1023, 1025):
            b, o = batch_of(edge_lens(n, k), 100 + n)
            eng.submit(b, o)
            dev.submit(eng, b, o, odd=True)
            dev.submit(eng, b, o, odd=False)
            want.add(b, o, times=3)
            want.check(eng, "%d reads" % n)


@pytest.mark.parametrize("odd", [False, True])
def test_geometry_past_one_grid_stride(gpu_engine_cls, oracle, odd):
    """1 048 579 reads of k .. k + 2 bases (a batch under 16 MB): the full grid of 1024 workgroups of 256 lanes -- four whole strides of the
    four-fold unrolled loop and three records of a second iteration"""
    k, n = 9, 1_048_579
    want, dev = Want(oracle, k, False), Device()
    b, o = batch_of(edge_lens(n, k), 7)
    with gpu_engine_cls(k, canonicalize=False, n_mode=DROP) as eng:
        dev.submit(eng, b, o, odd=odd)
        want.add(b, o)
        want.check(eng, "1 048 579 reads")
        # all of one length but the very last: a uniform batch to every workgroup but one
        lens = np.full(n, k + 1)
        lens[-1] = k
        b, o = batch_of(lens, 8)
        dev.submit(eng, b, o, odd=odd)
        want.add(b, o)
        want.check(eng, "1 048 579 reads, the last one shorter")


@pytest.mark.parametrize("k", [9, 12])
def test_ragged_record_starts(gpu_engine_cls, oracle, k):
    """first_rec: records that straddle 4 KiB boundaries, records longer than 8 KiB that own several blocks, blocks that hold dozens of records"""
    want, dev = Want(oracle, k, True), Device()
    rng = np.random.Generator(np.random.PCG64(11))
    cases = (("straddling", rng.integers(100, 201, size=900)),
             ("long records", np.array([50, 9000, 20000, 60, 4096, 8192, 12289, 33, 4095, 4097, 70000, 40])),
             ("dozens per block", rng.integers(k, k + 4, size=6000)),
             ("mixed", np.concatenate([rng.integers(k, k + 3, size=700), [30000], rng.integers(100, 201, size=100), [8193], rng.integers(k, 60, size=500)])))
    with gpu_engine_cls(k, canonicalize=True, n_mode=DROP) as eng:
        for i, (what, lens) in enumerate(cases):
            b, o = batch_of(lens, 20 + i)
            eng.submit(b, o)
            dev.submit(eng, b, o, odd=True)
            want.add(b, o, times=2)
            want.check(eng, what)


def test_offsets_that_do_not_tile_the_buffer(gpu_engine_cls, oracle):
    """device-resident offsets that do not start at 0, do not end at nbytes, or decrease: the job fails at the sync, nothing is counted, and after a
    reset the engine counts as if nothing had happened"""
    k = 12
    b, o = uniform(4000, 50, 31)
    good = Want(oracle, k, False)
    good.add(b, o)
    dev = Device()
    table = dev.torch.zeros(4 ** k, dtype=dev.torch.int64, device="cuda")      # (a vector of the caller's: it can be read when the engine refuses to)
    with gpu_engine_cls(k, canonicalize=False, n_mode=DROP, table_ptr=table.data_ptr()) as eng:
        for what, at, delta in (("start", 0, 1), ("end", -1, -1), ("end past", -1, 1)):
            bad = o.copy()
            bad[at] = np.uint64(int(bad[at]) + delta)
            for odd in (False, True):
                dev.submit(eng, b, bad, odd=odd, nbytes=b.size)
                with pytest.raises(ValueError, match="read_offsets must rise"):
                    eng.sync()
                assert int(table.sum().item()) == 0, what
                eng.reset()
        bad = o.copy()
        bad[[700, 701]] = bad[[701, 700]]                  # record 700 ends before it starts
        dev.submit(eng, b, bad, odd=True)
        with pytest.raises(ValueError, match="read_offsets must rise"):
            eng.sync()
        assert int(table.sum().item()) == 0
        eng.reset()
        dev.submit(eng, b, o, odd=True)
        good.check(eng, "clean batch after the refused ones")


# ---------------------------------------------------------------------------------------------------------------------------------
# tags and sort
# ---------------------------------------------------------------------------------------------------------------------------------
PATHS = [(12, 2), (12, 4), (9, 2), (9, 4), (13, 0)]        # (k, one_level_defer); k = 13: the immediate path


def path_engine(cls, k, defer, canon=True, n_mode=DROP):
    eng = cls(k, canonicalize=canon, n_mode=n_mode)
    eng.set_option("accum_bytes", 0)                       # (k = 13: every host submit is a batch of its own)
    eng.set_option("one_level_defer", defer)
    return eng


@pytest.fixture(scope="module")
def shapes():
    """batches shared by the tests below (inputs only: every test keeps its own running oracle vector)"""
    return {"large": [ragged(30_000, 35, 150, 40 + i) for i in range(2)],
            "small": [ragged(40, 35, 150, 50 + i) for i in range(2)],
            "ac": ragged(20_000, 35, 150, 60, letters=np.frombuffer(b"AC", dtype=np.uint8)),
            "polya": batch_of(np.full(3000, 150), 61, letters=np.frombuffer(b"A", dtype=np.uint8)),
            "with_n": ragged(20_000, 35, 150, 62, p_n=0.005)}


@pytest.mark.parametrize("k,defer", PATHS)
def test_three_cycles_large_small_large(gpu_engine_cls, oracle, shapes, k, defer):
    """three flush cycles on one engine without a reset: a tag of the first cycle left standing beyond the small cycle's regions would be counted
    again in the third"""
    want = Want(oracle, k, True)
    per_cycle = max(defer, 1)
    with path_engine(gpu_engine_cls, k, defer) as eng:
        f0 = eng.get_option("hist_flushes")
        for cycle, size in enumerate(("large", "small", "large")):
            for i in range(per_cycle):
                b, o = shapes[size][i % 2]
                eng.submit(b, o)
                want.add(b, o)
            if k <= 12:
                assert eng.get_option("one_level_pending") == 0 and eng.get_option("hist_flushes") - f0 >= cycle + 1
                want.check(eng, "cycle %d (%s)" % (cycle, size))
            else:
                assert eng.finish(copy=False)[0:2] == (None, want.total)          # (the engine's Sum check, without the copy of 4^13 bins)
        want.check(eng, "after the third cycle")


@pytest.mark.parametrize("k,defer", PATHS)
def test_reset_between_scatter_and_flush(gpu_engine_cls, oracle, shapes, k, defer):
    """a reset drops a scattered batch whose tags no sort has read: the next cycle clears them (the dirty-tags path), and the cycle after that
    finds them clean again"""
    with path_engine(gpu_engine_cls, k, defer) as eng:
        b, o = shapes["large"][0]
        eng.submit(b, o)
        if defer:
            assert eng.get_option("one_level_pending") == 1
        eng.reset()
        want = Want(oracle, k, True)
        for cycle in range(2):
            for i in range(max(defer, 1)):
                b, o = shapes["small" if cycle == 0 else "large"][i % 2]
                eng.submit(b, o)
                want.add(b, o)
        want.check(eng, "two cycles after the reset")


@pytest.mark.parametrize("k,defer", PATHS)
def test_sparse_and_hot_inputs(gpu_engine_cls, oracle, shapes, k, defer):
    """reads over {A, C} only (most buckets stay empty), then a poly-A batch (hot ids, almost no pages), then ordinary reads, on one engine"""
    want = Want(oracle, k, True)
    with path_engine(gpu_engine_cls, k, defer) as eng:
        for what in ("ac", "polya", "ac"):
            b, o = shapes[what]
            eng.submit(b, o)
            want.add(b, o)
        if k <= 12:
            want.check(eng, "AC, poly-A, AC")
        b, o = shapes["large"][1]
        eng.submit(b, o)
        want.add(b, o)
        want.check(eng, "and ordinary reads")


@pytest.mark.parametrize("k,defer", PATHS)
def test_n_expansion(gpu_engine_cls, oracle, shapes, k, defer):
    want = Want(oracle, k, True, EXPAND)
    with path_engine(gpu_engine_cls, k, defer, n_mode=EXPAND) as eng:
        for b, o in (shapes["with_n"], shapes["small"][0], shapes["with_n"]):
            eng.submit(b, o)
            want.add(b, o)
        want.check(eng, "N expansion")


def test_nine_regions_past_one_grid_stride_of_the_sort(gpu_engine_cls, oracle):
    """one_level_defer = 9 with batches of just over 256 tiles (the smallest whose region holds the page sequences of all 256 scatter workgroups,
    256 x 577 pages): nine regions are 1.33 M tags -- past the 256 workgroups x 4096 tags of one grid stride of the sort, most of them unused;
    two cycles, the second over what the first left behind"""
    k = 12
    want = Want(oracle, k, True)
    b, o = uniform(29_000, 150, 70)
    with path_engine(gpu_engine_cls, k, 9) as eng:
        for cycle in range(2):
            for i in range(9):
                eng.submit(b, o)
            want.add(b, o, times=9)
            assert eng.get_option("one_level_pending") == 0 and eng.get_option("arena_pages") > 256 * 4096
            want.check(eng, "cycle %d of nine regions" % cycle)


def test_same_reads_through_the_other_paths(gpu_engine_cls, oracle, shapes):
    """the immediate one-level path, the direct-atomics kernel and a k = 14 engine (two-level path on the shared sort, three flushes) give the oracle's vectors"""
    batches = [shapes["large"][0], shapes["ac"], shapes["small"][0]]
    for k, opts in ((12, {"one_level_defer": 0}), (12, {"algo": 1})):
        want = Want(oracle, k, True)
        with gpu_engine_cls(k, canonicalize=True, n_mode=DROP) as eng:
            for name, v in opts.items():
                eng.set_option(name, v)
            for b, o in batches:
                eng.submit(b, o)
                want.add(b, o)
            want.check(eng, "k=%d %r" % (k, opts))
    k = 14
    want = Want(oracle, k, True)
    with gpu_engine_cls(k, canonicalize=True, n_mode=DROP) as eng:
        eng.set_option("accum_bytes", 0)
        for cycle, (b, o) in enumerate((ragged(4000, 35, 150, 80), ragged(30, 35, 150, 81), ragged(4000, 35, 150, 82))):
            eng.submit(b, o)
            want.add(b, o)
            assert eng.finish(copy=False)[0:2] == (None, want.total)              # (a flush per read: large, small, large)
        want.check(eng, "k=14")
