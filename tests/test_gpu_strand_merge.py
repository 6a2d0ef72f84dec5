"""GPU: the strands of a canonical profile merged once per sync (csrc/kdb_strands.hip.h).

First the kernel alone, through kdb_strand_merge, on vectors that counting never produces (64-bit values, a non-zero vector underneath):
both forms and their boundary (k = 8 direct, k = 9 blocked), odd and even k, even k - 6 (tiles that are their own partner), and k = 13
on a sparse vector checked by gather.  Then the engine, whose canonical batches of the one-level paths count forward ids into a staging
vector: against the oracle, with the option on and off, across syncs, option changes, resets, a caller's writes, folds and reduces.

Expected values of the kernel tests come from the definition, vectorised in numpy:
    table + where(id < rc, F + F[rc], where(id == rc, F, 0)),     rc = the k two-bit digits reversed, each complemented."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LET = np.frombuffer(b"ACGTN", dtype=np.uint8)
DROP, EXPAND = 0, 1


def rc_ids(ids, k):
    ids = np.asarray(ids, dtype=np.uint64)
    out = np.zeros_like(ids)
    x = ids.copy()
    for _ in range(k):
        out = (out << np.uint64(2)) | (np.uint64(3) - (x & np.uint64(3)))
        x >>= np.uint64(2)
    return out


def strand_merge(fwd, table, k):
    """kdb_strand_merge on two torch int64 CUDA tensors of 4^k elements."""
    import torch
    import kmerdb_amd
    lib = kmerdb_amd._abi.lib()
    torch.cuda.synchronize()
    rc = lib.kdb_strand_merge(0, fwd.data_ptr(), table.data_ptr(), k)
    assert rc == 0, kmerdb_amd._abi.last_error()


# --------------------------------------------------------------------------------------------------------------------------------
# the kernel alone
# --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 2, 3, 8, 9, 10, 11, 12])
def test_merge_kernel_equals_the_definition(gpu_engine_cls, k):
    import torch
    n = 4 ** k
    rng = np.random.Generator(np.random.PCG64(1000 + k))
    F = rng.integers(0, 1 << 40, size=n, dtype=np.uint64)
    F[rng.random(n) < 0.25] = 0                               # pairs with one strand or both at zero
    table = rng.integers(1, 1 << 40, size=n, dtype=np.uint64)
    ids = np.arange(n, dtype=np.uint64)
    rc = rc_ids(ids, k)
    want = table + np.where(ids < rc, F + F[rc], np.where(ids == rc, F, np.uint64(0)))
    if k % 2 == 0:
        assert np.count_nonzero(ids == rc) == 4 ** (k // 2)   # palindromes
    d_F = torch.from_numpy(F.view(np.int64)).cuda()
    d_t = torch.from_numpy(table.view(np.int64)).cuda()
    strand_merge(d_F, d_t, k)
    got = d_t.cpu().numpy().view(np.uint64)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, "k=%d: %d bins differ, first id %d: got %d, want %d" % (k, bad.size, bad[0], got[bad[0]], want[bad[0]])
    assert int(torch.count_nonzero(d_F).item()) == 0          # cleared in the same sweep
    strand_merge(d_F, d_t, k)                                 # nothing staged: nothing changes
    assert np.array_equal(d_t.cpu().numpy().view(np.uint64), want)
    assert int(torch.count_nonzero(d_F).item()) == 0


def test_merge_kernel_k13_sparse(gpu_engine_cls):
    import torch
    k = 13
    n = 4 ** k
    rng = np.random.Generator(np.random.PCG64(1013))
    a_stride = 4 ** (k - 3)
    m = 1234                                                  # a tile (the middle k - 6 digits) and its partner
    m_rc = int(rc_ids([m], k - 6)[0])
    assert m_rc != m
    corners = [a * a_stride + mm * 64 + b for mm in (m, m_rc) for a in (0, 63) for b in (0, 63)]
    nz = np.unique(np.concatenate([np.array([0, n - 1] + corners, dtype=np.uint64), rng.integers(0, n, size=4000, dtype=np.uint64)]))
    vals = rng.integers(1, 1 << 40, size=nz.size, dtype=np.uint64)
    d_F = torch.zeros(n, dtype=torch.int64, device="cuda")
    d_F[torch.from_numpy(nz.view(np.int64)).cuda()] = torch.from_numpy(vals.view(np.int64)).cuda()
    d_t = torch.randint(1, 1 << 40, (n,), dtype=torch.int64, device="cuda", generator=torch.Generator(device="cuda").manual_seed(13))
    before = d_t.clone()
    # every id that has a strand set, with its partner; the definition on those
    f_of = dict(zip(nz.tolist(), vals.tolist()))
    touched = np.unique(np.concatenate([nz, rc_ids(nz, k)]))
    rc_t = rc_ids(touched, k)
    add = np.array([(f_of.get(i, 0) + f_of.get(r, 0)) if i < r else (f_of.get(i, 0) if i == r else 0) for i, r in zip(touched.tolist(), rc_t.tolist())],
                   dtype=np.uint64)
    strand_merge(d_F, d_t, k)
    idx = torch.from_numpy(touched.view(np.int64)).cuda()
    got = (d_t[idx] - before[idx]).cpu().numpy().view(np.uint64)
    assert np.array_equal(got, add)
    assert int(torch.count_nonzero(d_t != before).item()) == int(np.count_nonzero(add))       # and no other bin moved
    assert int(torch.count_nonzero(d_F).item()) == 0
    after = d_t.clone()
    strand_merge(d_F, d_t, k)
    assert torch.equal(d_t, after)


# --------------------------------------------------------------------------------------------------------------------------------
# the engine
# --------------------------------------------------------------------------------------------------------------------------------
KS = [2, 7, 8, 9, 12, 13]
CASES = [(k, mode) for k in KS for mode in (DROP, EXPAND)]
N_READS = 3000
CUTS = (0, 1000, 2000, 3000)                                  # three batches


def ragged_reads(k, mode):
    """3 000 seeded reads of 35..150 bases with 0.5 % N; EXPAND at k = 3: one all-N read on top (its windows go to the work list)."""
    rng = np.random.Generator(np.random.PCG64(7000 + 10 * k + mode))
    lens = rng.integers(35, 151, size=N_READS)
    flat = LET[rng.integers(0, 4, size=int(lens.sum()))].copy()
    flat[rng.random(flat.size) < 0.005] = ord("N")
    ends = np.cumsum(lens)
    recs = [flat[int(e - n):int(e)].tobytes() for n, e in zip(lens, ends)]
    if (k, mode) == (3, EXPAND):
        recs[CUTS[1] + 5] = b"N" * 40
    return recs


class Inputs:
    """The reads of one (k, mode), their batches and the oracle's vectors (sparse: ids, counts, total), computed once and not changed."""

    def __init__(self, oracle):
        self.oracle = oracle
        self._reads, self._want = {}, {}

    def batch(self, k, mode, i):
        if (k, mode) not in self._reads:
            recs = ragged_reads(k, mode)
            self._reads[(k, mode)] = [self.oracle.pack_records(recs[CUTS[j]:CUTS[j + 1]]) for j in range(3)]
        return self._reads[(k, mode)][i]

    def want(self, k, mode, which=(0, 1, 2)):
        key = (k, mode, tuple(which))
        if key not in self._want:
            counts, total = None, 0
            for i in which:
                counts, t = self.oracle.c_count(*self.batch(k, mode, i), k, True, mode, counts=counts)
                total += t
            ids = np.flatnonzero(counts)
            self._want[key] = (ids, counts[ids].copy(), total)
        return self._want[key]


@pytest.fixture(scope="module")
def inputs(oracle):
    return Inputs(oracle)


def check(got, total, unique, want, what=""):
    ids, vals, w_total = want
    assert (total, unique) == (w_total, ids.size), (what, total, unique, w_total, ids.size)
    if got is not None:
        assert np.count_nonzero(got) == ids.size and np.array_equal(got[ids], vals), what


def engine(cls, k, mode, **opts):
    eng = cls(k, canonicalize=True, n_mode=mode, device=0, table_ptr=opts.pop("table_ptr", None))
    if k == 13:
        eng.set_option("strand_merge_max_k", 13)              # (the default stops at 12: k = 13 is staged on request)
    for name, v in opts.items():
        eng.set_option(name, v)
    return eng


def stages(eng):
    """Does this engine's next canonical batch count forward ids?  (the defaults, unless the suite runs under KDB_ENGINE_OPTS)"""
    return bool(eng.get_option("strand_merge")) and eng.k <= min(eng.get_option("strand_merge_max_k"), eng.get_option("one_level_max_k")) \
        and eng.get_option("algo") in (0, 2, 3) and not eng.get_option("overlap") and not eng.get_option("smallk_old")


@pytest.mark.parametrize("k,mode", CASES + [(3, EXPAND)])
def test_option_on_and_off_give_the_oracles_vector(gpu_engine_cls, inputs, k, mode):
    want = inputs.want(k, mode)
    out = {}
    for on in (1, 0):
        with engine(gpu_engine_cls, k, mode, strand_merge=on) as eng:
            eng.prof_enable(True)
            for i in range(3):
                eng.submit(*inputs.batch(k, mode, i))
            out[on] = eng.finish()
            merges = eng.prof()["strand_merge_kernel"][1]
            assert merges == (1 if on and stages(eng) else 0), (on, merges)          # once per sync, and only with something staged
        check(*out[on], want, "strand_merge=%d" % on)
    assert np.array_equal(out[1][0], out[0][0]) and out[1][1:] == out[0][1:]


@pytest.mark.parametrize("k,mode", CASES)
def test_merge_is_repeatable_across_syncs(gpu_engine_cls, inputs, k, mode):
    with engine(gpu_engine_cls, k, mode) as eng:
        eng.prof_enable(True)
        eng.submit(*inputs.batch(k, mode, 0))
        eng.sync()
        eng.sync()                                            # nothing pending: launches nothing
        if stages(eng):
            assert eng.prof()["strand_merge_kernel"][1] == 1
        check(*eng.table_stats(), inputs.want(k, mode, (0,)), "after the first sync")
        eng.submit(*inputs.batch(k, mode, 1))
        eng.submit(*inputs.batch(k, mode, 2))
        check(*eng.finish(), inputs.want(k, mode), "submit, sync, submit, submit, finish")


@pytest.mark.parametrize("k,mode", CASES)
def test_option_switched_between_batches(gpu_engine_cls, inputs, k, mode):
    with engine(gpu_engine_cls, k, mode) as eng:
        eng.submit(*inputs.batch(k, mode, 0))
        eng.set_option("strand_merge", 0)
        eng.submit(*inputs.batch(k, mode, 1))
        eng.set_option("strand_merge", 1)
        eng.submit(*inputs.batch(k, mode, 2))
        check(*eng.finish(), inputs.want(k, mode), "on, off, on")


@pytest.mark.parametrize("k,mode", CASES)
def test_reset_leaves_nothing_staged(gpu_engine_cls, inputs, k, mode):
    with engine(gpu_engine_cls, k, mode) as eng:
        eng.submit(*inputs.batch(k, mode, 0))
        eng.submit(*inputs.batch(k, mode, 2))
        eng.reset()                                           # two batches staged, never merged
        eng.submit(*inputs.batch(k, mode, 1))
        check(*eng.finish(), inputs.want(k, mode, (1,)), "a job after reset without sync")
        eng.reset()
        assert eng.finish(copy=False)[1:] == (0, 0)
        eng.submit(*inputs.batch(k, mode, 1))
        check(*eng.finish(), inputs.want(k, mode, (1,)), "a job after reset")


def test_adopted_vector_keeps_what_the_caller_wrote(gpu_engine_cls, inputs):
    """The one-level form of test_gpu_lifecycle.py::test_counts_somebody_else_wrote_survive: the caller's vector is only ever added to,
    at canonical bins; what the caller wrote anywhere else, non-canonical bins included, is there after a batch, a sync, and -- written
    after a reset -- after the job that follows."""
    import torch
    k, mode = 12, DROP
    n = 4 ** k
    mine = torch.zeros(n, dtype=torch.int64, device="cuda")
    ids0, vals0, _ = inputs.want(k, mode, (0,))
    ids = np.arange(n, dtype=np.uint64)
    noncanon = np.flatnonzero(ids > rc_ids(ids, k))
    written = np.unique(np.concatenate([ids0[:4], ids0[-2:], noncanon[[0, 1, 77777, -1]], np.setdiff1d(np.arange(100, 200), ids0)[:2]])).astype(np.int64)
    assert written.size >= 12 - 1 and np.intersect1d(written, noncanon).size >= 4

    def dense(which, extra):
        w_ids, w_vals, total = inputs.want(k, mode, which)
        v = np.zeros(n, dtype=np.uint64)
        v[w_ids] = w_vals
        for where, c in extra:
            v[where] += np.uint64(c)
        return v, total + sum(c * len(where) for where, c in extra)

    with engine(gpu_engine_cls, k, mode, table_ptr=mine.data_ptr()) as eng:
        eng.submit(*inputs.batch(k, mode, 0))
        eng.sync()
        mine[torch.as_tensor(written, device="cuda")] += 5
        torch.cuda.synchronize()
        eng.submit(*inputs.batch(k, mode, 1))                 # staged: the caller's vector is not touched before the sync
        eng.submit(*inputs.batch(k, mode, 2))
        got, s, _ = eng.table_stats()
        v, total = dense((0, 1, 2), [(written, 5)])
        assert s == total and np.array_equal(got, v)
        assert np.array_equal(mine.cpu().numpy().view(np.uint64), v)
        eng.reset()
        one = np.array([int(noncanon[12345])], dtype=np.int64)
        mine[torch.as_tensor(one, device="cuda")] += 3
        torch.cuda.synchronize()
        eng.submit(*inputs.batch(k, mode, 1))
        got, s, _ = eng.table_stats()
        v, total = dense((1,), [(one, 3)])
        assert s == total and np.array_equal(got, v)


@pytest.mark.parametrize("k,mode", [(8, DROP), (9, EXPAND), (12, DROP)])
def test_samplesheet_fold_and_reduce(gpu_engine_cls, inputs, k, mode):
    import kmerdb_amd
    with engine(gpu_engine_cls, k, mode) as eng:              # two files: batch 0, then batches 1 and 2
        eng.submit(*inputs.batch(k, mode, 0))
        w = inputs.want(k, mode, (0,))
        assert tuple(eng.fold_file()) == (w[2], w[0].size)
        eng.submit(*inputs.batch(k, mode, 1))
        eng.submit(*inputs.batch(k, mode, 2))
        w = inputs.want(k, mode, (1, 2))
        assert tuple(eng.fold_file()) == (w[2], w[0].size)
        check(*eng.finish_folded(), inputs.want(k, mode), "finish_folded")
    with engine(gpu_engine_cls, k, mode) as a, engine(gpu_engine_cls, k, mode) as b:
        a.submit(*inputs.batch(k, mode, 0))
        b.submit(*inputs.batch(k, mode, 1))
        b.submit(*inputs.batch(k, mode, 2))
        kmerdb_amd.engine.reduce_engines([a, b], root=0)      # both engines' strands are still staged when it is called
        check(*a.finish(), inputs.want(k, mode), "reduce_engines")


@pytest.mark.parametrize("option,k,mode", [("overlap", 9, DROP), ("overlap", 12, DROP), ("overlap", 12, EXPAND), ("smallk_old", 7, DROP),
                                           ("smallk_old", 8, DROP), ("smallk_old", 8, EXPAND)])
def test_paths_that_are_not_staged_still_count(gpu_engine_cls, inputs, option, k, mode):
    with engine(gpu_engine_cls, k, mode, **{option: 1}) as eng:
        eng.prof_enable(True)
        for i in range(3):
            eng.submit(*inputs.batch(k, mode, i))
        check(*eng.finish(), inputs.want(k, mode), option)
        assert eng.prof()["strand_merge_kernel"][1] == 0      # canonical in the counting kernels


def test_strand_merge_max_k_14_at_k14(gpu_engine_cls, inputs):
    """strand_merge_max_k above one_level_max_k: the two-level paths are never staged, the vector is the default's."""
    import torch
    k, mode = 14, DROP
    recs = ragged_reads(k, mode)
    bases, offsets = inputs.oracle.pack_records(recs)
    vecs = []
    for opts in ({}, {"strand_merge_max_k": 14}):
        with engine(gpu_engine_cls, k, mode, **opts) as eng:
            eng.submit(bases, offsets)
            stats = eng.finish(copy=False)[1:]
            vecs.append((eng.table_tensor().clone(), stats))
    assert vecs[0][1] == vecs[1][1] and vecs[0][1][0] > 0 and torch.equal(vecs[0][0], vecs[1][0])


def test_no_room_for_the_staging_vector(gpu_engine_cls, inputs):
    """The device is full when the first batch comes: no staging vector, the batch is counted canonically into the vector (through the
    scatter path or, where its scratch does not fit either, by direct atomics).  With memory back the next batch is staged; both kinds
    in one job give the oracle's vector.  (The device is filled as in test_gpu_parity.py's out-of-memory test.)"""
    import torch
    k, mode = 12, DROP
    with engine(gpu_engine_cls, k, mode) as eng:
        staged = stages(eng)
        eng.prof_enable(True)
        bases, offsets = inputs.batch(k, mode, 0)             # in HBM before the device is filled: no host staging to allocate
        d_b = torch.from_numpy(bases).cuda()
        d_o = torch.from_numpy(offsets.view(np.int64).copy()).cuda()
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        free, _ = torch.cuda.mem_get_info()
        hog = [torch.empty(free - (1 << 30), dtype=torch.uint8, device="cuda")]
        for size in (256 << 20, 16 << 20, 1 << 20):
            while True:
                try:
                    hog.append(torch.empty(size, dtype=torch.uint8, device="cuda"))
                except torch.OutOfMemoryError:
                    break
        given_back = 0
        while given_back < (32 << 20):                        # room for the engine's small per-batch arrays, not for 128 MiB
            i = next((j for j in range(len(hog) - 1, -1, -1) if hog[j].numel() <= (16 << 20)), None)
            if i is None:
                break
            given_back += hog.pop(i).numel()
        torch.cuda.empty_cache()
        try:
            eng.submit_device(d_b.data_ptr(), bases.size, d_o.data_ptr(), len(offsets) - 1)
            eng.sync()
            assert eng.prof()["strand_merge_kernel"][1] == 0, "the staging vector was allocated on a full device"
        finally:
            del hog
            torch.cuda.empty_cache()
        check(*eng.table_stats(), inputs.want(k, mode, (0,)), "counted without the staging vector")
        eng.submit(*inputs.batch(k, mode, 1))
        eng.submit(*inputs.batch(k, mode, 2))
        check(*eng.finish(), inputs.want(k, mode), "one batch unstaged, two staged")
        assert eng.prof()["strand_merge_kernel"][1] == (1 if staged else 0)
