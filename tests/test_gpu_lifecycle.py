"""The engine's state that outlives a batch, against tests/lifecycle_model.py: which form the deferred histogram pass takes (store over
a vector that is known to be zero, or add), what a fold, a reset, a caller's write, an option change or an error leaves behind, the
flush after 64 pending batches, continuation pieces through every submit path -- scripted cases first, then the fixed seeds of
tests/test_lifecycle_model_cpu.py through the same driver that the stand-in engine passed there.

k = 13 runs with one_level_max_k = 12 (the two-level path over a 512 MiB vector) and k = 14 as it is.  An engine-owned vector is read
through finish() / table_stats() host copies: table_tensor() calls kdb_table, which ends the store form for the engine's life."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lifecycle_model as lm  # noqa: E402

pytestmark = pytest.mark.gpu

LO_BITS = 12                                      # SC_LO_BITS_TWO_LEVEL: id bits below the bucket field
BUCKET_STORE_BYTES = 8 * 32768                    # the store form writes every bin of a touched bucket once (k <= 16: 32768 bins of 8 bytes)


def reads(n, seed, lo=100, hi=150):
    rng = np.random.Generator(np.random.PCG64(seed))
    lens = rng.integers(lo, hi + 1, size=n)
    flat = lm.LET[rng.integers(0, 4, size=int(lens.sum()))]
    ends = np.cumsum(lens)
    return [flat[int(e - l):int(e)].tobytes() for l, e in zip(lens, ends)]


def two_level(engine_cls, k, canon=True, n_mode=0, **opts):
    eng = engine_cls(k, canonicalize=canon, n_mode=n_mode, algo=2)
    if k == 13:
        eng.set_option("one_level_max_k", 12)
    eng.set_option("accum_bytes", opts.pop("accum_bytes", 0))       # one device batch per submit
    for name, v in opts.items():
        eng.set_option(name, v)
    return eng


def ids_of(oracle, records, k, canon=True):
    return np.concatenate([oracle.c_shred(r, k, canon, oracle.N_DROP)[0] for r in records])


def buckets(ids, k):
    """The level-2 buckets that hold `ids`: id = [ hi ][ bucket: 2k - 15 bits ][ lo: 12 ]."""
    return np.unique((ids >> np.uint64(LO_BITS)) & np.uint64((1 << (2 * k - 15)) - 1))


def submit(eng, model, records):
    eng.submit(*lm.pack(records))
    model.submit(records)


def same_as_model(eng, model, how="finish", copy=True):
    vec, total, unique = getattr(model, how)()
    got, g_total, g_unique = getattr(eng, how)(copy=copy)
    print(how, "engine", (g_total, g_unique), "model", (total, unique))
    assert (g_total, g_unique) == (total, unique)
    if copy:
        assert lm.compare_vector(got, vec, model.nbins, g_total)


def error_counts(eng):
    a, b = ctypes.c_uint64(0), ctypes.c_uint64(0)
    assert eng._lib.kdb_error_counts(eng._h, ctypes.byref(a), ctypes.byref(b)) == 0
    return a.value, b.value


@pytest.fixture(scope="module")
def batches(oracle):
    """Three batches of 200..2000 reads of 100..150 bases, and their ids per k (computed once, never changed).  C is 200 reads of one
    2 kb sequence: it leaves a good part of the buckets alone, so a flush that stores over what a fold should have cleared shows."""
    rng = np.random.Generator(np.random.PCG64(13))
    genome = lm.LET[rng.integers(0, 4, size=2000)].tobytes()
    starts, lens = rng.integers(0, 2000 - 150, size=200), rng.integers(100, 151, size=200)
    recs = {"A": reads(300, 11), "B": reads(2000, 12), "C": [genome[int(s):int(s + n)] for s, n in zip(starts, lens)]}
    ids = {(name, k): ids_of(oracle, r, k) for name, r in recs.items() for k in (13, 14)}
    return recs, ids


# --------------------------------------------------------------------------------------------------------------------------------
# 1. store, then add, then fold, then store again -- and which form ran, from the bytes of the vector the pass says it moved
# --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [13, 14])
def test_store_then_add_then_fold_then_store_again(gpu_engine_cls, oracle, batches, k):
    """hist_flush_runs (kdb_scatter.hip.h) by its own account, for buckets whose pages fit one slice (every bucket of these batches: a
    bucket gets at most a page per level-2 workgroup that holds its leading digit, fewer than the 128 pages of the smallest slice):
      store form: every thread writes NH * PAIRS / P2_THREADS pairs of 16 bytes = 8 bytes for each of the bucket's 32768 bins, written
                  once and not read: 8 * 32768 bytes per touched bucket, whatever the bucket holds;
      add form:   a pair of adjacent bins (ids 2p, 2p + 1: the bucket field sits above bit 0) is read and written back, 16 + 16 bytes,
                  where either is nonzero: 32 bytes per distinct id >> 1 of the batches in the flush.
    The store form must run on the first flush after create, reset and fold_file, the add form on every other one."""
    recs, ids = batches
    model = lm.ModelEngine(k, True, 0, oracle)
    with two_level(gpu_engine_cls, k) as eng:
        def flush_bytes(name):
            assert eng.get_option("pending_batches") == 1
            before = eng.get_option("table_bytes")
            eng.sync()
            moved = eng.get_option("table_bytes") - before
            store = BUCKET_STORE_BYTES * len(buckets(ids[(name, k)], k))
            add = 32 * len(np.unique(ids[(name, k)] >> np.uint64(1)))
            print("k=%d batch %s: the pass moved %d bytes; store form %d, add form %d" % (k, name, moved, store, add))
            assert store != add
            return moved, store, add

        submit(eng, model, recs["A"])
        moved, store, add = flush_bytes("A")
        assert moved == store                                 # after create
        same_as_model(eng, model)
        submit(eng, model, recs["B"])
        moved, store, add = flush_bytes("B")
        assert moved == add                                   # the vector holds A
        same_as_model(eng, model)
        assert tuple(eng.fold_file()) == tuple(model.fold())
        submit(eng, model, recs["C"])
        moved, store, add = flush_bytes("C")
        assert moved == store                                 # after fold_file
        same_as_model(eng, model)                             # C alone
        assert tuple(eng.fold_file()) == tuple(model.fold())
        same_as_model(eng, model, "finish_folded")            # A + B + C
        eng.reset()
        model.reset()
        same_as_model(eng, model, "finish_folded", copy=k == 13)      # all zero, total 0
        assert eng.finish_folded(copy=False)[1:] == (0, 0)
        submit(eng, model, recs["A"])
        moved, store, add = flush_bytes("A")
        assert moved == store                                 # after reset
        same_as_model(eng, model)


# --------------------------------------------------------------------------------------------------------------------------------
# 2. somebody else wrote the vector
# --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("owner", ["engine", "caller"])
@pytest.mark.parametrize("k", [13, 14])
def test_counts_somebody_else_wrote_survive(gpu_engine_cls, oracle, batches, k, owner):
    """Once kdb_table has handed the vector out (or the vector is the caller's to begin with), no flush may take it for zero: not the
    one that follows the write, and not the first one after a reset."""
    import torch
    recs, ids = batches
    model = lm.ModelEngine(k, True, 0, oracle)
    mine = torch.zeros(4 ** k, dtype=torch.int64, device="cuda") if owner == "caller" else None
    eng = gpu_engine_cls(k, algo=2, table_ptr=mine.data_ptr() if mine is not None else None)
    with eng:
        if k == 13:
            eng.set_option("one_level_max_k", 12)
        eng.set_option("accum_bytes", 0)
        submit(eng, model, recs["A"])
        assert eng.get_option("pending_batches") == 1
        t = eng.table_tensor() if mine is None else mine
        a_ids = np.unique(ids[("A", k)])
        b_ids = np.unique(ids[("B", k)])
        both = np.union1d(a_ids, b_ids)
        # six bins that A or B count too, and six that they do not: in buckets that neither touches where there are any
        free = np.setdiff1d(np.arange(1 << (2 * k - 15), dtype=np.uint64), buckets(both, k))[:6]
        outside = [int(b) << LO_BITS | 5 for b in free.tolist()]
        spare = np.setdiff1d(np.arange(4096, dtype=np.uint64) + (a_ids[0] & ~np.uint64(4095)), both)
        outside += [int(x) for x in spare[:6 - len(outside)]]
        written = sorted(set([int(x) for x in np.intersect1d(a_ids, b_ids)[:3]] + [int(x) for x in a_ids[:3]] + outside))
        assert len(written) >= 9
        if mine is not None:
            eng.sync()
        t[torch.as_tensor(written, device="cuda")] += 5
        torch.cuda.synchronize()
        model.caller_adds(written, 5)
        submit(eng, model, recs["B"])
        same_as_model(eng, model, "table_stats")              # A + B + the writes
        with pytest.raises(Exception) as exc:
            eng.finish(copy=False)
        assert lm.error_kind(exc.value) == "sum"
        eng.reset()
        model.reset()
        one = int(a_ids[len(a_ids) // 2]) ^ 1                 # a bin inside one of A's buckets
        t[one] += 3
        torch.cuda.synchronize()
        model.caller_adds([one], 3)
        submit(eng, model, recs["A"])
        same_as_model(eng, model, "table_stats")              # A + 3


# --------------------------------------------------------------------------------------------------------------------------------
# 3. options that change with batches pending
# --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [13, 14])
def test_options_change_with_batches_pending(gpu_engine_cls, oracle, batches, k):
    recs, _ = batches
    model = lm.ModelEngine(k, True, 0, oracle)
    with two_level(gpu_engine_cls, k) as eng:
        submit(eng, model, recs["A"])
        assert eng.get_option("pending_batches") == 1
        eng.set_option("algo", 1)                             # direct atomics add B to a vector that the pending pass still believes is zero
        submit(eng, model, recs["B"])
        assert eng.get_option("pending_batches") == 1
        same_as_model(eng, model)                             # A + B: the pending pass must add
    model = lm.ModelEngine(k, True, 0, oracle)
    with two_level(gpu_engine_cls, k) as eng:
        submit(eng, model, recs["A"])
        assert (eng.get_option("pending_batches"), eng.get_option("hist_flushes")) == (1, 0)
        eng.set_option("sc_lo_bits", 9)                       # A was scattered under the old bucket field: flushed before it moves
        assert (eng.get_option("pending_batches"), eng.get_option("hist_flushes"), eng.get_option("flushed_batches")) == (0, 1, 1)
        submit(eng, model, recs["B"])
        assert eng.get_option("pending_batches") == 1
        eng.set_option("defer_flush", 0)
        assert (eng.get_option("pending_batches"), eng.get_option("hist_flushes"), eng.get_option("flushed_batches")) == (0, 2, 2)
        submit(eng, model, recs["C"])
        assert (eng.get_option("pending_batches"), eng.get_option("hist_flushes")) == (0, 3)
        same_as_model(eng, model)                             # A + B + C
    if k != 13:
        return
    model = lm.ModelEngine(k, True, 0, oracle)
    with two_level(gpu_engine_cls, k) as eng:                 # 12 -> 13 -> 12 -> 13, a batch pending at every change away from the two-level path
        submit(eng, model, recs["A"])
        assert eng.get_option("pending_batches") == 1
        eng.set_option("one_level_max_k", 13)
        assert (eng.get_option("pending_batches"), eng.get_option("hist_flushes")) == (0, 1)
        submit(eng, model, recs["B"])                         # one scatter level: added at once
        assert eng.get_option("pending_batches") == 0
        eng.set_option("one_level_max_k", 12)
        submit(eng, model, recs["C"])
        assert eng.get_option("pending_batches") == 1
        eng.set_option("one_level_max_k", 13)
        assert (eng.get_option("pending_batches"), eng.get_option("hist_flushes")) == (0, 2)
        submit(eng, model, recs["A"])
        same_as_model(eng, model)


# --------------------------------------------------------------------------------------------------------------------------------
# 4. the flush after PAGED_PENDING_MAX (64) batches
# --------------------------------------------------------------------------------------------------------------------------------
def test_sixty_four_pending_batches_are_flushed(gpu_engine_cls, oracle):
    """An arena with room for 64 batches that never grows: the 64th batch brings the pass on, not a full arena and not a sync.
    (k = 13 only: a batch's worst case is ~131 MiB of pages whatever its size -- 512 partial pages for each of the 4 + 256 digit
    spans and level-2 workgroups -- so the arena is 8.2 GiB here and would be no smaller at k = 14.)"""
    k = 13
    model = lm.ModelEngine(k, True, 0, oracle)
    with two_level(gpu_engine_cls, k, arena_batches=64, arena_grow=0) as eng:
        for i in range(70):
            submit(eng, model, reads(50, 500 + i, 120, 120))
            if i == 62:
                assert (eng.get_option("pending_batches"), eng.get_option("hist_flushes")) == (63, 0)
        assert (eng.get_option("hist_flushes"), eng.get_option("flushed_batches"), eng.get_option("pending_batches")) == (1, 64, 6)
        assert eng.get_option("arena_reallocs") == 1
        same_as_model(eng, model)


# --------------------------------------------------------------------------------------------------------------------------------
# 5. errors and recovery
# --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", lm.KINDS)
@pytest.mark.parametrize("k", [6, 11, 14])
def test_reset_after_an_error_gives_a_clean_engine(gpu_engine_cls, oracle, k, kind):
    rng = np.random.Generator(np.random.PCG64(77 + k))
    good = [reads(200, 900 + j + 10 * k) for j in range(4)]
    bad = lm._bad_batch(rng, k, kind)
    model = lm.ModelEngine(k, True, 0, oracle)
    host = lm.GpuHost()
    keep = []
    with gpu_engine_cls(k, algo=2) as eng:
        eng.set_option("accum_bytes", 1 << 20)                # host submits wait in the accumulation buffer until something flushes them
        submit(eng, model, good[0])
        assert tuple(eng.fold_file()) == tuple(model.fold())  # (so that the accumulator exists and holds counts)
        submit(eng, model, good[1])
        bases, offsets = lm.pack(bad)
        if kind == "not_uniform":
            eng.set_option("algo", 1)
        if kind in ("short", "bad_residue"):
            eng.submit(bases, offsets)
        else:
            d_b, p_b = host.to_device(bases)
            d_o, p_o = host.to_device(offsets + np.uint64(1) if kind == "bad_layout" else offsets)
            keep.append((d_b, d_o))
            (eng.submit_device if kind == "bad_layout" else eng.submit_device_const)(p_b, bases.size, p_o, len(offsets) - 1)
        model.submit_bad(kind)
        submit(eng, model, good[2])                           # a later good batch does not erase it
        for call in (eng.sync, lambda: eng.finish(copy=False), eng.fold_file, eng.nullomers, lambda: eng.table_stats(copy=False)):
            with pytest.raises(ValueError) as exc:
                call()
            assert lm.error_kind(exc.value) == kind, str(exc.value)
        print("error counts", kind, error_counts(eng))
        assert error_counts(eng) == {"short": (1, 0), "bad_residue": (0, 1)}.get(kind, (0, 0))
        submit(eng, model, good[3])                           # staged, not counted, when the reset comes
        eng.reset()
        model.reset()
        if kind == "not_uniform":
            eng.set_option("algo", 2)
        assert error_counts(eng) == (0, 0)
        assert eng.get_option("pending_batches") == 0
        assert eng.finish_folded(copy=False)[1:] == (0, 0)
        submit(eng, model, good[1])
        same_as_model(eng, model)                             # A alone: nothing staged or pending came through the reset
        assert lm._nullomer_count(eng, False) == model.nullomer_count()
        same_as_model(eng, model, "finish_folded", copy=k <= 11)
        eng.sync()


# --------------------------------------------------------------------------------------------------------------------------------
# 6. continuation pieces
# --------------------------------------------------------------------------------------------------------------------------------
def _long_records(k, seed):
    """Two records of 20..40 kB with their cuts: pieces of k - 1 and of exactly k residues, and an N inside an overlap."""
    rng = np.random.Generator(np.random.PCG64(seed))
    out = []
    for n in (int(rng.integers(20000, 30000)), int(rng.integers(30000, 40001))):
        rec = bytearray(lm.LET[rng.integers(0, 4, size=n)].tobytes())
        c = [int(rng.integers(k + 1, n // 4)), int(rng.integers(n // 4 + k, n // 2)), int(rng.integers(n // 2 + k, n - 10))]
        cuts = [c[0], c[0], c[0] + 1, c[1], c[2]] if not out else [c[0], c[1], c[2]]
        rec[c[1] - 2] = ord("N")                              # among the k - 1 residues that the piece behind cut c[1] repeats
        rec[c[2] - (k - 1)] = ord("N")                        # the first residue of the last piece
        out.append((bytes(rec), cuts))
    return out


@pytest.mark.parametrize("n_mode", [0, 1])
@pytest.mark.parametrize("k", [5, 11, 14])
def test_continuation_pieces_through_every_submit_path(gpu_engine_cls, oracle, k, n_mode):
    import torch
    longs = _long_records(k, 40 + k)
    tail = reads(50, 60 + k)
    model = lm.ModelEngine(k, True, n_mode, oracle)           # the whole records and the reads, once
    for rec, cuts in longs:
        assert 3 <= len(lm.pieces(rec, k, cuts)) <= 6
        model.submit_pieces(rec, cuts)
    model.submit(tail)
    vec, total, unique = model.finish()
    want_ids = np.fromiter(vec.keys(), dtype=np.int64, count=len(vec))
    want = np.fromiter(vec.values(), dtype=np.int64, count=len(vec))
    host = lm.GpuHost()
    for algo in (1, 2):
        for pinned in (False, True):
            for stage in (4096, None):
                for accum in (0, 1 << 20):
                    keep = []
                    with gpu_engine_cls(k, n_mode=n_mode, algo=algo) as eng:
                        if stage:
                            eng.set_option("stage_bytes", stage)
                        eng.set_option("accum_bytes", accum)
                        lm.submit_record_pieces(eng, host, k, longs[0][0], longs[0][1], tail, pinned, keep)
                        lm.submit_record_pieces(eng, host, k, longs[1][0], longs[1][1], (), pinned, keep)
                        _, g_total, g_unique = eng.finish(copy=False)           # raises on any error
                        assert (g_total, g_unique) == (total, unique), (algo, pinned, stage, accum)
                        t = eng.table_tensor()                # (nothing follows on this engine: the gather is the whole-vector compare)
                        got = t[torch.as_tensor(want_ids, device=t.device)].cpu().numpy()
                        assert np.array_equal(got, want) and int(t.sum().item()) == total, (algo, pinned, stage, accum)
                        del t


def test_the_edges_of_the_submit_cut_at_the_smallest_staging_buffer(gpu_engine_cls, oracle):
    """The edge list of tests/submit_cases.py (the engine cuts a submit itself where a record, or a run of records, does not fit a staging
    buffer) at the smallest real buffer: one batch through submit and submit_pinned, appended to the accumulated batch or counted
    from the staging slot, both counting kernels; the whole vector against the oracle's, and finish()'s own Sum check."""
    import kmerdb_amd
    import submit_cases as sc
    cap, max_recs, k = 4096, 3, 11
    lengths = [k] * 4 + [cap, cap + 1, 2 * cap - (k - 1), 2 * cap - (k - 1) + 1] + [cap + 1, k, k]
    offsets = np.array(sc.offsets_of(lengths), dtype=np.uint64)
    pieces, refusal = sc.cut([int(o) for o in offsets], False, cap, max_recs, k)
    shapes = [(p["nbytes"], p["nrecs"], p["cont"], p["inside"]) for p in pieces]
    assert refusal is None and len(pieces) == 12
    for shape in ((cap, 1, 0, 0), (cap, 1, 0, 1), (k, 1, 1, 0), (cap, 1, 1, 0), (cap, 1, 1, 1), (3 * k, 3, 0, 0), (k, 1, 0, 0), (3 * k, 3, 1, 0)):
        assert shape in shapes, shape
    rng = np.random.Generator(np.random.PCG64(11))
    bases = lm.LET[rng.integers(0, 4, size=int(offsets[-1]))].copy()
    tile = next(p for p in pieces if p["inside"])
    bases[[tile["start"] - 3, tile["start"] + cap - 6]] = ord("N")      # in a whole piece; in the k - 1 bytes a tile and the piece behind it share
    want, want_total = oracle.c_count(bases, offsets, k, True, oracle.N_DROP)
    pinned = kmerdb_amd.pinned_empty(bases.size)
    pinned[:] = bases
    for algo in (1, 2):
        for src in (bases, pinned):
            for accum in (0, 1 << 20):
                with gpu_engine_cls(k, algo=algo) as eng:
                    for name, value in (("stage_bytes", cap), ("stage_reads", max_recs), ("accum_bytes", accum)):
                        eng.set_option(name, value)
                    (eng.submit_pinned if src is pinned else eng.submit)(src, offsets)
                    counts, total, unique = eng.finish()
                    assert total == want_total and unique == int(np.count_nonzero(want)), (algo, src is pinned, accum)
                    assert np.array_equal(counts, want), (algo, src is pinned, accum)


# --------------------------------------------------------------------------------------------------------------------------------
# 7. the fixed seeds, through the driver that the stand-in engine passed on the CPU
# --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,seed", lm.SEEDS)
def test_seeded_sequence_equals_the_model(gpu_engine_cls, oracle, k, seed):
    ops = lm.fixed_sequence(k, seed)
    pend = lm.pending_before(ops, k)
    seen = []

    def observe(i, op, eng):
        # where the order of ops is meant to catch a batch in the arena, it is there (small counts: an arena of eight holds them for sure)
        if op["op"] == "set_option" and not op.get("init") and pend[i] is not None and 0 < pend[i] <= 4:
            assert eng.get_option("pending_batches") == pend[i], (i, op)
            seen.append(i)

    model = lm.ModelEngine(k, ops[0]["canon"], ops[0]["n_mode"], oracle)
    checks = lm.run_sequence(lambda canon, n_mode: gpu_engine_cls(k, canonicalize=canon, n_mode=n_mode), ops, model, observe=observe)
    print("k=%d seed %d: %d ops, %d checks, options changed over pending batches at ops %s" % (k, seed, len(ops), len(checks), seen))
    assert len(checks) >= 3
