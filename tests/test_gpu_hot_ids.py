"""The "same id in many lanes" shortcuts of the counting kernels at their edges: the cases of tests/hot_cases.py (each proven, by
tests/test_hot_cases_cpu.py, to reach the branch it names) counted by the engine and compared, bin for bin, with the oracle.

  k <= 13: the whole vector against oracle.c_count; k >= 14: the oracle's ids and counts against a gather from the vector, and
  Sum(vector) == total, which leaves every other bin zero (test_gpu_parity's sparse compare).  total and unique always.
A job is a few cases submitted one after the other to one engine and read once.  Every engine here runs with `accum_bytes` 0, so that
each submit is a device batch, and a launch, of its own: the residues lie where the model puts them."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fuzz_gpu  # noqa: E402
import hot_cases as hc  # noqa: E402
import lifecycle_model as lm  # noqa: E402
from test_gpu_lifecycle import BUCKET_STORE_BYTES, buckets, reads  # noqa: E402
from test_gpu_parity import _sparse_expect, _sparse_got  # noqa: E402

pytestmark = pytest.mark.gpu

_EXPECT = {}


@pytest.fixture(scope="module", autouse=True)
def _drop_expectations():
    """the dense oracle vectors (512 MiB each at k = 13) go when the module ends"""
    yield
    _EXPECT.clear()


def expectation(oracle, key, cases, k, canon, expand):
    """What the oracle counts for the records of `cases` together (computed once per key, never changed)."""
    key = (key, k, canon, expand)
    if key not in _EXPECT:
        omode = oracle.N_EXPAND if expand else oracle.N_DROP
        if k <= 13:
            bases = np.concatenate([c.bases for c in cases])
            offs = np.concatenate([[0], np.cumsum(np.concatenate([np.diff(c.offsets.astype(np.int64)) for c in cases]))]).astype(np.uint64)
            counts, total = oracle.c_count(bases, offs, k, canon, omode)
            _EXPECT[key] = ("dense", counts, total, int(np.count_nonzero(counts)))
        else:
            uniq, cnt, total = _sparse_expect(oracle, [r for c in cases for r in c.records], k, canon, omode)
            _EXPECT[key] = ("sparse", (uniq, cnt), total, int(uniq.size))
    return _EXPECT[key]


def same_as_oracle(eng, exp, what=""):
    kind, want, total, unique = exp
    if kind == "dense":
        got, g_total, g_unique = eng.finish()
        print(what, "engine", (g_total, g_unique), "oracle", (total, unique))
        assert (g_total, g_unique) == (total, unique), what
        diff = np.flatnonzero(got != want)
        assert diff.size == 0, "%s: %d bins differ, first id %d: got %d, want %d" % (what, diff.size, diff[0], got[diff[0]], want[diff[0]])
    else:
        _, g_total, g_unique = eng.finish(copy=False)
        print(what, "engine", (g_total, g_unique), "oracle", (total, unique))
        assert (g_total, g_unique) == (total, unique), what
        uniq, cnt = want
        got = _sparse_got(eng, uniq)
        diff = np.flatnonzero(got != cnt)
        assert diff.size == 0, "%s: %d ids differ, first id %d: got %d, want %d" % (what, diff.size, uniq[diff[0]], got[diff[0]], cnt[diff[0]])
        assert int(eng.table_tensor().sum().item()) == total, what


def submit(eng, case, device=False, keep=None):
    if not device:
        eng.submit(case.bases, case.offsets)
        return
    import torch
    d_b = torch.from_numpy(case.bases.copy()).cuda()
    d_o = torch.from_numpy(case.offsets.view(np.int64).copy()).cuda()
    keep.append((d_b, d_o))                         # (asynchronous: the buffers live until the read)
    eng.submit_device(d_b.data_ptr(), case.bases.size, d_o.data_ptr(), len(case.offsets) - 1)


def engine(cls, k, **kw):
    """An engine that counts every host submit as a device batch of its own: at k >= 13 the default (`accum_bytes` -1) gathers host submits on
    the device and counts them as ONE batch at the read -- the cases' residues would lie end to end, not where the model puts them."""
    eng = cls(k, **kw)
    eng.set_option("accum_bytes", 0)
    return eng


DEFAULTS = {"algo": 2, "smallk_old": 0, "strand_merge": 1, "sc_wide_lines": 1, "l1_wide_lines": 1, "one_level_max_k": 13, "sc_grid": 0, "defer_flush": 1,
            "overlap": 0}


def configure(eng, opts):
    for name, v in dict(DEFAULTS, **opts).items():
        if eng.get_option(name) != v:               # (a change of some options syncs the engine and makes its streams anew)
            eng.set_option(name, v)


# --------------------------------------------------------------------------------------------------------------------------------
# 1. threshold, leader, periods, both_strands: every path, both record forms, host and device submits
# --------------------------------------------------------------------------------------------------------------------------------
def _paths(k, canon):
    if k <= 8:
        p = [("default", {}), ("smallk_old", {"smallk_old": 1}), ("direct", {"algo": 1})]
    elif k <= 12:
        p = [("default", {}), ("narrow", {"sc_wide_lines": 0}), ("direct", {"algo": 1})]
    elif k == 13:
        p = [("default", {}), ("two_level", {"one_level_max_k": 12}), ("two_level_narrow", {"one_level_max_k": 12, "l1_wide_lines": 0}), ("direct", {"algo": 1})]
    else:
        p = [("default", {}), ("narrow", {"l1_wide_lines": 0}), ("direct", {"algo": 1})]
    if canon and k <= 12:                           # the CANON = true kernels themselves: strands folded per window, not at the sync
        p += [("unmerged", {"strand_merge": 0})] + ([("unmerged_narrow", {"strand_merge": 0, "sc_wide_lines": 0})] if k > 8 else [])
    return p


LAYOUT_PARAMS = [(k, canon, name) for k in (5, 8, 9, 12, 13, 14, 16) for canon in (False, True) for name, _ in _paths(k, canon)]


@pytest.mark.parametrize("k,canon,path", LAYOUT_PARAMS)
def test_layout_cases_equal_the_oracle(gpu_engine_cls, oracle, k, canon, path):
    opts = dict(_paths(k, canon))[path]
    for expand in (False, True):
        builders = (hc.leader, hc.periods) if expand else (hc.threshold, hc.leader, hc.periods, hc.both_strands)
        with engine(gpu_engine_cls, k, canonicalize=canon, n_mode=1 if expand else 0) as eng:
            configure(eng, opts)
            for ragged in (False, True):
                cases = [b(k, ragged) for b in builders]
                exp = expectation(oracle, ("layout", ragged), cases, k, canon, expand)
                for device in ((False, True) if path in ("default", "direct", "unmerged") else (False,)):
                    keep = []
                    eng.reset()
                    for c in cases:
                        submit(eng, c, device, keep)
                    same_as_oracle(eng, exp, "k=%d canon=%d %s expand=%d ragged=%d device=%d" % (k, canon, path, expand, ragged, device))


# --------------------------------------------------------------------------------------------------------------------------------
# 2. more hot ids than a workgroup's table has slots: conflicts, direct adds, and the side list under overlap
# --------------------------------------------------------------------------------------------------------------------------------
MANY_PARAMS = [(9, 13), (12, 13), (13, 13), (13, 12), (15, 13)]


@pytest.mark.parametrize("k,one_level_max_k", MANY_PARAMS)
def test_many_hot_ids_in_one_workgroup(gpu_engine_cls, oracle, k, one_level_max_k):
    small = hc.many_ids(hc.MANY_SMALL)
    for canon in (False, True):
        exp = expectation(oracle, "many_small", [small], k, canon, False)
        with engine(gpu_engine_cls, k, canonicalize=canon, algo=2) as eng:
            for defer in ((1, 0) if k > one_level_max_k else (1,)):
                for merge in ((1, 0) if canon and k <= 12 else (1,)):
                    configure(eng, {"sc_grid": 1, "one_level_max_k": one_level_max_k, "defer_flush": defer, "strand_merge": merge})
                    eng.reset()
                    submit(eng, small)
                    same_as_oracle(eng, exp, "k=%d canon=%d sc_grid=1 defer=%d merge=%d" % (k, canon, defer, merge))


@pytest.mark.parametrize("k,one_level_max_k", MANY_PARAMS)
def test_many_hot_ids_in_every_workgroup_of_the_default_grid(gpu_engine_cls, oracle, k, one_level_max_k):
    big = hc.many_ids(hc.MANY_DEFAULT)
    exp = expectation(oracle, "many_default", [big], k, False, False)
    with engine(gpu_engine_cls, k, canonicalize=False, algo=2) as eng:
        for defer in ((1, 0) if k > one_level_max_k else (1,)):
            configure(eng, {"one_level_max_k": one_level_max_k, "defer_flush": defer})
            eng.reset()
            submit(eng, big)
            same_as_oracle(eng, exp, "k=%d default grid defer=%d" % (k, defer))


@pytest.mark.parametrize("sc_grid", [1, 0])
@pytest.mark.parametrize("k", [9, 12, 13])
def test_many_hot_ids_under_overlap(gpu_engine_cls, oracle, k, sc_grid):
    """Four batches in a row: a scatter kernel runs beside the histogram pass of the batch before it, both side lists are used twice."""
    batches = [hc.many_ids(n, seed=s) for s, n in enumerate((hc.MANY_SMALL, 40, hc.MANY_SMALL + 1, 41))]
    for canon in (False, True):
        exp = expectation(oracle, "many_overlap", batches, k, canon, False)
        with engine(gpu_engine_cls, k, canonicalize=canon, algo=2) as eng:
            configure(eng, {"overlap": 1, "sc_grid": sc_grid})
            for b in batches:
                submit(eng, b)
            same_as_oracle(eng, exp, "k=%d canon=%d overlap sc_grid=%d" % (k, canon, sc_grid))


@pytest.mark.parametrize("canon", [False, True])
def test_side_list_holds_a_batch_of_many_distinct_repeats(gpu_engine_cls, oracle, canon):
    """6 MiB of period-16 repeats, 384 distinct units, one workgroup: at least 92 000 groups find the table's 64 slots taken
    (test_hot_cases_cpu.py).  The side list held 65 600 pairs whatever the batch; the engine then failed the job at the sync with
    KDB_ERR_STATE, "a scatter kernel ran out of its page sequence ... counts are incomplete", on input that is perfectly valid."""
    case = hc.side_overflow()
    exp = expectation(oracle, "side_overflow", [case], 12, canon, False)
    with engine(gpu_engine_cls, 12, canonicalize=canon, algo=2) as eng:
        configure(eng, {"overlap": 1, "sc_grid": 1})
        submit(eng, case)
        same_as_oracle(eng, exp, "side_overflow canon=%d" % canon)


# --------------------------------------------------------------------------------------------------------------------------------
# 3. ids equal in their low 32 bits
# --------------------------------------------------------------------------------------------------------------------------------
def test_k17_hot_ids_that_differ_above_bit_31(gpu_engine_cls, oracle):
    case = hc.high_bits()
    exp = expectation(oracle, "high_bits", [case], 17, False, False)
    with engine(gpu_engine_cls, 17, canonicalize=False, algo=2) as eng:
        submit(eng, case)
        same_as_oracle(eng, exp, "k=17 algo 2")
        eng.reset()
        eng.set_option("algo", 1)
        submit(eng, case)
        same_as_oracle(eng, exp, "k=17 algo 1")


@pytest.mark.parametrize("algo", [2, 1])
def test_k16_twin_of_the_high_bits_case(gpu_engine_cls, oracle, algo):
    case = hc.high_bits()
    for canon in (False, True):
        exp = expectation(oracle, "high_bits", [case], 16, canon, False)
        with engine(gpu_engine_cls, 16, canonicalize=canon, algo=algo) as eng:
            submit(eng, case)
            same_as_oracle(eng, exp, "k=16 algo %d canon=%d" % (algo, canon))


# --------------------------------------------------------------------------------------------------------------------------------
# 4. one k-mer that is never hot: 150 000 times through the rings
# --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,opts", [(12, {}), (13, {}), (13, {"one_level_max_k": 12}), (13, {"one_level_max_k": 12, "defer_flush": 0})])
def test_planted_kmer_floods_one_bucket(gpu_engine_cls, oracle, k, opts):
    case = hc.planted(k)
    exp = expectation(oracle, "planted", [case], k, False, False)
    with engine(gpu_engine_cls, k, canonicalize=False, algo=2) as eng:
        configure(eng, opts)
        submit(eng, case)
        same_as_oracle(eng, exp, "planted k=%d %r" % (k, opts))


# --------------------------------------------------------------------------------------------------------------------------------
# 5. table_dirty over an engine's life (engine-owned vector, DROP, deferred pass), through lifecycle_model's driver
# --------------------------------------------------------------------------------------------------------------------------------
def _life(k, body):
    ops = [{"op": "create", "canon": True, "n_mode": 0}, {"op": "set_option", "init": True, "name": "accum_bytes", "value": 0},
           {"op": "set_option", "init": True, "name": "algo", "value": 2}]
    if k == 13:
        ops.append({"op": "set_option", "init": True, "name": "one_level_max_k", "value": 12})
    return ops + body


def _sub(records):
    return {"op": "submit_host", "records": records}


def _run(gpu_engine_cls, oracle, k, ops):
    """-> bytes of the vector that each sync's histogram pass moved, by op index."""
    moved, last = {}, {}

    def observe(i, op, eng):
        if "sync" in last:
            moved[last.pop("sync")] = eng.get_option("table_bytes") - last.pop("bytes")
        if op["op"] == "sync":
            last["sync"], last["bytes"] = i, eng.get_option("table_bytes")

    model = lm.ModelEngine(k, True, 0, oracle)
    checks = lm.run_sequence(lambda canon, n_mode: gpu_engine_cls(k, canonicalize=canon, n_mode=n_mode), ops, model, observe=observe)
    assert checks
    return moved


def _hot_records(k):
    return hc.threshold(k).records + hc.leader(k).records + hc.many_ids(2, n_random=0).records


def _store_bytes(oracle, records, k):
    ids = np.concatenate([oracle.c_shred(r, k, True, oracle.N_DROP)[0] for r in records])
    return BUCKET_STORE_BYTES * len(buckets(ids, k))


@pytest.mark.parametrize("k", [13, 14])
def test_hot_batch_then_random_then_sync(gpu_engine_cls, oracle, k):
    _run(gpu_engine_cls, oracle, k, _life(k, [_sub(_hot_records(k)), _sub(reads(2000, 21)), {"op": "sync"}, {"op": "finish", "copy": True}]))


@pytest.mark.parametrize("k", [13, 14])
def test_random_sync_hot_sync(gpu_engine_cls, oracle, k):
    rnd = reads(2000, 22)
    moved = _run(gpu_engine_cls, oracle, k, _life(k, [_sub(rnd), {"op": "sync"}, _sub(_hot_records(k)), {"op": "sync"}, {"op": "finish", "copy": True}]))
    first = min(moved)
    print("k=%d: the first pass moved %d bytes, store form %d" % (k, moved[first], _store_bytes(oracle, rnd, k)))
    assert moved[first] == _store_bytes(oracle, rnd, k)           # nothing had been added directly yet


@pytest.mark.parametrize("k", [13, 14])
def test_dirt_does_not_outlive_a_reset(gpu_engine_cls, oracle, k):
    rnd = reads(2000, 23)
    moved = _run(gpu_engine_cls, oracle, k, _life(k, [_sub(_hot_records(k)), {"op": "reset"}, _sub(rnd), {"op": "sync"}, {"op": "finish", "copy": True}]))
    (got,) = moved.values()
    print("k=%d: the pass behind the reset moved %d bytes, store form %d" % (k, got, _store_bytes(oracle, rnd, k)))
    assert got == _store_bytes(oracle, rnd, k)                    # the store form is back


@pytest.mark.parametrize("k", [13, 14])
def test_hot_fold_random_finish_folded(gpu_engine_cls, oracle, k):
    _run(gpu_engine_cls, oracle, k, _life(k, [_sub(_hot_records(k)), {"op": "fold"}, _sub(reads(2000, 24)), {"op": "finish", "copy": k == 13}, {"op": "fold"},
                                              {"op": "finish_folded", "copy": True}]))


@pytest.mark.parametrize("k", [13, 14])
def test_hot_id_in_a_bucket_that_no_page_touches(gpu_engine_cls, oracle, k):
    """poly-A in whole waves: every window of it is hot, id 0 is added to the vector and reaches no ring; the three random reads beside it
    touch other buckets.  The pass stores or adds around a bin that only the direct add wrote."""
    few = reads(3, 25, 60, 60)
    ids = np.concatenate([oracle.c_shred(r, k, True, oracle.N_DROP)[0] for r in few])
    assert 0 not in buckets(ids, k).tolist()
    _run(gpu_engine_cls, oracle, k, _life(k, [_sub(hc.all_hot(k).records + few), {"op": "sync"}, {"op": "finish", "copy": True}]))


@pytest.mark.parametrize("n", [15, 16])
@pytest.mark.parametrize("k", [13, 14])
def test_groups_of_exactly_15_and_16_by_the_form_of_the_pass(gpu_engine_cls, oracle, k, n):
    """The threshold itself shows in no count -- a group is the lanes with one id whatever its size -- but in what it does to the vector:
    a batch whose groups all have 15 members adds nothing directly, and the deferred pass may store; one with groups of 16 must add.
    Store form: 8 bytes for each of the 32768 bins of a touched bucket; add form: 32 bytes per pair of adjacent bins that the pages
    hold (test_gpu_lifecycle.py, case 1) -- the ids that the model leaves to the rings."""
    case = hc.exact_groups(k, n)
    moved = _run(gpu_engine_cls, oracle, k, _life(k, [_sub(case.records), {"op": "sync"}, {"op": "finish", "copy": True}]))
    (got,) = moved.values()
    m = hc.lane_model(case, k, True, 1024)
    store = _store_bytes(oracle, case.records, k)
    add = 32 * len(np.unique(m.ring_ids() >> np.uint64(1)))
    print("k=%d groups of %d: the pass moved %d bytes; store form %d, add form %d" % (k, n, got, store, add))
    assert store != add and got == (store if n == 15 else add)


@pytest.mark.parametrize("k", [13, 14])
def test_first_live_lane_leads_by_the_form_of_the_pass(gpu_engine_cls, oracle, k):
    """Which lane leads shows in no count either.  hot_cases.dead_leader: the only groups of 16 or more sit in slots where lane 0 is dead and the
    id that its residues would give is another one.  The first live lane leads them to the vector, so the pass must take its add form; a
    kernel that asked lane 0 would find no group, leave the vector clean and let the pass store."""
    case = hc.dead_leader(k)
    moved = _run(gpu_engine_cls, oracle, k, _life(k, [_sub(case.records), {"op": "sync"}, {"op": "finish", "copy": True}]))
    (got,) = moved.values()
    m = hc.lane_model(case, k, True, 1024)
    store = _store_bytes(oracle, case.records, k)
    add = 32 * len(np.unique(m.ring_ids() >> np.uint64(1)))
    print("k=%d dead leader: the pass moved %d bytes; store form %d, add form %d" % (k, got, store, add))
    assert store != add and got == add


# --------------------------------------------------------------------------------------------------------------------------------
# 6. seeded mixed batches, options drawn as tests/fuzz_gpu.py draws them
# --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kclass,seed", [(c, s) for c in sorted(hc.K_CLASSES) for s in hc.REPEAT_SEEDS])
def test_seeded_repeats_equal_the_oracle(gpu_engine_cls, oracle, kclass, seed):
    desc, case = hc.fixed_repeat(kclass, seed)
    print(desc)
    assert fuzz_gpu.check_case(desc, case.bases, case.offsets), desc
