"""GPU: kdb_score_reads -- Markov log-probabilities of reads under a profile (csrc/kdb_score.hip.h) -- against the numpy + decimal oracle of
tests/score_cases.py, and the layers above it (kmerdb_amd.probability, the `probability` subcommand).

The integer outputs are compared bit for bit.  log10_p is compared within score_cases.bound, derived there from the kernel's actual
summation depth: u = 2^-53; per term two integer-to-float64 conversions, two logarithms within 1 ulp and one subtraction,
e_t = u (2 + 2 |ln c| + 2 |ln D| + |t|); over the sum depth x u x Sum |t| with
    depth = KDB_SCORE_PIECE / KDB_SCORE_LANES + log2(KDB_SCORE_LANES) + 2 x pieces (+ 3 per KDB_SCORE_CONTINUES join)
(2048 / 64 + 6 + 2 = 40 for a record of one piece); and 2 u |log10_p| for the division by ln 10.  tests/test_score_cpu.py checks that
plain float64 numpy is inside the same bound on the same inputs (worst share 0.10).  Measured worst share on the device: DESIGN section 14.
Every test here fails without kdb_score_reads: the library does not export the symbol."""
import ctypes
import io
import math
import os
import re

import numpy as np
import pytest

import score_cases as sc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOP = sc.TOP
NO_WINDOW = np.uint64(TOP)


def _header_constant(name):
    text = open(os.path.join(ROOT, "include", "kdbhip.h")).read()
    return int(re.search(r"#define\s+%s\s+(\d+)" % name, text).group(1))


PIECE, LANES = _header_constant("KDB_SCORE_PIECE"), _header_constant("KDB_SCORE_LANES")


@pytest.fixture(scope="module")
def dev(gpu_engine_cls):
    import torch
    from kmerdb_amd import _abi, probability

    class Dev:
        lib = _abi.lib()
        OK, ARG, SHORT, BAD = _abi.KDB_OK, _abi.KDB_ERR_ARG, _abi.KDB_ERR_SHORT_READ, _abi.KDB_ERR_BAD_RESIDUE

        @staticmethod
        def upload(v):
            return torch.from_numpy(np.ascontiguousarray(v, dtype=np.uint64).view(np.int64)).to("cuda:0")

        @staticmethod
        def score(records, t, k, canonical, total, a=0, continues=False):
            bases, offsets = sc.pack(records)
            return probability.score_reads(bases, offsets, t, k, canonical, total, a, continues=continues)

        @classmethod
        def raw(cls, ptr, k, canonical, total, a, bases, offsets, flags=0, nreads=None, nbytes=None, null=()):
            """kdb_score_reads with arguments as given -> status"""
            n = len(offsets) - 1 if nreads is None else nreads
            outs = [np.zeros(max(n, 1), dtype=np.float64)] + [np.zeros(max(n, 1), dtype=np.uint64) for _ in range(3)]
            po = [None if i in null else o.ctypes.data for i, o in enumerate(outs)]
            torch.cuda.synchronize(0)
            return cls.lib.kdb_score_reads(0, ctypes.c_void_p(ptr), k, canonical, total, a, None if "bases" in null else bases.ctypes.data,
                                           bases.size if nbytes is None else nbytes, None if "offsets" in null else offsets.ctypes.data, n, flags,
                                           po[0], po[1], po[2], po[3], None)
    return Dev


_WORST = {"share": 0.0}


def _check_batch(dev, records, v, t, k, canonical, total, a=0, continues=False, floats=True, name=""):
    """one call against the oracle, record by record -> the device's four arrays"""
    got = dev.score(records, t, k, canonical, total, a, continues)
    log10_p, windows, zeros, mins = got
    for r, rec in enumerate(records):
        s = sc.score_record(rec, v, k, canonical, total, a, continues=continues and r == 0)
        where = (name, r, len(rec))
        assert (int(windows[r]), int(zeros[r]), int(mins[r])) == (s.windows, s.zero_windows, s.min_count), where
        if s.log10_p is None:
            assert math.isnan(log10_p[r]) and int(mins[r]) == TOP and int(windows[r]) == 0, where
        elif s.log10_p == float("-inf"):
            assert log10_p[r] == float("-inf") and int(zeros[r]) > 0, where
        elif floats:
            eps, err = sc.bound(s, PIECE, LANES), sc.error(log10_p[r], s)
            _WORST["share"] = max(_WORST["share"], err / eps)
            assert err <= eps, where + (err, eps)
    return got


# ---- integer outputs, and the scored windows against kdb_window_ids ----

@pytest.mark.parametrize("k,canonical", [(1, False), (2, False), (3, False), (3, True), (8, False), (8, True), (12, False), (13, False), (13, True)])
def test_integer_outputs_bit_for_bit_and_windows_as_kdb_window_ids(dev, k, canonical):
    from kmerdb_amd.engine import IdsEngine
    records = sc.ladder_records(k, PIECE, 300 + k, p_n=0.003) + sc.n_records(k) + sc.ragged_records(k, 400 + k, n=30)
    # the profile knows half of the records: the others meet bins that are 0
    v, _ = (sc.canonical_profile if canonical else sc.forward_profile)(records[::2], k)
    v[1::3] = 0                                                              # (at small k half of the records already hold every k-mer)
    total = int(v.sum())
    t = dev.upload(v)
    log10_p, windows, zeros, mins = _check_batch(dev, records, v, t, k, canonical, total, floats=False, name="k=%d" % k)
    bases, offsets = sc.pack(records)
    with IdsEngine(k, canonicalize=False) as ids_engine:
        ids = ids_engine.window_ids(bases, offsets)
    per_record = [int(np.count_nonzero(ids[int(s):int(e)] != NO_WINDOW)) for s, e in zip(offsets[:-1], offsets[1:])]
    assert windows.tolist() == per_record
    assert int(zeros.sum()) > 0 and int(np.count_nonzero(windows == 0)) >= 2 and float("-inf") in log10_p.tolist()
    # a pseudocount of 1 makes the same reads finite; the integers do not move
    lp1, w1, z1, m1 = dev.score(records, t, k, canonical, total, 1)
    assert np.all(np.isfinite(lp1[windows > 0])) and np.all(np.isnan(lp1[windows == 0]))
    assert (w1.tobytes(), z1.tobytes(), m1.tobytes()) == (windows.tobytes(), zeros.tobytes(), mins.tobytes())


# ---- log10_p within the bound of its roundings ----

@pytest.mark.parametrize("case", range(sc.N_ACCURACY_CASES))
def test_log10_p_within_the_bound_of_its_roundings(dev, case):
    name, k, canonical, v, total, a, records = sc.accuracy_cases(PIECE)[case]
    t = dev.upload(v)
    log10_p, windows, zeros, _ = _check_batch(dev, records, v, t, k, canonical, total, a, name=name)
    assert np.count_nonzero(np.isfinite(log10_p)) >= 8 and not np.any(np.isinf(log10_p))
    print(name, "worst share of the bound so far", _WORST["share"])
    again = dev.score(records, t, k, canonical, total, a)                    # two calls: the same bits
    assert all(x.tobytes() == y.tobytes() for x, y in zip(again, (log10_p, windows, zeros, _)))


def test_reads_against_their_own_profile_are_finite_and_an_unseen_kmer_is_not(dev):
    k = 8
    records = sc.ragged_records(k, 21, n=60, p_n=0.0)
    v, total = sc.forward_profile(records, k)
    t = dev.upload(v)
    log10_p, windows, zeros, mins = _check_batch(dev, records, v, t, k, False, total, name="own")
    assert np.all(np.isfinite(log10_p)) and np.all(log10_p < 0) and not zeros.any() and np.all(mins >= 1)
    absent = sc.id_kmer(int(np.flatnonzero(v == 0)[0]), k).encode()
    odd = [records[0] + absent, absent + records[1], records[2]]
    lp, w, z, m = _check_batch(dev, odd, v, t, k, False, total, name="unseen")
    assert lp[0] == lp[1] == float("-inf") and z[0] > 0 and z[1] > 0 and m[0] == m[1] == 0 and lp[2] == log10_p[2]
    lp1 = _check_batch(dev, odd, v, t, k, False, total, 1, name="unseen, pseudocount 1")[0]
    assert np.all(np.isfinite(lp1))


# ---- exact metamorphic equalities ----

@pytest.mark.parametrize("k", [2, 5, 8])
def test_canonical_scoring_is_forward_scoring_of_the_symmetrised_vector(dev, k):
    records = sc.ladder_records(k, PIECE, 500 + k, p_n=0.002) + sc.ragged_records(k, 600 + k, n=20)
    v, total = sc.canonical_profile(records[1::2], k)
    a = dev.score(records, dev.upload(v), k, True, total, 2)
    b = dev.score(records, dev.upload(sc.symmetrised(v, k)), k, False, total, 2)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    assert np.count_nonzero(np.isfinite(a[0])) > 20


@pytest.mark.parametrize("k,a", [(3, 1), (6, 7), (8, 2 ** 40)])
def test_a_pseudocount_is_the_vector_plus_a(dev, k, a):
    records = sc.ladder_records(k, PIECE, 700 + k) + sc.ragged_records(k, 800 + k, n=20)
    v = sc.spread_vector(k, k)
    total = int(v.sum())
    lp, w, z, m = dev.score(records, dev.upload(v), k, False, total, a)
    lp2, w2, z2, m2 = dev.score(records, dev.upload(v + np.uint64(a)), k, False, total + a * 4 ** k, 0)
    assert lp.tobytes() == lp2.tobytes() and w.tobytes() == w2.tobytes() and np.all(np.isfinite(lp))
    assert np.all(m2 == m + np.uint64(a)) and not z2.any() and z.any()       # (the bins themselves differ by a)


def test_a_record_scores_the_same_alone_among_others_and_in_reversed_order(dev):
    k = 7
    records = sc.ladder_records(k, PIECE, 31, p_n=0.002) + sc.n_records(k) + sc.ragged_records(k, 32, n=25)
    v, total = sc.forward_profile(records[::3], k)
    t = dev.upload(v)
    whole = dev.score(records, t, k, False, total, 1)
    rev = dev.score(records[::-1], t, k, False, total, 1)
    assert all(x.tobytes() == y[::-1].tobytes() for x, y in zip(whole, rev))
    for r in (0, 3, 7, 8, 9, 11, len(records) - 1):                          # one piece, PIECE + 1 and 2 PIECE + 1 windows, N layouts, a ragged one
        alone = dev.score([records[r]], t, k, False, total, 1)
        assert all(x[0:1].tobytes() == y[r:r + 1].tobytes() for x, y in zip(alone, whole)), r
    again = dev.score(records, t, k, False, total, 1)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(again, whole))


# ---- wide arithmetic ----

def test_ids_above_2_31_and_byte_offsets_above_2_32_at_k16(dev):
    import torch
    k = 16
    try:
        t = torch.zeros(4 ** k, dtype=torch.int64, device="cuda:0")
    except (RuntimeError, MemoryError) as e:
        pytest.skip("no room for the 32 GiB vector of k = 16: {0}".format(e))
    kmers = ["ACGT" * 4, "C" + "A" * 15, "G" + "T" * 15, "GATTACAGATTACAGA", "T" * 16, "T" * 15 + "G", "TTGCATGCATGCATGC", "A" * 16]
    ids = [sc.kmer_id(x) for x in kmers]
    assert sum(i >= 2 ** 31 for i in ids) >= 4 and sum(i * 8 >= 2 ** 32 for i in ids) >= 6
    sparse = {i: 3 + 5 * n for n, i in enumerate(ids)}
    t[torch.tensor(ids, device="cuda:0")] = torch.tensor([sparse[i] for i in ids], dtype=torch.int64, device="cuda:0")
    total = sum(sparse.values())

    class Sparse:                                                            # the oracle's view of the vector: zeros but for the set bins
        def __len__(self):
            return 4 ** k

        def __getitem__(self, i):
            return sparse.get(int(i), 0)

    records = [x.encode() for x in kmers] + [("T" * 17).encode(), ("G" + "T" * 15 + "T" * 3).encode(), ("ACGT" * 5).encode()]
    for canonical in (False, True):
        got = _check_batch(dev, records, Sparse(), t, k, canonical, total, 1, name="k=16")
        assert np.all(np.isfinite(got[0]))
    del t
    torch.cuda.empty_cache()


@pytest.mark.parametrize("k", [14, 15, 17])
def test_the_decode_at_k_14_15_17_at_every_byte_alignment(dev, k):
    """window_id's fourth and fifth word: m[3] covers two (k = 14) and three (k = 15) bytes, and k = 17 alone uses m[4] and
    x[4] = w[2] >> s, of which it needs the one byte that has no word behind it.  The vectors are 2 GiB, 8 GiB and 128 GiB, zero but for
    a few bins.  Per alignment of the window's start: k-mers that differ in their last residue, in residue 13 and in residue 12 hold
    different counts; an N one past the window's end leaves the window scored, an N as its last residue does not; the last record ends
    where the buffer does."""
    import torch
    try:
        t = torch.zeros(4 ** k, dtype=torch.int64, device="cuda:0")
    except (RuntimeError, MemoryError) as e:
        pytest.skip("no room for the {0} GiB vector of k = {1}: {2}".format(4 ** k * 8 // 2 ** 30, k, e))
    try:
        kmers = sc.decode_edge_kmers(k)
        corners = [("ACGT" * 5)[:k], "C" + "A" * (k - 1), "G" + "T" * (k - 1), "T" * k, "T" * (k - 1) + "G", "A" * k]
        ids = []
        for x in list(kmers.values()) + corners:                             # the k-mers and their reverse complements: canonical lookups differ too
            for i in (sc.kmer_id(x), sc.rc_id(sc.kmer_id(x), k)):
                if i not in ids:
                    ids.append(i)
        if k == 17:
            assert sum(i >= 2 ** 32 for i in ids) >= 4 and sum(i * 8 >= 2 ** 36 for i in ids) >= 4
        sparse = {i: 3 + 5 * n for n, i in enumerate(ids)}
        t[torch.tensor(ids, device="cuda:0")] = torch.tensor([sparse[i] for i in ids], dtype=torch.int64, device="cuda:0")
        total = sum(sparse.values())

        class Sparse:                                                        # the oracle's view of the vector: zeros but for the set bins
            def __len__(self):
                return 4 ** k

            def __getitem__(self, i):
                return sparse.get(int(i), 0)

        count = {name: sparse[sc.kmer_id(x)] for name, x in kmers.items()}
        assert len(set(count.values())) == (3 if k == 14 else 4)
        for alignment in range(8):
            records, roles = sc.decode_edge_records(k, alignment, start=len(corners) * k)
            records = [x.encode() for x in corners] + records
            _, offsets = sc.pack(records)
            at = {role: i + len(corners) for role, i in roles.items()}
            assert all(int(offsets[i]) % 8 == alignment for i in at.values()) and at["ends_buffer"] == len(records) - 1
            for canonical in (False, True):
                got = _check_batch(dev, records, Sparse(), t, k, canonical, total, 1, name="k=%d alignment %d" % (k, alignment))
                log10_p, windows, zeros, mins = got
                assert [int(windows[at[r]]) for r in sc.DECODE_EDGE_ROLES] == [1, 1, 1, 1, 1, 0, 2, 2 * k + 1, 1]
                assert math.isnan(log10_p[at["n_last"]]) and np.all(np.isfinite(np.delete(log10_p, at["n_last"])))
                if not canonical:
                    assert [int(mins[at[r]]) for r in ("alone", "last", "r13", "r12", "n_after", "n_after_more", "ends_buffer")] == \
                        [count["K"], count["last"], count["r13"], count["r12"], count["K"], count["K"], count["K"]]
                    assert int(zeros[at["inside"]]) == 2 * k + 1 - 3 and int(zeros[at["n_after_more"]]) == 0
    finally:
        del t
        torch.cuda.empty_cache()


# ---- KDB_SCORE_CONTINUES ----

@pytest.mark.parametrize("k", [1, 4, 9])
def test_a_long_record_cut_into_continuation_pieces_joins(dev, k):
    rng = np.random.default_rng(90 + k)
    whole = sc.random_record(rng, 3 * PIECE + 1000, p_n=0.001)
    v, total = sc.forward_profile([whole], k)
    t = dev.upload(v)
    ref = sc.score_record(whole, v, k, False, total)
    one = dev.score([whole], t, k, False, total)
    cuts = [0, 70, PIECE + k, PIECE + k + 5, 2 * PIECE + 517, len(whole)]
    lp, windows, zeros, mn = 0.0, 0, 0, TOP
    for n, (a, b) in enumerate(zip(cuts[:-1], cuts[1:])):
        piece = whole[max(0, a - (k - 1)):b]
        other = sc.random_record(rng, k + 20)                                 # a second record in the call: only record 0 continues
        got = _check_batch(dev, [piece, other], v, t, k, False, total, 1, continues=n > 0, floats=False, name="piece %d" % n)
        got = dev.score([piece, other], t, k, False, total, 0, continues=n > 0)
        lp, windows, zeros, mn = lp + float(got[0][0]), windows + int(got[1][0]), zeros + int(got[2][0]), min(mn, int(got[3][0]))
    assert (windows, zeros, mn) == (ref.windows, ref.zero_windows, ref.min_count) == (int(one[1][0]), int(one[2][0]), int(one[3][0]))
    eps = sc.bound(ref, PIECE, LANES, joins=len(cuts) - 2)
    assert sc.error(lp, ref) <= eps and sc.error(one[0][0], ref) <= sc.bound(ref, PIECE, LANES)
    # a continuation piece shorter than k is no short read, and has no window
    got = dev.score([whole[:k - 1], whole[:k + 3]], t, k, False, total, continues=True)
    assert int(got[1][0]) == 0 and math.isnan(got[0][0]) and int(got[1][1]) == len([w for w in sc.window_ids(whole[:k + 3], k) if w is not None])


@pytest.mark.parametrize("k", [1, 4, 9])
def test_a_first_piece_without_a_scored_window_leaves_the_initial_term_to_the_next(dev, k):
    """A record that begins with Ns (or with fewer than k clean residues) and is cut inside them: no window of the first piece is scored,
    so the first scored window of the continuing piece is the record's first and is weighed against total', not against D(w).
    KDB_SCORE_NONE_SCORED says so; without it the join is off by ln D(w) - ln total', far outside the bound.  (Found by the seeded
    run of tests/fuzz_records.py: seed 202, case 11 of the score call.)"""
    from kmerdb_amd import _abi, probability
    rng = np.random.default_rng(190 + k)
    body = sc.random_record(rng, PIECE + 300, p_n=0.001)
    v, total = sc.forward_profile([body], k)
    t = dev.upload(v)
    other = sc.random_record(rng, k + 20)
    for head, cut in [(b"N" * 50, 30), (b"N" * 50, 50 + k - 1), (body[:k - 1] + b"N", k), (b"N" * (2 * k), k)]:
        whole = head + body
        ref = sc.score_record(whole, v, k, False, total)
        assert all(w is None for w in sc.window_ids(whole[:cut], k)) and ref.windows > PIECE and math.isfinite(float(ref.log10_p))
        first = dev.score([other, whole[:cut]], t, k, False, total)
        assert int(first[1][1]) == 0 and math.isnan(first[0][1])
        piece = whole[cut - (k - 1):]
        got = probability.score_reads(*sc.pack([piece, other]), t, k, False, total, continues=True, none_scored=True)
        assert (int(got[1][0]), int(got[2][0]), int(got[3][0])) == (ref.windows, ref.zero_windows, ref.min_count)
        assert sc.error(got[0][0], ref) <= sc.bound(ref, PIECE, LANES, joins=1), (cut, len(head))
        plain = dev.score([piece, other], t, k, False, total, continues=True)                # every window a transition: another number
        assert int(plain[1][0]) == ref.windows
        assert k == 1 or sc.error(plain[0][0], ref) > 100 * sc.bound(ref, PIECE, LANES, joins=1)          # (at k = 1 D(w) is total')
        assert got[0][1] == plain[0][1] == dev.score([other], t, k, False, total)[0][0]       # (only record 0 is concerned)
    # a piece shorter than k stays exempt from the length check under both flags; the new flag alone is refused
    got = probability.score_reads(*sc.pack([body[:k - 1], body[:k + 3]]), t, k, False, total, continues=True, none_scored=True)
    assert int(got[1][0]) == 0 and math.isnan(got[0][0])
    bases, offsets = sc.pack([body[:k + 5]])
    ok = dict(ptr=t.data_ptr(), k=k, canonical=0, total=total, a=0, bases=bases, offsets=offsets)
    assert dev.raw(flags=_abi.KDB_SCORE_NONE_SCORED, **ok) == dev.ARG and dev.raw(flags=_abi.KDB_SCORE_CONTINUES | _abi.KDB_SCORE_NONE_SCORED, **ok) == dev.OK
    with pytest.raises(ValueError):
        probability.score_reads(bases, offsets, t, k, False, total, none_scored=True)


def test_score_file_joins_a_record_that_begins_with_more_n_than_a_reader_block_holds(dev, tmp_path):
    from kmerdb_amd import fileutil, probability
    import ids_cases
    k = 6
    rng = np.random.default_rng(18)
    records = [("n_first", b"N" * 150000 + sc.random_record(rng, 50000, p_n=0.0005)), ("short", sc.random_record(rng, 300)),
               ("n_then_short", b"N" * 70000 + sc.random_record(rng, 40))]
    fa = str(tmp_path / "n_first.fa")
    ids_cases.write_fasta(fa, [(n, s.decode()) for n, s in records])
    v, total = sc.forward_profile([s for _, s in records], k)
    md = {"version": fileutil.VERSION, "metadata_blocks": 1, "k": k, "total_kmers": total, "unique_kmers": int(np.count_nonzero(v)), "unique_nullomers": 0,
          "sorted": False, "tags": [], "files": []}
    kdb = str(tmp_path / ("n_first.%d.kdb" % k))
    fileutil.write_kdb(kdb, md, v)
    rows = list(probability.score_file(fa, kdb, block_bytes=1 << 16))        # the Ns of the first record fill two blocks and more
    one_block = list(probability.score_file(fa, kdb))
    assert [r[0] for r in rows] == [n for n, _ in records] and [r[1] for r in rows] == [len(s) for _, s in records]
    for row, whole, (_, s) in zip(rows, one_block, records):
        ref = sc.score_record(s, v, k, False, total)
        assert row[2:5] == whole[2:5] == (ref.windows, ref.zero_windows, ref.min_count) and ref.windows > 0
        assert sc.error(row[5], ref) <= sc.bound(ref, PIECE, LANES, joins=len(s) // (1 << 16) + 1)
        assert sc.error(whole[5], ref) <= sc.bound(ref, PIECE, LANES)


def test_score_file_joins_a_fasta_record_longer_than_a_reader_block(dev, tmp_path):
    from kmerdb_amd import fileutil, probability
    import ids_cases
    k = 6
    rng = np.random.default_rng(17)
    records = [("long", sc.random_record(rng, 200000, p_n=0.0005)), ("short", sc.random_record(rng, 300)), ("tail", sc.random_record(rng, 70000))]
    fa = str(tmp_path / "long.fa")
    ids_cases.write_fasta(fa, [(n, s.decode()) for n, s in records])
    v, total = sc.forward_profile([s for _, s in records], k)
    md = {"version": fileutil.VERSION, "metadata_blocks": 1, "k": k, "total_kmers": total, "unique_kmers": int(np.count_nonzero(v)), "unique_nullomers": 0,
          "sorted": False, "tags": [], "files": []}
    kdb = str(tmp_path / ("long.%d.kdb" % k))
    fileutil.write_kdb(kdb, md, v)
    rows = list(probability.score_file(fa, kdb, block_bytes=1 << 16))        # the long record spans four blocks
    assert [r[0] for r in rows] == ["long", "short", "tail"] and [r[1] for r in rows] == [len(s) for _, s in records]
    for row, (_, s) in zip(rows, records):
        ref = sc.score_record(s, v, k, False, total)
        assert row[2:5] == (ref.windows, ref.zero_windows, ref.min_count)
        assert sc.error(row[5], ref) <= sc.bound(ref, PIECE, LANES, joins=len(s) // (1 << 16) + 1)
        assert row[6] == probability.log_odds_ratio(row[5], k)
    assert rows == list(probability.score_file(fa, kdb, block_bytes=1 << 16))
    one_block = list(probability.score_file(fa, kdb))
    assert [r[:5] for r in one_block] == [r[:5] for r in rows]
    assert all(abs(x[5] - y[5]) <= 1e-9 * abs(x[5]) for x, y in zip(one_block, rows))


# ---- refusals ----

def test_refusals(dev):
    k = 3
    v = np.arange(1, 65, dtype=np.uint64)
    t = dev.upload(v)
    p, total = t.data_ptr(), int(v.sum())
    bases, offsets = sc.pack([b"ACGTAC", b"GGTAN", b"TTT"])
    ok = dict(ptr=p, k=k, canonical=0, total=total, a=0, bases=bases, offsets=offsets)

    def raw(**kw):
        return dev.raw(**dict(ok, **kw))

    assert raw() == dev.OK and raw(canonical=1, a=5, flags=1) == dev.OK
    for kw in ({"k": 0}, {"k": 18}, {"k": -1}, {"ptr": 0}, {"ptr": p + 8}, {"total": 0}, {"total": TOP - 63, "a": 1}, {"total": 1, "a": 2 ** 62},
               {"null": ("bases",)}, {"null": ("offsets",)}, {"null": (0,)}, {"null": (1,)}, {"null": (2,)}, {"null": (3,)}, {"flags": 2}, {"flags": 4},
               {"offsets": np.array([1, 6, 11, 14], dtype=np.uint64)}, {"offsets": np.array([0, 6, 11, 13], dtype=np.uint64)},
               {"offsets": np.array([0, 11, 6, 14], dtype=np.uint64)}, {"offsets": np.array([0, 6, 15, 14], dtype=np.uint64)},
               {"nbytes": 2 ** 30 + 1, "offsets": np.array([0, 2 ** 30 + 1], dtype=np.uint64)}):
        assert raw(**kw) == dev.ARG, kw
    assert raw(total=TOP - 64, a=1) == dev.OK and raw(total=1, a=2 ** 62 - 1, k=1, ptr=p) == dev.OK
    for recs in ([b"ACGTAC", b"GG"], [b"AC", b"GGTA"], [b"ACGT", b""]):
        b2, o2 = sc.pack(recs)
        assert raw(bases=b2, offsets=o2) == dev.SHORT, recs
    b2, o2 = sc.pack([b"AC", b"GGTA"])
    assert raw(bases=b2, offsets=o2, flags=1) == dev.OK                      # record 0 continues: exempt from the length check
    b2, o2 = sc.pack([b"GGTA", b"AC"])
    assert raw(bases=b2, offsets=o2, flags=1) == dev.SHORT                   # (only record 0 is)
    for recs in ([b"ACGTXC"], [b"ACGTAC", b"acgt"], [b"ACG\xc1AC"], [b"ACRTAC"], [b"ACGTAC" * 20 + b"-"]):
        b2, o2 = sc.pack(recs)
        assert raw(bases=b2, offsets=o2) == dev.BAD, recs
    b2, o2 = sc.pack([b"ACGTANRNACG", b"RNACGT"])                            # an IUPAC code that an N shields from every window: the engine counts such a record
    assert raw(bases=b2, offsets=o2) == dev.OK
    from kmerdb_amd.engine import IdsEngine
    with IdsEngine(k, canonicalize=False) as e:
        assert int(np.count_nonzero(e.window_ids(b2, o2) != NO_WINDOW)) == 4 + 2
        with pytest.raises(ValueError):
            e.window_ids(*sc.pack([b"ACRTAC"]))
    from kmerdb_amd import probability
    with pytest.raises(ValueError):
        probability.score_reads(*sc.pack([b"ACGTAC", b"GG"]), t, k, False, total)
    with pytest.raises(ValueError):
        probability.score_reads(*sc.pack([b"ACGTXC"]), t, k, False, total)


# ---- the layers ----

def test_markov_probability_and_the_subcommand(dev, tmp_path, capsys):
    from kmerdb_amd import fileutil, probability, profile
    import ids_cases
    k = 5
    reads = ids_cases.graph_records("ragged")[:8]
    fq = str(tmp_path / "reads.fq")
    ids_cases.write_fastq(fq, reads)
    seqs = [s.encode() for _, s in reads]
    for canonical in (False, True):
        v, total = (sc.canonical_profile if canonical else sc.forward_profile)(seqs, k)
        md = {"version": fileutil.VERSION, "metadata_blocks": 1, "k": k, "total_kmers": total, "unique_kmers": int(np.count_nonzero(v)), "unique_nullomers": 0,
              "sorted": False, "tags": [], "files": []}
        kdb = str(tmp_path / ("c" if canonical else "f") / "reads.5.kdb")
        os.makedirs(os.path.dirname(kdb))
        fileutil.write_kdb(kdb, md, v)
        t = dev.upload(v)
        rows = list(probability.score_file(fq, kdb))
        direct = dev.score(seqs, t, k, canonical, total)
        assert [r[0] for r in rows] == [n for n, _ in reads] and [r[1] for r in rows] == [len(s) for s in seqs]
        assert [r[5] for r in rows] == direct[0].tolist() and [r[2] for r in rows] == direct[1].tolist()
        assert all(math.isfinite(r[5]) and r[6] == probability.log_odds_ratio(r[5], k) > 0 for r in rows)
        # markov_probability on a string is score_reads on it; a reader object serves as well as a path; a record with .seq as a string
        name, s = reads[3]
        got = probability.markov_probability(s, kdb)
        assert got["log10_p"] == rows[3][5] and got["log_odds_ratio"] == rows[3][6] and got["seq"] == s
        assert got["p_of_seq"] == 10.0 ** rows[3][5]

        class Record:
            seq = s
        rdr = fileutil.open(kdb, slurp=True)
        assert probability.markov_probability(Record(), rdr)["log10_p"] == rows[3][5]
        absent = sc.id_kmer(int(np.flatnonzero((sc.symmetrised(v, k) if canonical else v) == 0)[0]), k)
        with pytest.raises(ValueError, match="math domain error"):
            probability.markov_probability(s + absent, kdb)
        assert math.isfinite(probability.markov_probability(s + absent, kdb, pseudocount=1)["log10_p"])
        with pytest.raises(ValueError):
            probability.markov_probability("N" * 20, kdb)
        # `python -m kmerdb_amd probability ...` is sys.exit(profile.main()): the same parser and dispatch, in this process
        capsys.readouterr()
        assert profile.main(["probability", fq, kdb]) == 0
        text = capsys.readouterr().out
        assert text == "\t".join(probability.COLUMNS) + "\n" + "".join(probability.format_row(r) for r in rows)
        out = io.StringIO()
        assert probability.probabilities(fq, kdb, pseudocount=1, output_delimiter=",", out=out) == len(rows)
        lines = out.getvalue().splitlines()
        assert lines[0] == ",".join(probability.COLUMNS) and lines[4].split(",")[5] == repr(probability.markov_probability(s, kdb, pseudocount=1)["log10_p"])
