"""CPU: the restatements of tests/alignment_cases.py against each other and against hand-worked cases, and the numpy seeding of
kmerdb_amd.alignment (which needs no device) against its restatement."""
import numpy as np
import pytest

import alignment_cases as ac
import minimizer_cases as mc

X, Y, Z = b"ACGTTGCATGAC", b"TCGCCTGATACG", b"AGT"        # Y occurs nowhere else, shifted or not, with more than a stray match
AFFINE = dict(match=3, mismatch=-1, gap_open=-4, gap_extend=-1)


def _random_pair(rng, alphabet, top=40):
    m, n = int(rng.integers(0, top + 1)), int(rng.integers(0, top + 1))
    letters = np.frombuffer(alphabet, dtype=np.uint8)
    q = letters[rng.integers(0, letters.size, size=m)].tobytes()
    if rng.random() < 0.5 and m:                                              # a relative of q, so that long alignments with gaps occur
        r = ac.mutate(rng, q, 0.1, 0.15)[:top]
    else:
        r = letters[rng.integers(0, letters.size, size=n)].tobytes()
    return q, r


@pytest.mark.parametrize("alphabet,seed", [(b"ACGT", 1), (b"AC", 2), (b"A", 3), (b"ACGTN", 4), (b"AAAC", 5)])
def test_banded_equals_unbanded_where_the_band_covers_the_matrix(alphabet, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    scorings = [ac.DEFAULT, AFFINE, dict(match=2, mismatch=-2, gap_open=-2, gap_extend=-2), dict(match=1, mismatch=0, gap_open=0, gap_extend=0),
                dict(match=5, mismatch=-3, gap_open=-1, gap_extend=-3), dict(match=2, mismatch=-1, gap_open=-3, gap_extend=0)]
    ties = 0
    for case in range(400):
        q, r = _random_pair(rng, alphabet)
        scores = scorings[case % len(scorings)]
        strand = case & 1
        band = max(len(q), len(r), 1) + int(rng.integers(0, 3))
        d = int(rng.integers(-2, 3)) if band > max(len(q), len(r)) + 1 else 0
        want = ac.unbanded(ac.orient(q, strand), r, **scores)
        assert ac.banded(q, r, d, band + abs(d), strand, **scores) == want, (q, r, strand, scores)
        ties += want[0] > 0 and want[2] - want[1] != want[4] - want[3]
    assert ties > 10                                                          # (alignments with gaps are among them)


def test_the_batched_restatement_is_the_plain_one():
    rng = np.random.Generator(np.random.PCG64(6))
    for alphabet, band, scores in [(b"ACGT", 3, ac.DEFAULT), (b"AC", 1, AFFINE), (b"ACGTN", 5, dict(match=1, mismatch=0, gap_open=0, gap_extend=0)),
                                   (b"AAC", 2, dict(match=2, mismatch=-1, gap_open=-1, gap_extend=-2))]:
        pairs = [_random_pair(rng, alphabet, 25) for _ in range(150)]
        queries, refs = [p[0] for p in pairs], [p[1] for p in pairs]
        tasks = [(i, i, int(rng.integers(-6, 7)), int(rng.integers(0, 2))) for i in range(len(pairs))]
        tasks += [(3, 7, 0, 0), (7, 3, 1, 1), (0, 0, 10 ** 12, 0), (0, 0, -10 ** 12, 1)]
        want = ac.run_tasks(queries, refs, tasks, band, **scores)
        got = ac.banded_batch(*mc.pack(queries), *mc.pack(refs), *ac.task_arrays(tasks), band, **scores)
        for name, g, x in zip(("score", "qstart", "qend", "rstart", "rend"), got, want):
            assert g.dtype == x.dtype and g.tolist() == x.tolist(), (alphabet, name)
        assert (want[0] > 0).sum() > 50


# ---- hand-worked ----

def test_exact_match_and_one_mismatch():
    assert ac.banded(b"ACGTACGT", b"ACGTACGT", 0, 2) == (24, 0, 8, 0, 8)                        # 8 x 3
    assert ac.banded(b"ACGTACGT", b"TTACGTACGTTT", 2, 1) == (24, 0, 8, 2, 10)                   # ... on the diagonal 2
    assert ac.banded(b"ACGTACGT", b"TTACGTACGTTT", 0, 1) != (24, 0, 8, 2, 10)                   # ... which a band of 1 around 0 does not hold
    assert ac.banded(b"ACGTACGTAC", b"ACGTTCGTAC", 0, 2) == (26, 0, 10, 0, 10)                  # 9 x 3 - 1: through the mismatch, 12 and 15 on either side
    assert ac.banded(b"ACGTACGTAC", b"ACGTTCGTAC", 0, 2, mismatch=-16) == (15, 5, 10, 5, 10)    # too dear: the longer side alone
    # the reverse complement of the query is what aligns with strand 1; the coordinates are the oriented query's
    assert ac.orient(b"AACGTN", 1) == b"NACGTT"
    assert ac.banded(ac.orient(b"GGACGTACGT", 1), b"TTACGTACGTTT", 2, 2, strand=1) == (24, 2, 10, 2, 10)


def test_gaps_of_one_and_three_with_affine_cost():
    q = X + Y
    assert ac.banded(q, X + Y[1:], 0, 2, **AFFINE) == (65, 0, 24, 0, 23)                        # 12 x 3 - 4 + 11 x 3: one query residue without a partner
    assert ac.banded(q, X + b"A" + Y, 0, 2, **AFFINE) == (68, 0, 24, 0, 25)                     # 24 x 3 - 4: one reference residue without
    assert ac.banded(q, X + Z + Y, 0, 3, **AFFINE) == (66, 0, 24, 0, 27)                        # 72 - (4 + 1 + 1): open once, extend twice
    assert ac.banded(q, X + Z + Y, 0, 3, match=3, mismatch=-1, gap_open=-4, gap_extend=-4) == (60, 0, 24, 0, 27)     # 72 - 3 x 4
    assert ac.banded(X + Z + Y, q, 0, 3, **AFFINE) == (66, 0, 27, 0, 24)                        # the same gap in the other sequence
    assert ac.unbanded(q, X + Z + Y, **AFFINE) == (66, 0, 24, 0, 27)


def test_a_gap_the_band_forbids():
    q, r = X + Y, X + Z + Y
    assert ac.banded(q, r, 0, 2, **AFFINE) == (36, 0, 12, 0, 12)              # the diagonal 3 is outside: X alone
    around_3 = ac.banded(q, r, 3, 2, **AFFINE)                                # around 3 the diagonal 0 is outside: Y alone gives 36, the whole not
    assert 36 <= around_3[0] < 66 and around_3[2] == 24 and around_3[4] == 27
    assert ac.banded(q, r, 1, 2, **AFFINE) == ac.banded(q, r, 2, 2, **AFFINE) == (66, 0, 24, 0, 27)      # both inside
    assert ac.banded(q, r, 6, 2, **AFFINE)[0] < 12 and ac.banded(q, r, 40, 2, **AFFINE) == (0, 0, 0, 0, 0)


def test_n_matches_nothing():
    assert ac.banded(b"ACGNACG", b"ACGNACG", 0, 2) == (17, 0, 7, 0, 7)                          # 9 - 1 + 9
    assert ac.banded(b"NNNN", b"NNNN", 0, 2) == (0, 0, 0, 0, 0)
    assert ac.banded(b"ACGNACG", b"ACGNACG", 0, 2, mismatch=-10) == (9, 0, 3, 0, 3)             # the first of two equal segments
    assert ac.unbanded(b"ACGNACG", b"ACGNACG") == (17, 0, 7, 0, 7)


def test_ties():
    # two equal segments: the smaller i wins; on one row the smaller j
    assert ac.banded(b"ACGTTTTTACG", b"ACGAAAAAACG", 0, 1, mismatch=-5) == (9, 0, 3, 0, 3)
    assert ac.banded(b"ACG", b"ACGTACG", 2, 4) == ac.unbanded(b"ACG", b"ACGTACG") == (9, 0, 3, 0, 3)
    # poly-A: the best cell is the last of the main diagonal, its origin the first
    assert ac.banded(b"A" * 9, b"A" * 9, 0, 3) == (27, 0, 9, 0, 9)
    # an origin tie between the diagonal and a gap: the diagonal is asked first.  AA against AAA, all costs 0 but match 1: H(1, 2) = 2 is
    # reached by the diagonal from H(0, 1) = 1, which began at (0, 1), and by E from H(1, 1) = 2, which began at (0, 0)
    free = dict(match=1, mismatch=0, gap_open=0, gap_extend=0)
    assert ac.banded(b"AA", b"AAA", 0, 3, **free) == ac.unbanded(b"AA", b"AAA", **free) == (2, 0, 2, 0, 2)
    assert ac.banded(b"AA", b"TAA", 0, 3, **free) == (2, 0, 2, 1, 3)
    assert ac.banded(b"ACAC", b"ACACAC", 0, 3, **free) == ac.unbanded(b"ACAC", b"ACACAC", **free)


# ---- the seeding ----

K, BAND, M = 5, 3, 50
TABLE = {7: [(0, 110, 0)], 8: [(0, 121, 0)],                                 # -> ref 0, rel 0, diagonals 100 and 101: one bin (25)
         9: [(0, 200, 0)],                                                    # with query strand 1: rel 1, at 50 - 5 - 30 = 15, diagonal 185: alone
         11: [(1, 1, 1)], 12: [(1, 6, 1)], 13: [(1, 9, 1)],                   # rel 1 with query strand 0: diagonals -4, -1 (bin -1) and 0 (bin 0)
         20: [(0, 300, 0), (1, 300, 0), (1, 400, 1)],                         # three occurrences
         21: [(2, 64, 0)], 22: [(2, 74, 0)], 23: [(2, 85, 0)]}                # ref 2: diagonals 60, 60, 61 -> lower median 60
QMINS = [(10, 7, 0), (20, 8, 0), (30, 9, 1), (40, 11, 0), (38, 12, 0), (36, 13, 0), (2, 20, 0), (4, 21, 0), (14, 22, 0), (24, 23, 0)]


def test_seeding_by_hand():
    table = ac.drop_frequent(TABLE, 2)
    assert 20 not in table and len(table) == len(TABLE) - 1
    cands = ac.seed_hits(table, M, K, QMINS, BAND)
    # three hits before two; of the two with two hits the smaller ref; the diagonals 185 and 0 stand alone and are no candidates
    assert cands == [(2, 0, 60, 3), (0, 0, 100, 2), (1, 1, -4, 2)]
    assert ac.seed_hits(table, M, K, QMINS, BAND, max_candidates=2) == cands[:2]
    assert ac.seed_hits(table, M, K, QMINS, BAND, min_seeds=3) == cands[:1]
    assert ac.seed_hits(table, M, K, QMINS, BAND, min_seeds=1, max_candidates=9)[3:] == [(0, 1, 185, 1), (1, 1, 0, 1)]
    with_20 = ac.seed_hits(ac.drop_frequent(TABLE, 3), M, K, QMINS, BAND, min_seeds=1, max_candidates=9)
    assert (0, 0, 298, 1) in with_20 and (1, 0, 298, 1) in with_20 and (1, 1, 357, 1) in with_20          # 300 - 2; rel 1: 400 - (50 - 5 - 2)
    # a wider band: bins of 8 -- -4 and -1 and 0 are in two bins still (-1 and 0), 100 and 101 in one
    assert ac.seed_hits(table, M, K, QMINS, 7)[1:] == [(0, 0, 100, 2), (1, 1, -4, 2)]


def test_finishing_by_hand():
    cands = [(2, 0, 60, 3), (0, 0, 100, 2), (1, 1, -4, 2), (1, 1, 0, 2), (0, 0, 104, 2)]
    outs = [(90, 0, 50, 60, 110), (120, 5, 50, 105, 150), (30, 10, 30, 6, 26), (30, 10, 30, 6, 26), (0, 0, 0, 0, 0)]
    found = ac.finish(M, cands, outs)
    # by score; rel 1 turns the query coordinates round: [10, 30) of the oriented query is [20, 40) of the record; the second (1, 1) repeats the first
    assert found == [(5, 50, 0, 0, 105, 150, 120, 2, 100), (0, 50, 0, 2, 60, 110, 90, 3, 60), (20, 40, 1, 1, 6, 26, 30, 2, -4)]
    assert ac.finish(M, cands, outs, min_score=90) == found[:2] and ac.finish(M, cands, outs, min_score=121) == []


def _product_candidates(refs, queries, k, w, order, band, **kw):
    """kmerdb_amd.alignment's numpy seeding on restated sketches -> per query [(ref, rel, diag, seeds), ..]"""
    from kmerdb_amd import alignment
    max_occ = kw.pop("max_occ", 50)
    sketch = alignment.build_sketch(*mc.batch_minimizers(refs, k, w, True, order), max_occ)
    counts, ids, pos, strand = mc.batch_minimizers(queries, k, w, True, order)
    tq, tr, diag, rel, seeds = alignment.seed_tasks(sketch, [len(q) for q in queries], counts, ids, pos, strand, k, band, **kw)
    assert tq.dtype == tr.dtype == np.uint32 and diag.dtype == np.int64 and rel.dtype == np.uint8
    out = [[] for _ in queries]
    for q, r, d, s, n in zip(tq.tolist(), tr.tolist(), diag.tolist(), rel.tolist(), seeds.tolist()):
        out[q].append((r, s, d, n))
    return out, (tq, tr, diag, rel, seeds)


@pytest.mark.parametrize("k,w,order,band,kw", [(7, 4, mc.HASHED, 8, {}), (5, 3, mc.LEX, 2, dict(max_occ=3, min_seeds=1, max_candidates=3)),
                                               (9, 5, mc.HASHED, 16, dict(min_seeds=3, max_candidates=1))])
def test_the_products_seeding_is_the_restatement(k, w, order, band, kw):
    from kmerdb_amd import alignment
    rng = np.random.Generator(np.random.PCG64(k))
    refs = [mc.random_record(rng, 1500, 0.002), mc.random_record(rng, 900), b"ACGTTGCA" * 40]
    refs[1] = refs[1][:400] + refs[0][300:600] + refs[1][400:]                # a repeat between two records
    queries = []
    for i in range(60):
        ref = refs[i % 3]
        a = int(rng.integers(0, len(ref) - 130))
        read = ac.mutate(rng, ref[a:a + int(rng.integers(60, 130))], 0.02, 0.01)
        queries.append(ac.orient(read, 1) if i & 1 else read)
    queries += [mc.random_record(rng, 80), b"", b"ACG", mc.random_record(rng, 40) + refs[0][:90]]       # (the last hangs over the record's start: diagonal -40)
    table = ac.sketch(refs, k, w, order, kw.get("max_occ", 50))
    seeding = {key: v for key, v in kw.items() if key != "max_occ"}
    want = [ac.seed(table, q, k, w, order, band, **seeding) for q in queries]
    got, tasks = _product_candidates(refs, queries, k, w, order, band, **kw)
    assert got == want and sum(len(x) for x in want) >= 30
    assert any(rel for c in want for _, rel, _, _ in c) and any(d < 0 for c in want for _, _, d, _ in c)
    # ... and its last step, on the restatement's alignments
    outs = ac.run_tasks(queries, refs, [(q, r, d, s) for q, r, d, s in zip(*(x.tolist() for x in tasks[:4]))], band)
    results = alignment.finish_tasks(len(queries), [len(q) for q in queries], tasks, outs, 0)
    at = 0
    for q, cands in enumerate(want):
        mine = [tuple(int(col[t]) for col in outs) for t in range(at, at + len(cands))]
        assert results[q] == ac.finish(len(queries[q]), cands, mine), q
        at += len(cands)
