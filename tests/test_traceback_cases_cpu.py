"""CPU: the restatement of kdb_align_traceback (tests/traceback_cases.py) against what its definition promises -- the walk ends at
alignment_cases.banded's origin, the runs consume the two spans and add up to the score, the banded form equals the full-matrix form
where the band covers the matrix -- on seeded random cases and on cases worked by hand; and kmerdb_amd.alignment's cigar_string and
cigar_nm on fixed inputs.  The GPU tests compare the device with this restatement, so what is checked here is what they stand on."""
import numpy as np
import pytest

import alignment_cases as ac
import traceback_cases as tc

SCORINGS = [ac.DEFAULT, dict(match=1, mismatch=0, gap_open=0, gap_extend=0), dict(match=2, mismatch=-1, gap_open=-1, gap_extend=-3),
            dict(match=127, mismatch=-127, gap_open=-127, gap_extend=-127), dict(match=2, mismatch=-1, gap_open=-2, gap_extend=-1)]
ALPHABETS = [b"ACGT", b"AC", b"A", b"ACGTN"]
BANDS = [1, 2, 5, 16]
NCASES, SEED = 2400, 20261021


def _random(rng, alphabet, n):
    return bytes(alphabet[int(x)] for x in rng.integers(0, len(alphabet), size=n))


def _cases():
    """(q, r, d, band, strand, scores): the partner is a mutated copy of what aligns (two thirds) or unrelated"""
    rng = np.random.Generator(np.random.PCG64(SEED))
    for x in range(NCASES):
        alphabet, band, scores, strand = ALPHABETS[x % 4], BANDS[(x // 4) % 4], SCORINGS[(x // 16) % 5], (x // 80) % 2
        q = _random(rng, alphabet, int(rng.integers(0, 41)))
        if x % 3:
            r = ac.mutate(rng, ac.orient(q, strand), 0.06, 0.08)
            r = _random(rng, alphabet, int(rng.integers(0, 4))) + r + _random(rng, alphabet, int(rng.integers(0, 4)))
        else:
            r = _random(rng, alphabet, int(rng.integers(0, 41)))
        yield q, r, int(rng.integers(-3, 6)), band, strand, scores


@pytest.fixture(scope="module")
def traced():
    return [(case, tc.trace(*case[:5], **case[5])) for case in _cases()]


def test_the_walk_ends_at_the_origin_and_the_runs_add_up(traced):
    assert len(traced) >= 2000
    for (q, r, d, band, strand, scores), (out, runs) in traced:
        assert out == ac.banded(q, r, d, band, strand, **scores), (q, r, d, band, strand, scores)   # (the origin: where the walk stopped)
        score, qstart, qend, rstart, rend = out
        assert tc.spans(runs) == (qend - qstart, rend - rstart) and tc.rescore(runs, **scores) == score, (q, r, d, band, strand, scores, tc.text(runs))
        assert len(runs) <= (qend - qstart) + (rend - rstart) and (score > 0) == bool(runs)
        assert all(int(a) & 15 != int(b) & 15 for a, b in zip(runs, runs[1:])) and all(int(x) >> 4 >= 1 for x in runs)
        if runs:
            assert runs[0] & 15 in (tc.OP_EQ, tc.OP_X) and runs[-1] & 15 in (tc.OP_EQ, tc.OP_X)


def test_the_cases_bite(traced):
    """the restatement alone, on these seeds: most cases align, every op occurs, many paths hold more than one gap"""
    ops = {int(x) & 15 for _, (_, runs) in traced for x in runs}
    assert ops == {tc.OP_I, tc.OP_D, tc.OP_EQ, tc.OP_X}
    assert sum(1 for _, (out, _) in traced if out[0] > 0) >= len(traced) // 2
    gaps = lambda runs: sum(1 for x in runs if int(x) & 15 in (tc.OP_I, tc.OP_D))
    assert sum(1 for _, (_, runs) in traced if gaps(runs) >= 2) >= 100
    for scores in SCORINGS:
        assert sum(1 for case, (_, runs) in traced if case[5] is scores and gaps(runs) >= 1) >= 20, scores
    for strand in (0, 1):
        assert sum(1 for case, (_, runs) in traced if case[4] == strand and gaps(runs) >= 1) >= 100


def test_the_banded_form_is_the_full_matrix_where_the_band_covers_it(traced):
    n = 0
    for (q, r, d, band, strand, scores), got in traced:
        m, k = len(q), len(r)
        if m and k and -(m - 1) >= d - band and k - 1 <= d + band:             # every j - i of the matrix lies inside the band
            full = tc.trace_full(ac.orient(q, strand), r, **scores)
            assert full[0] == ac.unbanded(ac.orient(q, strand), r, **scores) and got == full, (q, r, d, band, strand, scores)
            n += 1
    assert n >= 50
    # and on longer pairs, with a band that is made to cover them
    rng = np.random.Generator(np.random.PCG64(SEED + 1))
    gaps = 0
    for x in range(150):
        q = _random(rng, ALPHABETS[x % 4], int(rng.integers(1, 31)))
        r = ac.mutate(rng, q, 0.08, 0.1) or b"A"
        scores = SCORINGS[x % 5]
        got = tc.trace(q, r, 0, 40, 0, **scores)
        assert got == tc.trace_full(q, r, **scores), (q, r, scores)
        gaps += any(int(v) & 15 in (tc.OP_I, tc.OP_D) for v in got[1])
    assert gaps >= 30


CHEAP = dict(match=3, mismatch=-1, gap_open=-2, gap_extend=-1)


def test_cases_worked_by_hand():
    t = lambda q, r, d=0, band=4, strand=0, **scores: (lambda out: (out[0], tc.text(out[1])))(tc.trace(q, r, d, band, strand, **scores))
    # one mismatch: 7 matches and a mismatch beat the 4 matches behind it
    assert t(b"ACGTACGT", b"ACGAACGT") == ((20, 0, 8, 0, 8), "3=1X4=")
    # one insertion: a T the reference lacks, between a C and a G (no neighbour equals it: one placement)
    assert t(b"ACGACGAC" + b"T" + b"GGACCAGG", b"ACGACGACGGACCAGG", **CHEAP) == ((16 * 3 - 2, 0, 17, 0, 16), "8=1I8=")
    # one deletion: the same with the two roles changed
    assert t(b"ACGACGACGGACCAGG", b"ACGACGAC" + b"T" + b"GGACCAGG", **CHEAP) == ((16 * 3 - 2, 0, 16, 0, 17), "8=1D8=")
    # a gap of 3: an opening and two extensions
    assert t(b"ACGACGAC" + b"GGACCAGG", b"ACGACGAC" + b"TTT" + b"GGACCAGG", **CHEAP) == ((16 * 3 - 2 - 2, 0, 16, 0, 19), "8=3D8=")
    # two gaps, one of either kind, and a mismatch between them
    q, r = b"ACGACGAC" + b"T" + b"GGACCAGG" + b"CATCATCA", b"ACGACGAC" + b"GGACGAGG" + b"TT" + b"CATCATCA"
    assert t(q, r, **CHEAP) == ((23 * 3 - 1 - 2 - 3, 0, 25, 0, 26), "8=1I4=1X3=2D8=")
    # the same pair on the other strand: the oriented query is what aligns
    assert t(ac.orient(q, 1), r, strand=1, **CHEAP) == ((23 * 3 - 1 - 2 - 3, 0, 25, 0, 26), "8=1I4=1X3=2D8=")
    # open > extend: a gap of 2 is two openings at -1, not an opening and an extension at -3; the two abut and read as one run
    dear = dict(match=3, mismatch=-4, gap_open=-1, gap_extend=-3)
    out, runs = tc.trace(b"ACGACGAC" + b"GGACCAGG", b"ACGACGAC" + b"TT" + b"GGACCAGG", 0, 4, 0, **dear)
    assert (out, tc.text(runs)) == ((16 * 3 - 2, 0, 16, 0, 18), "8=2D8=") and tc.rescore(runs, **dear) == 46
    # a local alignment: what does not pay is clipped, and the path starts where H left 0
    assert t(b"TTTT" + b"ACGACGAC" + b"TTTT", b"GGGG" + b"ACGACGAC" + b"GGG", match=3, mismatch=-4, gap_open=-10, gap_extend=-1) == ((24, 4, 12, 4, 12), "8=")
    # an N matches nothing, not even an N
    assert t(b"ACGNACGT", b"ACGNACGT") == ((3 * 7 - 1, 0, 8, 0, 8), "3=1X4=")
    # nothing aligns: no runs
    assert tc.trace(b"AAAA", b"CCCC", 0, 4) == ((0, 0, 0, 0, 0), []) and tc.trace(b"", b"ACGT", 0, 4) == ((0, 0, 0, 0, 0), [])
    assert tc.trace(b"ACGT", b"ACGT", 40, 4) == ((0, 0, 0, 0, 0), [])


def test_cigar_strings():
    from kmerdb_amd import alignment
    run = lambda *pairs: np.array([(n << 4) | op for n, op in pairs], dtype=np.uint32)
    runs = run((8, 7), (1, 1), (4, 7), (1, 8), (3, 7), (2, 2), (8, 7))
    assert alignment.cigar_string(runs, 0, 25, 25, eqx=True) == "8=1I4=1X3=2D8="
    assert alignment.cigar_string(runs, 0, 25, 25) == "8M1I8M2D8M"                 # = and X merge into M, across the X
    assert alignment.cigar_string(runs, 3, 28, 30, eqx=True) == "3S8=1I4=1X3=2D8=2S" and alignment.cigar_string(runs, 3, 28, 30) == "3S8M1I8M2D8M2S"
    assert alignment.cigar_string(runs, 0, 25, 26) == "8M1I8M2D8M1S" and alignment.cigar_string(runs, 1, 26, 26) == "1S8M1I8M2D8M"
    assert alignment.cigar_nm(runs) == 1 + 1 + 2 and alignment.cigar_nm(run((150, 7))) == 0 and alignment.cigar_nm(run()) == 0
    assert alignment.cigar_string(run((150, 7)), 0, 150, 150) == "150M" and alignment.cigar_string(run((150, 7)), 0, 150, 150, eqx=True) == "150="
    assert alignment.cigar_string(run((5, 8), (5, 7)), 0, 10, 10) == "10M" and alignment.cigar_string(list(run((2, 7))), 4, 6, 9) == "4S2M3S"
    # strand 1: the runs come along the oriented (reverse-complemented) query, and so do the clips -- qstart, qend are the oriented ones
    q, r = b"GG" + b"ACGACGAC" + b"T" + b"GGACCAGG" + b"CCC", b"ACGACGACGGACCAGG"
    out, path = tc.trace(ac.orient(q, 1), r, 0, 4, 1, match=3, mismatch=-4, gap_open=-2, gap_extend=-1)
    assert out == (46, 2, 19, 0, 16)
    assert alignment.cigar_string(path, out[1], out[2], len(q)) == "2S8M1I8M3S" and alignment.cigar_nm(path) == 1
    assert alignment.OP_I == tc.OP_I and alignment.OP_D == tc.OP_D and alignment.OP_EQ == tc.OP_EQ and alignment.OP_X == tc.OP_X
