"""CPU: the oracle of tests/score_cases.py against cases worked by hand, its inputs against what tests/test_gpu_score.py needs of them,
and the parts of kmerdb_amd.probability that run before any device call: the argument ladder, the command line's parser, and
log_odds_ratio's identity with the reference's expression (kmerdb/probability.py:137-147)."""
import decimal
import math
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import score_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header_constant(name):
    text = open(os.path.join(ROOT, "include", "kdbhip.h")).read()
    return int(re.search(r"#define\s+%s\s+(\d+)" % name, text).group(1))


PIECE, LANES = _header_constant("KDB_SCORE_PIECE"), _header_constant("KDB_SCORE_LANES")


def _p(score):
    """10 ** log10_p as a Fraction, to 40 digits"""
    with decimal.localcontext(sc.CTX):
        return Fraction(str(round(sc.CTX.power(decimal.Decimal(10), score.log10_p), 40)))


def _close(score, frac):
    return abs(_p(score) - frac) < Fraction(1, 10 ** 38)


# ---- the oracle, by hand ----

def test_k1_is_a_product_of_frequencies():
    v = np.array([1, 2, 3, 4], dtype=np.uint64)                              # A C G T; total 10; at k = 1 every D is the whole vector
    s = sc.score_record(b"ACGT", v, 1, False, 10)
    assert (s.windows, s.zero_windows, s.min_count, s.all_windows) == (4, 0, 1, 4)
    assert _close(s, Fraction(1 * 2 * 3 * 4, 10 ** 4))
    assert s.terms == [(1, 10), (2, 10), (3, 10), (4, 10)]


def test_acgt_at_k2_on_a_stated_vector():
    v = np.arange(1, 17, dtype=np.uint64)                                    # v[i] = i + 1, total 136
    s = sc.score_record(b"ACGT", v, 2, False, 136)
    # AC = 1: 2 / 136;  CG = 6: 7 / (5 + 6 + 7 + 8);  GT = 11: 12 / (9 + 10 + 11 + 12)
    assert s.terms == [(2, 136), (7, 26), (12, 42)]
    assert _close(s, Fraction(2, 136) * Fraction(7, 26) * Fraction(12, 42)) and Fraction(2, 136) * Fraction(7, 26) * Fraction(12, 42) == Fraction(1, 884)
    assert (s.windows, s.zero_windows, s.min_count) == (3, 0, 2)
    # as the next piece of a longer record every window is a transition: AC against AA + AC + AG + AT
    s = sc.score_record(b"ACGT", v, 2, False, 136, continues=True)
    assert s.terms == [(2, 10), (7, 26), (12, 42)] and _close(s, Fraction(1, 65))


def test_acgt_at_k2_on_a_canonical_vector():
    v = np.zeros(16, dtype=np.uint64)
    canonical = [i for i in range(16) if i <= sc.rc_id(i, 2)]
    assert canonical == [0, 1, 2, 3, 4, 5, 6, 8, 9, 12]                      # AA AC AG AT CA CC CG GA GC TA
    for i in canonical:
        v[i] = i + 1
    s = sc.score_record(b"ACGT", v, 2, True, 100)
    # AC -> 1;  CG -> 6, its prefix C: CA 4, CC 5, CG 6, CT -> AG 2;  GT -> AC 1, its prefix G: GA 8, GC 9, GG -> CC 5, GT -> AC 1
    assert s.terms == [(2, 100), (7, 5 + 6 + 7 + 3), (2, 9 + 10 + 6 + 2)]
    assert _close(s, Fraction(1, 2025))
    sym = sc.symmetrised(v, 2)
    assert sc.score_record(b"ACGT", sym, 2, False, 100).terms == s.terms


def test_pseudocount_zero_windows_and_n():
    v = np.array([0, 1, 1, 2], dtype=np.uint64)
    s = sc.score_record(b"AC", v, 1, False, 4, a=1)                          # total' = 8
    assert s.terms == [(1, 8), (2, 8)] and _close(s, Fraction(1, 32)) and (s.zero_windows, s.min_count) == (1, 0)
    s = sc.score_record(b"AC", v, 1, False, 4)
    assert s.log10_p == float("-inf") and s.windows == 2 and s.zero_windows == 1
    assert math.isinf(sc.float64_log10_p(s))
    # the first SCORED window takes the initial term, wherever it lies
    s = sc.score_record(b"NNCG", v, 1, False, 4)
    assert s.terms == [(1, 4), (1, 4)] and (s.windows, s.all_windows) == (2, 4)
    s = sc.score_record(b"ANNA", np.arange(1, 17, dtype=np.uint64), 2, False, 136)
    assert s.log10_p is None and (s.windows, s.zero_windows, s.min_count, s.all_windows) == (0, 0, sc.TOP, 3)
    assert math.isnan(sc.float64_log10_p(s))
    assert sc.window_ids(b"acgt", 2) == [None, None, None]                   # lower case is not a residue the engine counts
    assert sc.rc_id(sc.kmer_id("AAC"), 3) == sc.kmer_id("GTT") and sc.id_kmer(sc.kmer_id("GATTACA"), 7) == "GATTACA"


def test_the_inputs_reach_the_edges_the_gpu_tests_name():
    for k in (1, 2, 3, 8, 12, 13):
        assert [n - k + 1 for n in sc.length_ladder(k, PIECE)] == [1, 2, 63, 64, 65, PIECE - 1, PIECE, PIECE + 1, 2 * PIECE + 1]
        first, last, none, all_n, clean = sc.n_records(k)
        assert first[0:1] == b"N" and last[-1:] == b"N" and b"N" not in clean
        assert all(w is None for w in sc.window_ids(none, k)) and len(sc.window_ids(none, k)) > 3
        assert sc.window_ids(all_n, k) == [None]
    assert PIECE % LANES == 0 and LANES == 64
    assert sc.pieces_of(0, PIECE) == 1 and sc.pieces_of(PIECE, PIECE) == 1 and sc.pieces_of(PIECE + 1, PIECE) == 2


def test_plain_float64_is_inside_the_bound_on_the_accuracy_cases():
    """the bound is not so tight that ordinary float64 arithmetic misses it: numpy's evaluation of the same formula on the same inputs"""
    worst = 0.0
    for name, k, canonical, v, total, a, records in sc.accuracy_cases(PIECE):
        finite = 0
        for r in records:
            s = sc.score_record(r, v, k, canonical, total, a)
            if s.log10_p is None:
                continue
            assert s.log10_p != float("-inf"), (name, r[:40])
            eps = sc.bound(s, PIECE, LANES)
            err = sc.error(sc.float64_log10_p(s), s)
            worst = max(worst, err / eps)
            assert err <= eps, (name, len(r), err, eps)
            finite += 1
        assert finite >= 8, name
    print("worst share of the bound, numpy float64:", worst)
    name, k, _, v, total, _, records = sc.accuracy_cases(PIECE)[-2]
    assert max(d for r in records for _, d in sc.score_record(r, v, k, False, total).terms) == 4 * sc.TOP > 2 ** 65      # D needs 66 bits


# ---- kmerdb_amd.probability before any device call ----

def test_log_odds_ratio_is_the_references_expression():
    from kmerdb_amd import probability

    def reference_lor(log10_px_plus_total, k, length, mononucleotides):
        """probability.py:53, :87, :91-99, :131, :137-147 as written there"""
        N = 4 ** k
        um = 1 / N
        total2 = 0
        total_nucleotides = sum(mononucleotides.values())
        for _ in range(k, length):
            sum_aij = 0
            for char in "ACGT":                                              # neighbors["suffixes"]: one per letter
                sum_aij += mononucleotides[char] / total_nucleotides
            total2 += math.log10(sum_aij)
        null_model = math.log10(um) + total2
        return log10_px_plus_total / null_model

    exact = {"A": 3, "C": 5, "G": 7, "T": 1}                                 # sixteenths: the four quotients add up to 1.0 without rounding
    for k, length, lp in ((1, 4, -2.5), (8, 150, -87.25), (12, 13, -7.0), (17, 1000, -601.5)):
        assert probability.log_odds_ratio(lp, k) == reference_lor(lp, k, length, exact)
        rounded = reference_lor(lp, k, length, {"A": 301, "C": 197, "G": 211, "T": 290})          # the sum may be one ulp off 1
        assert probability.log_odds_ratio(lp, k) == pytest.approx(rounded, rel=1e-12)
    assert probability.log_odds_ratio(-12 * math.log10(4.0), 12) == pytest.approx(1.0, rel=1e-15)  # a uniform profile's own score


def test_the_argument_ladder_is_checked_before_the_device():
    import torch
    from kmerdb_amd import probability
    bases, offsets = sc.pack([b"ACGT", b"GGTA"])
    v = torch.zeros(16, dtype=torch.int64)
    good = dict(bases=bases, offsets=offsets, vector=v, k=2, canonical=False, total=10)

    def call(**kw):
        return probability.score_reads(**dict(good, **kw))

    for kw in ({"k": 2.0}, {"k": True}, {"total": 10.0}, {"pseudocount": 0.5}, {"bases": "ACGTGGTA"}, {"bases": bases.astype(np.int32)},
               {"vector": np.zeros(16, dtype=np.uint64)}, {"vector": None}):
        with pytest.raises(TypeError):
            call(**kw)
    for kw in ({"k": 0}, {"k": 18}, {"total": 0}, {"total": -1}, {"pseudocount": -1}, {"total": 2 ** 64}, {"total": 2 ** 64 - 16, "pseudocount": 1},
               {"pseudocount": 2 ** 62, "k": 1, "vector": torch.zeros(4, dtype=torch.int64)},
               {"offsets": np.array([0, 4], dtype=np.uint64)}, {"offsets": np.array([1, 4, 8], dtype=np.uint64)},
               {"offsets": np.array([0, 5, 4, 8], dtype=np.uint64)}, {"offsets": np.array([], dtype=np.uint64)},
               {"vector": torch.zeros(15, dtype=torch.int64)}, {"vector": torch.zeros(16, dtype=torch.float64)}, {"vector": torch.zeros(16, dtype=torch.int32)},
               {"vector": torch.zeros(32, dtype=torch.int64)[::2]}, {"vector": 0}, {"vector": 4104},
               {"vector": v}):                                               # (a host tensor: there is no CPU fallback)
        with pytest.raises(ValueError):
            call(**kw)
    with pytest.raises(TypeError):
        probability.markov_probability(12, "x.kdb")
    with pytest.raises(TypeError):
        probability.markov_probability("ACGT", 12)
    with pytest.raises(TypeError):
        list(probability.score_file(12, "x.kdb"))
    assert probability.format_row(("r1", 150, 139, 0, 3, -87.25, 1.5), ",") == "r1,150,139,0,3,-87.25,1.5\n"
    assert probability.format_row(("r1", 4, 0, 0, probability.NO_COUNT, float("nan"), float("nan"))) == "r1\t4\t0\t0\t18446744073709551615\tnan\tnan\n"


def test_markov_probability_refuses_a_short_sequence_like_the_reference(tmp_path):
    from kmerdb_amd import fileutil, probability
    k = 3
    v = np.arange(64, dtype=np.uint64)
    md = {"version": fileutil.VERSION, "metadata_blocks": 1, "k": k, "total_kmers": int(v.sum()), "unique_kmers": 63, "unique_nullomers": 1, "sorted": False,
          "tags": [], "files": []}
    p = str(tmp_path / "p.3.kdb")
    fileutil.write_kdb(p, md, v)
    with pytest.raises(ValueError, match="at least k=3"):
        probability.markov_probability("AC", p)                              # probability.py:57-58


def test_a_profile_is_canonical_iff_nothing_lies_above_its_reverse_complement():
    from kmerdb_amd import probability
    records = sc.ragged_records(4, 9)
    fwd, _ = sc.forward_profile(records, 4)
    can, _ = sc.canonical_profile(records, 4)
    assert not probability.profile_is_canonical(fwd, 4) and probability.profile_is_canonical(can, 4)
    assert probability.profile_is_canonical(fwd, 4, {"canonical": True}) and not probability.profile_is_canonical(can, 4, {"canonical": False})
    big = np.zeros(4 ** 13, dtype=np.uint64)                                 # above k = 12 the first occupied bins decide
    big[sc.kmer_id("A" * 12 + "C")] = 1
    assert probability.profile_is_canonical(big, 13)
    big[sc.kmer_id("T" * 13)] = 1
    assert not probability.profile_is_canonical(big, 13)


def test_the_probability_subcommand_parses_the_references_positionals():
    from kmerdb_amd import profile
    ap = profile.build_parser()
    a = ap.parse_args(["probability", "reads.fq.gz", "genome.12.kdb"])
    assert (a.cmd, a.seqfile, a.kdb, a.pseudocount, a.output_delimiter, a.device) == ("probability", "reads.fq.gz", "genome.12.kdb", 0, "\t", 0)
    a = ap.parse_args(["probability", "--pseudocount", "2", "--output-delimiter", ",", "--device", "1", "a.fa", "b.kdb"])
    assert (a.seqfile, a.kdb, a.pseudocount, a.output_delimiter, a.device) == ("a.fa", "b.kdb", 2, ",", 1)
    for bad in (["probability", "reads.fq"], ["probability"], ["probability", "--pseudocount", "x", "a.fa", "b.kdb"]):
        with pytest.raises(SystemExit):
            ap.parse_args(bad)
    assert ap.parse_args(["spectrum", "a.kdb"]).cmd == "spectrum"            # (the other subcommands are where they were)


# ---- the records of the decode's edges (k = 14 .. 17) ----

@pytest.mark.parametrize("k", [14, 15, 16, 17])
def test_decode_edge_records_are_where_they_claim_to_be(k):
    kmers = sc.decode_edge_kmers(k)
    K = kmers["K"]
    ids = {name: sc.kmer_id(x) for name, x in kmers.items()}
    assert len(K) == k and K[-1] == "T" and "T" not in K[-9:-1]
    assert ids["K"] ^ ids["last"] in (1, 2, 3)                               # the last residue alone
    assert (ids["K"] ^ ids["r13"]) >> (2 * (k - 14)) in (1, 2, 3) and (ids["K"] ^ ids["r12"]) >> (2 * (k - 13)) in (1, 2, 3)
    assert (kmers["r13"] == kmers["last"]) == (k == 14) and len(set(ids.values())) == (3 if k == 14 else 4)

    class Sparse:
        def __len__(self):
            return 4 ** k

        def __getitem__(self, i):
            return {ids["K"]: 3, ids["last"]: 8, ids["r13"]: 13 if k > 14 else 8, ids["r12"]: 18}.get(int(i), 0)

    for alignment in range(8):
        records, roles = sc.decode_edge_records(k, alignment)
        bases, offsets = sc.pack(records)
        assert sorted(roles) == sorted(sc.DECODE_EDGE_ROLES) and len(records) == 2 * len(roles)
        assert all(int(offsets[i]) % 8 == alignment for i in roles.values())
        assert roles["ends_buffer"] == len(records) - 1 and int(offsets[-1]) == bases.size == int(offsets[roles["ends_buffer"]]) + k
        assert all(len(records[i - 1]) >= k and b"N" not in records[i - 1] for i in roles.values())
        s = {role: sc.score_record(records[i], Sparse(), k, False, 42, 1) for role, i in roles.items()}
        assert [s[r].windows for r in sc.DECODE_EDGE_ROLES] == [1, 1, 1, 1, 1, 0, 2, 2 * k + 1, 1]
        assert [s[r].min_count for r in ("alone", "last", "r13", "r12", "n_after", "ends_buffer")] == [3, 8, 13 if k > 14 else 8, 18, 3, 3]
        assert s["n_last"].log10_p is None and s["n_after_more"].all_windows == k + 2 and s["inside"].min_count == 0
        # the window starts of `inside` pass through all eight alignments
        assert {(int(offsets[roles["inside"]]) + p) % 8 for p in range(2 * k + 1)} == set(range(8))
