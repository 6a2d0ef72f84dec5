"""CPU: the host side of the per-record k-mer tables (kmerdb_amd.composition, kmerdb_amd.codons) with the numpy restatement of
tests/tables_cases.py in the device call's place, against the reference's own results in tests/golden/codons.json
(tests/golden/make_golden_codons.py).

The restatement at k = 3, stride 3, canonical ids is the device's part of the reference's codon functions; the rules that turn its five
outputs into the reference's counts, flags and exceptions are kmerdb_amd.codons' and are what is tested here.  chisq is compared within
64 x 2^-53 relative of the exactly evaluated formula: 61 non-negative terms of three float64 operations each (a difference, a square, a
quotient: 3 roundings, each 2^-53 relative, on terms that are all >= 0 so that nothing cancels in the sum) and at most 60 additions --
a derived bound, not a measured one."""
import io
import json
import math
import os

import numpy as np
import pytest

import tables_cases as tc
from tables_cases import read_fasta, write_fasta

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
CDS = os.path.join(GOLDEN, "inputs", "cds.fa")


@pytest.fixture(scope="module")
def golden():
    return json.load(open(os.path.join(GOLDEN, "codons.json")))


@pytest.fixture(scope="module")
def sequences():
    return dict(read_fasta(CDS))


@pytest.fixture()
def stubbed(monkeypatch):
    """kmerdb_amd.codons and .composition with the restatement where the device call is"""
    from kmerdb_amd import codons, composition
    monkeypatch.setattr(composition, "record_tables", tc.record_tables_stub)
    return codons, composition


def same_floats(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(np.all((a == b) | (np.isnan(a) & np.isnan(b))))


def test_cds_fa_is_the_file_the_golden_script_describes(golden, sequences):
    assert [c["id"] for c in golden["records"]] == [rid for rid, _ in read_fasta(CDS)]
    assert all(len(sequences[c["id"]]) == c["length"] for c in golden["records"])
    assert {3, 6, 7, 3000} <= {c["length"] for c in golden["records"]} and os.path.getsize(CDS) < 16384
    assert max(len(line) for line in open(CDS)) <= 61 and sum(1 for line in open(CDS)) > 2 * len(golden["records"])


def test_restatement_and_host_rules_reproduce_the_reference_list(golden, sequences):
    from kmerdb_amd import codons
    seen = set()
    for c in golden["records"]:
        s, g = sequences[c["id"]], c["get_codons_in_order"]
        row, windows, skipped, first_id, last_id = tc.record_table(s.encode(), 3, 3, canonical=True)
        if g["raises"]:
            assert g["raises"] == "ValueError" and len(s) % 3 != 0
            with pytest.raises(ValueError):
                codons.check_triplet_count(c["id"], len(s), skipped)
            seen.add("length")
            continue
        ids, flag = g["value"]
        assert (windows, skipped) == (len(ids), len(s) // 3 - len(ids)), c["id"]
        assert (first_id, last_id) == ((ids[0], ids[-1]) if ids else (-1, -1)), c["id"]
        assert row.tolist() == np.bincount(ids, minlength=64).tolist(), c["id"]
        assert codons.is_non_canonical(windows, skipped, first_id, last_id) is flag, c["id"]
        seen.add(("flag", flag, skipped))
    assert "length" in seen and {("flag", False, 0), ("flag", True, 0), ("flag", True, 1), ("flag", True, 2), ("flag", True, 3)} <= seen


@pytest.mark.parametrize("canonical", [False, True])
@pytest.mark.parametrize("k,stride", [(1, 1), (2, 1), (3, 3), (4, 2), (6, 1), (6, 6)])
def test_uniform_tables_equals_the_per_record_restatement(k, stride, canonical):
    """tc.uniform_tables, the vectorised form the GPU tests use for thousands of records of one length, against tc.record_table"""
    rng = np.random.Generator(np.random.PCG64(1000 * k + 10 * stride + canonical))
    for length in (0, k - 1, k, k + stride, 37, 64):
        recs = [tc.random_record(rng, length, p) for p in (0.0, 0.0, 0.05, 0.3, 0.3)] + [b"N" * length, b"T" * length]
        if length >= 2 * k + 1:
            recs += [b"N" * k + recs[0][k:], recs[1][:-k] + b"N" * k, b"N" * (length - k) + recs[0][:k]]      # no first window, no last one, only the last
        block = np.frombuffer(b"".join(recs), dtype=np.uint8).reshape(len(recs), length)
        got, want = tc.uniform_tables(block, k, stride, canonical), tc.batch_tables(recs, k, stride, canonical)
        for g, x in zip(got, want):
            assert g.dtype == x.dtype and g.shape == x.shape and g.tobytes() == x.tobytes(), (length, g.tolist(), x.tolist())
    with pytest.raises(ValueError):
        tc.uniform_tables(np.frombuffer(b"ACGTRACG", dtype=np.uint8).reshape(2, 4), 2)


def test_codon_frequency_table_as_reference_equals_the_reference(golden, sequences, stubbed):
    codons, _ = stubbed
    raised = returned = 0
    for c in golden["records"]:
        s = sequences[c["id"]]
        for (start, stop), g in zip(golden["flags"], c["codon_frequency_table"]):
            where = (c["id"], start, stop)
            if g["raises"]:
                with pytest.raises(ValueError):
                    codons.codon_frequency_table(s, c["id"], include_stop_codons=stop, include_start_codons=start, as_reference=True)
                assert g["raises"] == "ValueError", where
                raised += 1
                continue
            ids, counts, wrt_length, in_family = codons.codon_frequency_table(s, c["id"], include_stop_codons=stop, include_start_codons=start, as_reference=True)
            assert ids == g["value"][0] and counts.dtype == np.uint32 and counts.tolist() == g["value"][1], where
            if len(g["value"]) == 4:
                assert same_floats(wrt_length, g["value"][2]) and same_floats(in_family, g["value"][3]), where
            returned += 1
    assert raised >= 9 and returned >= 80


def test_is_sequence_cds_is_the_reference_as_a_plain_bool(golden, sequences, stubbed):
    codons, _ = stubbed

    class Record:
        def __init__(self, rid, seq):
            self.id, self.seq = rid, seq
    verdicts = set()
    for c in golden["records"]:
        for inc, g in zip((False, True), c["is_sequence_cds"]):
            assert g["raises"] is None, c["id"]
            got = codons.is_sequence_cds(Record(c["id"], sequences[c["id"]]), include_noncanonicals=inc, as_reference=True)
            assert got is bool(g["value"]), (c["id"], inc)
            verdicts.add((inc, g["value"]))
    assert verdicts == {(False, True), (False, False), (False, None), (True, True), (True, False), (True, None)}
    with pytest.raises(TypeError):
        codons.is_sequence_cds(17)


def test_constants_equal_the_reference_but_for_serine(golden):
    from kmerdb_amd import codons, kmer
    k = golden["constants"]
    assert {int(i): aa for i, aa in k["codon_table"].items()} == codons.codon_table and len(codons.codon_table) == 64
    assert sorted(k["STOP_CODONS"]) == codons.STOP_CODONS and sorted(k["POSSIBLE_START_CODONS"]) == codons.POSSIBLE_START_CODONS
    assert codons.CODON_LIST == list(range(64))
    ref = {aa: sorted(v) for aa, v in k["synonymous_codons"].items()}
    ours = {aa: sorted(v) for aa, v in codons.synonymous_codons.items()}
    assert ref.pop("S") == codons.REFERENCE_SERINE_FAMILY == [9, 11] and ours.pop("S") == [9, 11, 52, 53, 54, 55]
    # (the reference's arginine entry lacks AGA and AGG, which its codon_table calls R: the same kind of slip, found by the golden data)
    assert ref.pop("R") == codons.REFERENCE_ARGININE_FAMILY == [24, 25, 26, 27] and ours.pop("R") == [8, 10, 24, 25, 26, 27]
    assert ref == ours
    assert {aa: sorted(v) for aa, v in codons._families(True).items()} == {aa: sorted(v) for aa, v in k["synonymous_codons"].items()}
    assert codons._families(False) is codons.synonymous_codons
    # the ids are forward ids: the table's own keys say so
    assert [kmer.id_to_kmer(i, 3) for i in (14, 63, 48, 50, 56)] == ["ATG", "TTT", "TAA", "TAG", "TGA"]
    assert sorted(i for v in codons.synonymous_codons.values() for i in v) == [i for i in range(64) if i not in codons.STOP_CODONS]


@pytest.mark.parametrize("block_bytes", [None, 256])
def test_codon_tables_of_a_file_equal_the_reference_per_flag_combination(golden, sequences, stubbed, tmp_path, block_bytes):
    """through BlockReader: with blocks of 256 bytes the 3 000-residue gene and others arrive in continuation pieces joined on the host"""
    codons, _ = stubbed
    ok = [c for c in golden["records"] if not c["codon_frequency_table"][0]["raises"]]
    path = write_fasta(tmp_path / "ok.fa", [(c["id"], sequences[c["id"]]) for c in ok])
    for f, (start, stop) in enumerate(golden["flags"]):
        ids, counts, flags = codons.codon_tables(path, include_start_codons=start, include_stop_codons=stop, include_noncanonicals=True, as_reference=True,
                                                 block_bytes=block_bytes)
        assert ids == [c["id"] for c in ok] and counts.dtype == np.uint32 and counts.shape == (len(ok), 64)
        assert counts.tolist() == [c["codon_frequency_table"][f]["value"][1] for c in ok]
        assert flags.tolist() == [c["get_codons_in_order"]["value"][1] for c in ok]
    # the refusals, in the reference's order
    everything = write_fasta(tmp_path / "all.fa", [(c["id"], sequences[c["id"]]) for c in golden["records"]])
    with pytest.raises(ValueError, match="non-canonical"):
        codons.codon_tables(everything, as_reference=True, block_bytes=block_bytes)
    with pytest.raises(ValueError, match="n_three"):
        codons.codon_tables(everything, include_noncanonicals=True, ignore_invalid_cds=True, as_reference=True, block_bytes=block_bytes)
    ragged = write_fasta(tmp_path / "ragged.fa", [(c["id"], sequences[c["id"]]) for c in golden["records"] if c["id"] != "n_three"])
    with pytest.raises(ValueError, match="not evenly divisible"):
        codons.codon_tables(ragged, include_noncanonicals=True, as_reference=True, block_bytes=block_bytes)
    assert codons.codon_tables(ragged, include_noncanonicals=True, ignore_invalid_cds=True, as_reference=True, block_bytes=block_bytes)[0] == [c["id"] for c in ok]
    # forward ids: a TAG and a TGA stop and a GTG start are what they are
    plain = write_fasta(tmp_path / "plain.fa", [(i, sequences[i]) for i in ("gene_a", "stop_tag", "stop_tga", "start_gtg", "start_ttg", "long_gene")])
    ids, counts, flags = codons.codon_tables(plain, block_bytes=block_bytes)
    assert not flags.any() and counts.sum(axis=1).tolist() == [len(sequences[i]) // 3 - 2 for i in ids]
    for i, row in zip(ids, counts):
        want = tc.record_table(sequences[i].encode()[3:-3], 3, 3)[0]
        assert row.tolist() == want.tolist(), i


def test_tables_file_joins_pieces_in_frame_at_every_block_size(stubbed, tmp_path):
    _, composition = stubbed
    rng = np.random.Generator(np.random.PCG64(77))
    recs = [("r%d" % i, tc.random_record(rng, n, 0.02).decode()) for i, n in enumerate([5, 700, 1, 64, 1500, 2, 333])]
    for k, stride in [(6, 3), (3, 3), (4, 1), (1, 1), (4, 2), (6, 6)]:
        for bb, wrap in [(64, 60), (100, 7), (257, 80), (None, 60)]:
            path = write_fasta(tmp_path / "x.fa", recs, wrap)
            got = list(composition.tables_file(path, k, stride=stride, canonical=True, block_bytes=bb))
            assert [g[0] for g in got] == [r[0] for r in recs]
            for g, (rid, s) in zip(got, recs):
                row, windows, skipped, first_id, last_id = tc.record_table(s.encode(), k, stride, True)
                assert g[1:6] == (len(s), windows, skipped, first_id, last_id), (k, stride, bb, rid)
                assert g[6].dtype == np.uint64 and g[6].tolist() == row.tolist(), (k, stride, bb, rid)


def test_codons_tsv_is_what_pandas_prints(golden, sequences, stubbed, tmp_path):
    pd = pytest.importorskip("pandas")
    codons, _ = stubbed
    from kmerdb_amd import kmer
    ok = [c for c in golden["records"] if not c["codon_frequency_table"][0]["raises"]]
    path = write_fasta(tmp_path / "ok.fa", [(c["id"], sequences[c["id"]]) for c in ok])
    for as_freq, no_stop, sep in [(False, False, "\t"), (True, False, "\t"), (False, True, ","), (False, False, ";")]:
        data = {}
        for c in ok:                                                          # the reference's loop (its __init__.py:269-299) on its own results
            ids, counts, _, in_family = c["codon_frequency_table"][0]["value"]
            if as_freq:
                data[c["id"]] = in_family
            elif no_stop:
                data[c["id"]] = [counts[i] for i in ids if i not in codons.STOP_CODONS]
            else:
                data[c["id"]] = np.array(counts, dtype=np.uint32)
        names = [kmer.id_to_kmer(i, 3) for i in range(64) if not (no_stop and i in codons.STOP_CODONS)]
        want = io.StringIO()
        pd.DataFrame(data).transpose().to_csv(want, sep=sep, index=True, header=names)
        got = io.StringIO()
        n = codons.codons(path, as_frequencies=as_freq, include_noncanonicals=True, no_stop_codons_in_table=no_stop, output_delimiter=sep, as_reference=True,
                          out=got)
        assert n == len(ok) and got.getvalue() == want.getvalue(), (as_freq, no_stop, sep)
    with pytest.raises(ValueError):
        codons.codons(path, as_frequencies=True, no_stop_codons_in_table=True, include_noncanonicals=True, out=io.StringIO())


def test_expected_frequencies_and_chisq_against_the_golden_script(golden, sequences, stubbed, tmp_path):
    codons, _ = stubbed
    table = np.array(golden["table"], dtype=np.uint32)
    for e in golden["expected"]:
        cnt, freq = codons.get_expected_codon_frequencies(e["L"], table)
        assert cnt.dtype == np.uint32 and cnt.tolist() == e["value"][0] and same_floats(freq, e["value"][1]), e["L"]
    with pytest.raises(TypeError):
        codons.get_expected_codon_frequencies(3.0, table)
    with pytest.raises(ValueError):
        codons.get_expected_codon_frequencies(3, table[:, :61])
    # the table through the `codons` subcommand's text, 64 and 61 columns, then CUB on the same genes
    genes = write_fasta(tmp_path / "genes.fa", [(i, sequences[i]) for i in golden["table_ids"]])
    for no_stop in (False, True):
        text = io.StringIO()
        codons.codons(genes, include_noncanonicals=True, no_stop_codons_in_table=no_stop, out=text)
        tsv = tmp_path / ("table%d.tsv" % no_stop)
        tsv.write_text(text.getvalue())
        ids, back = codons.read_codon_table(str(tsv))
        assert ids == golden["table_ids"] and back.shape == (len(ids), 64) and back.tolist() == table.astype(np.float64).tolist()
        out = io.StringIO()
        results = codons.codon_usage_bias(str(tsv), genes, out=out)
        want = [c for c in golden["cub"] if c["chisq"] is not None]
        assert [r[0] for r in results] == [c["id"] for c in want] and len(want) < len(golden["cub"])
        assert sum(1 for c in want if not math.isnan(c["chisq"])) >= 3 and any(math.isnan(c["chisq"]) for c in want)
        for (rid, chisq, pval), c in zip(results, want):
            assert math.isnan(pval)                                           # ddof = 60 on 61 categories: no degree of freedom
            if math.isnan(c["chisq"]):                                        # (a gene too short for a single expected count: 0 / 0)
                assert math.isnan(chisq), rid
                continue
            print(rid, chisq, c["chisq"], abs(chisq - c["chisq"]) / c["chisq"])
            assert abs(chisq - c["chisq"]) <= 64 * 2.0 ** -53 * c["chisq"], rid
        lines = out.getvalue().splitlines()
        assert lines[0] == "\tchisq\tpval" and lines[1:] == ["{0}\t{1!r}\t{2!r}".format(*r) for r in results]
    scipy_stats = pytest.importorskip("scipy.stats")
    results = codons.codon_usage_bias(str(tsv), genes, ddof=0, out=io.StringIO())
    finite = [(chisq, pval) for _, chisq, pval in results if not math.isnan(chisq)]
    assert len(finite) >= 3
    for chisq, pval in finite:
        assert pval == float(scipy_stats.chi2.sf(chisq, 60)) and 0.0 <= pval <= 1.0


def test_composition_text(stubbed, tmp_path):
    _, composition = stubbed
    from kmerdb_amd import kmer
    recs = [("a", "ACGTACGTNACGTTTT"), ("b", "AC"), ("c", "NNNNNNNN"), ("d", "GATTACAGATTACA" * 9)]
    path = write_fasta(tmp_path / "c.fa", recs, 11)
    for k, canonical, freq in [(4, True, False), (4, True, True), (2, False, False), (3, False, True), (1, True, False)]:
        out = io.StringIO()
        assert composition.composition(path, k, canonical=canonical, as_frequencies=freq, out=out, block_bytes=40) == len(recs)
        lines = [line.split("\t") for line in out.getvalue().splitlines()]
        cols = [i for i in range(4 ** k) if not canonical or i <= int(tc.rc_ids([i], k)[0])]
        assert lines[0] == ["id", "length", "windows"] + [kmer.id_to_kmer(i, k) for i in cols]
        assert (len(cols) == 136) if (k == 4 and canonical) else True
        for line, (rid, s) in zip(lines[1:], recs):
            row, windows, _, _, _ = tc.record_table(s.encode(), k, 1, canonical)
            assert line[:3] == [rid, str(len(s)), str(windows)]
            assert int(row.sum()) == int(row[cols].sum()) == windows
            want = [("nan" if not windows else repr(int(c) / windows)) if freq else str(int(c)) for c in row[cols]]
            assert line[3:] == want, (k, canonical, freq, rid)


def test_argument_errors_are_raised_without_a_device():
    from kmerdb_amd import codons, composition
    good = (b"ACGTACGT", [0, 8])
    for bad_k in (0, 7, -1):
        with pytest.raises(ValueError):
            composition.record_tables(*good, bad_k)
    for k, stride in [(3, 0), (3, 4), (1, 2)]:
        with pytest.raises(ValueError):
            composition.record_tables(*good, k, stride=stride)
    with pytest.raises(ValueError):
        composition.record_tables(*good, 3, stride=3, phase=3, continues=True)
    with pytest.raises(ValueError):
        composition.record_tables(*good, 3, stride=3, phase=1)                 # a phase without continues
    for k in (True, "3", 3.0, None):
        with pytest.raises(TypeError):
            composition.record_tables(*good, k)
    with pytest.raises(TypeError):
        composition.record_tables("ACGT", [0, 4], 3)
    with pytest.raises(TypeError):
        composition.record_tables(np.zeros(4, dtype=np.int32), [0, 4], 3)
    for offsets in ([1, 8], [0, 7], [0, 5, 4, 8], []):
        with pytest.raises(ValueError):
            composition.record_tables(good[0], offsets, 3)
    with pytest.raises(ValueError, match="2\\^31"):
        composition.record_tables(b"", np.zeros(524289 + 1, dtype=np.uint64), 6)
    with pytest.raises(TypeError):
        list(composition.tables_file(None, 3))
    with pytest.raises(ValueError):
        list(composition.tables_file("x.fa", 9))
    with pytest.raises(TypeError):
        codons.codon_tables("x.fa", include_noncanonicals=1)
    with pytest.raises(TypeError):
        codons.codon_frequency_table(b"ATGTAA", "x")
    with pytest.raises(TypeError):
        codons.codon_frequency_table("ATGTAA", 5)
    with pytest.raises(ValueError):
        codons.codon_frequency_table("ATGTAAA", "x")                          # (before the device: the length is not divisible by 3)
    with pytest.raises(TypeError):
        codons.codon_usage_bias(None, "x.fa")
    with pytest.raises(TypeError):
        codons.codons(None)


def test_command_line_has_the_three_subcommands():
    from kmerdb_amd import profile
    ap = profile.build_parser()
    a = ap.parse_args(["composition", "-k", "4", "--do-not-canonicalize", "--as-frequencies", "x.fa"])
    assert (a.cmd, a.k, a.do_not_canonicalize, a.as_frequencies, a.seqfile, a.device) == ("composition", 4, True, True, "x.fa", 0)
    a = ap.parse_args(["codons", "--as-frequencies", "--ignore-invalid-cds", "--include-noncanonicals", "--include-stop-codons", "--include-start-codons",
                       "--no-stop-codons-in-table", "--output-delimiter", ",", "--as-reference", "--device", "1", "x.fa"])
    assert (a.cmd, a.as_frequencies, a.ignore_invalid_cds, a.include_noncanonicals, a.include_stop_codons, a.include_start_codons, a.no_stop_codons_in_table,
            a.output_delimiter, a.as_reference, a.device, a.fasta) == ("codons", True, True, True, True, True, True, ",", True, 1, "x.fa")
    a = ap.parse_args(["CUB", "--sequences", "genes.fa", "table.tsv"])
    assert (a.cmd, a.sequences, a.input, a.ddof, a.delimiter, a.as_reference) == ("CUB", "genes.fa", "table.tsv", 60, "\t", False)
