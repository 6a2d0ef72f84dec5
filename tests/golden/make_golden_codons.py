#!/usr/bin/env python3
"""Golden data for codon tables: what the REFERENCE's own kmerdb/codons.py (loaded unmodified, as in make_golden.py, with the Bio
stand-in) returns or raises on a small seeded FASTA of coding sequences.

    python tests/golden/make_golden_codons.py        (build container only: needs the reference checkout and pandas)

Writes inputs/cds.fa and codons.json (data only):
  constants   the reference's codon_table, STOP_CODONS, POSSIBLE_START_CODONS, synonymous_codons
  records     per record: get_codons_in_order, is_sequence_cds (both include_noncanonicals) and, per (include_start_codons,
              include_stop_codons), codon_frequency_table -- each as its result or the class of the exception it raised
  expected    get_expected_codon_frequencies for a few L, on the forward codon counts of the valid genes (counted here, plainly)
  cub         per gene against that table: the expected frequencies, and chisq = Sum (obs - exp)^2 / exp over the 61 codons that are no
              stop, evaluated exactly on the float64 inputs (fractions.Fraction) and rounded once; null where an expected value is 0
              (the reference leaves the gene out, __init__.py:396-398), nan where every expected count is truncated to 0 and the
              frequencies are 0 / 0 (a short gene: the reference's test for zeros does not see a nan, and it prints nan)
"""
import importlib.util
import json
import os
import sys
from fractions import Fraction

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import REFPKG, load_reference  # noqa: E402

FLAGS = [(False, False), (True, False), (False, True), (True, True)]       # (include_start_codons, include_stop_codons)
EXPECTED_L = [3, 300, 999, 3000, 30000]
WRAP = 60


def load_codons():
    load_reference()
    spec = importlib.util.spec_from_file_location("kmerdb.codons", os.path.join(REFPKG, "codons.py"))
    m = importlib.util.module_from_spec(spec)
    sys.modules["kmerdb.codons"] = m
    spec.loader.exec_module(m)
    return m


def make_records():
    rng = np.random.Generator(np.random.PCG64(20260917))
    sense = [a + b + c for a in "ACGT" for b in "ACGT" for c in "ACGT" if a + b + c not in ("TAA", "TAG", "TGA")]

    def body(n):
        return "".join(sense[i] for i in rng.integers(0, len(sense), size=n))

    def with_n(seq, triplets, at=1):
        s = list(seq)
        for t in triplets:
            s[3 * t + at] = "N"
        return "".join(s)

    recs = [("gene_a", "ATG" + body(28) + "TAA"), ("gene_b", "ATG" + body(58) + "TAA"), ("gene_c", "ATG" + body(97) + "TAA"),
            ("stop_tag", "ATG" + body(40) + "TAG"), ("stop_tga", "ATG" + body(33) + "TGA"),
            ("start_gtg", "GTG" + body(45) + "TAA"), ("start_ttg", "TTG" + body(21) + "TAA"),
            ("start_ccc", "CCC" + body(30) + "TAA"), ("stop_ccc", "ATG" + body(30) + "CCC"),
            ("poly_aaa_ttt", "ATG" + "TTTAAA" * 8 + "TAA")]
    g = "ATG" + body(50) + "TAA"
    recs += [("n_first", with_n(g, [0])), ("n_second", with_n(g, [1], at=0)), ("n_middle", with_n(g, [25], at=2)), ("n_last", with_n(g, [51])),
             ("n_first_last", with_n(g, [0, 51])), ("n_two", with_n(g, [7, 30])), ("n_three", with_n(g, [7, 30, 44])),
             ("n_run", with_n(with_n(g, [12], at=2), [13], at=0))]
    recs += [("len3_atg", "ATG"), ("len3_taa", "TAA"), ("len6", "ATGTAA"), ("len7", "ATGTAAA"), ("len8", "ATGCCTAA"), ("len9", "ATGCCCTAA"),
             ("len6_n", "ANGTAA")]
    recs.append(("long_gene", "ATG" + body(998) + "TAA"))                   # 3 000 residues
    recs.append(("gene_d", "ATG" + body(600) + "TGA"))
    return recs


def jsonable(x):
    if isinstance(x, (np.integer,)):
        return int(x)
    if isinstance(x, (np.floating,)):
        return float(x)
    if isinstance(x, np.ndarray):
        return [jsonable(v) for v in x.tolist()]
    if isinstance(x, (list, tuple)):
        return [jsonable(v) for v in x]
    return x


def attempt(f):
    try:
        return {"raises": None, "value": jsonable(f())}
    except BaseException as e:  # noqa: BLE001 - whatever class the reference raises is the datum
        return {"raises": type(e).__name__}


def forward_counts(seq):
    """the frame-0 triplets of a gene without N, first and last left out, by forward id"""
    digit = {"A": 0, "C": 1, "G": 2, "T": 3}
    counts = np.zeros(64, dtype=np.uint32)
    trip = [seq[i:i + 3] for i in range(0, len(seq), 3)]
    for t in trip[1:-1]:
        counts[16 * digit[t[0]] + 4 * digit[t[1]] + digit[t[2]]] += 1
    return counts


def exact_chisq(obs, exp):
    total = sum(((Fraction(float(o)) - Fraction(float(e))) ** 2) / Fraction(float(e)) for o, e in zip(obs, exp))
    return float(total)


def main():
    import pandas as pd
    codons = load_codons()                                                   # (puts the Bio stand-in on the path)
    from Bio.Seq import Seq
    from Bio.SeqRecord import SeqRecord
    recs = make_records()
    with open(os.path.join(HERE, "inputs", "cds.fa"), "w") as f:
        for rid, s in recs:
            f.write(">{0} seeded coding sequence\n".format(rid))
            f.write("".join(s[i:i + WRAP] + "\n" for i in range(0, len(s), WRAP)))
    out = {"constants": {"codon_table": {str(k): v for k, v in codons.codon_table.items()}, "STOP_CODONS": codons.STOP_CODONS,
                         "POSSIBLE_START_CODONS": codons.POSSIBLE_START_CODONS, "synonymous_codons": codons.synonymous_codons},
           "flags": FLAGS, "records": []}
    for rid, s in recs:
        case = {"id": rid, "length": len(s),
                "get_codons_in_order": attempt(lambda: codons.get_codons_in_order(s, seq_id=rid)),
                "is_sequence_cds": [attempt(lambda: codons.is_sequence_cds(SeqRecord(Seq(s), id=rid), include_noncanonicals=inc)) for inc in (False, True)],
                "codon_frequency_table": []}
        for start, stop in FLAGS:
            got = attempt(lambda: codons.codon_frequency_table(s, rid, include_stop_codons=stop, include_start_codons=start))
            if got["raises"] is None and start != stop:
                got["value"] = got["value"][:2]                              # (the two lists of floats are kept for two of the four)
            case["codon_frequency_table"].append(got)
        out["records"].append(case)
    genes = [(rid, s) for rid, s in recs if len(s) % 3 == 0 and "N" not in s and len(s) >= 9]
    table = np.array([forward_counts(s) for _, s in genes], dtype=np.uint32)
    df = pd.DataFrame(table, index=[rid for rid, _ in genes])
    out["table_ids"] = [rid for rid, _ in genes]
    out["table"] = jsonable(table)
    out["expected"] = [{"L": L, "value": jsonable(codons.get_expected_codon_frequencies(L, df))} for L in EXPECTED_L]
    keep = [i for i in range(64) if i not in codons.STOP_CODONS]
    out["cub"] = []
    for (rid, s), row in zip(genes, table):
        _, exp = codons.get_expected_codon_frequencies(len(s), df)
        obs = np.array(row) / np.sum(row)
        o, e = [obs[i] for i in keep], [exp[i] for i in keep]
        out["cub"].append({"id": rid, "expected": jsonable(exp), "chisq": None if 0.0 in e else float("nan") if np.any(np.isnan(e)) else exact_chisq(o, e)})
    json.dump(out, open(os.path.join(HERE, "codons.json"), "w"))
    nraise = sum(1 for c in out["records"] for g in c["codon_frequency_table"] if g["raises"])
    print("{0} records, {1} codon_frequency_table cases raise, {2} genes in the table, {3} with a chi-square".format(
        len(recs), nraise, len(genes), sum(1 for c in out["cub"] if c["chisq"] is not None and c["chisq"] == c["chisq"])))
    for c in out["records"]:
        g = c["get_codons_in_order"]
        print(c["id"], c["length"], g["raises"] or (len(g["value"][0]), g["value"][1]), [x["raises"] or x["value"] for x in c["is_sequence_cds"]])


if __name__ == "__main__":
    main()
