"""Codon tables and codon usage bias with the counting on the device: the reference's kmerdb/codons.py and its `codons` and `CUB`
subcommands (kmerdb/__init__.py:214-421) on kdb_record_tables at k = 3, stride 3 (kmerdb_amd.composition).

The device returns, per record, the 64 counts of its frame-0 triplets, how many triplets hold an N (they are skipped and the frame is
kept, codons.py:205-222) and the ids of the first and the last counted triplet.  Everything the reference derives from its list of
codon ids follows from those on the host: the list's element 0 is first_id, its last element last_id.

Two deliberate deviations from the reference, both undone by as_reference=True (which exists to pin this module to the reference bit
for bit):
  * ids.  The reference calls kmer_to_id(codon) with its default canonicalize=True (codons.py:208), so every id is min(id, rc(id)):
    TTT and AAA share bin 0, ...TAG ends in id 28 and ...TGA in 52, which are no stop codons, and GTG... starts with 17.  The keys of its
    own codon_table (14 = ATG = M, 63 = TTT = F) show that forward ids were meant; forward ids are the default here.
  * serine.  The dict literal synonymous_codons has the key "S" twice (codons.py:122 and :136); [9, 11] survives, so the reference
    divides the family frequency of ids 52..55 by counts[9] + counts[11].  Here the serine family is all six codons.  Its "R" entry
    (codons.py:135) lacks AGA and AGG, ids 8 and 10, which codon_table calls R: their family frequency is divided by the other four's
    counts and can pass 1.  Here the arginine family is all six codons too.
One more, not undone: a residue outside upper-case ACGTN is refused (ValueError), also where it shares a triplet with an N; the
reference never looks at the letters of such a triplet.  There is no CPU fallback: without a device the counting functions raise.
"""
import sys

import numpy as np

from . import composition, kmer

# the standard genetic code over forward 3-mer ids (A 0, C 1, G 2, T 3; id = 16 first + 4 second + third); * = stop
GENETIC_CODE = "KNKNTTTTRSRSIIMI" "QHQHPPPPRRRRLLLL" "EDEDAAAAGGGGVVVV" "*Y*YSSSS*CWCLFLF"
assert len(GENETIC_CODE) == 64

CODON_LIST = list(range(64))
codon_table = {i: (None if aa == "*" else aa) for i, aa in enumerate(GENETIC_CODE)}
CODON_IUPAC_CODES = [codon_table[i] for i in CODON_LIST]
STOP_CODONS = [i for i in CODON_LIST if codon_table[i] is None]                         # TAA 48, TAG 50, TGA 56
POSSIBLE_START_CODONS = sorted(kmer.kmer_to_id(c, canonicalize=False) for c in ("ATG", "GTG", "TTG"))
synonymous_codons = {}
for _i in CODON_LIST:
    if codon_table[_i] is not None:
        synonymous_codons.setdefault(codon_table[_i], []).append(_i)
del _i
REFERENCE_SERINE_FAMILY = [9, 11]                                                       # what survives of the reference's two "S" keys
REFERENCE_ARGININE_FAMILY = [24, 25, 26, 27]                                            # its "R" entry: without AGA 8 and AGG 10


def _families(as_reference):
    if not as_reference:
        return synonymous_codons
    fam = dict(synonymous_codons)
    fam["S"] = REFERENCE_SERINE_FAMILY
    fam["R"] = REFERENCE_ARGININE_FAMILY
    return fam


def _sequence(seq):
    """-> (str of the residues, id or None) of a str or a record with .seq"""
    s = seq if isinstance(seq, str) else getattr(seq, "seq", None)
    if s is None:
        raise TypeError("kmerdb_amd.codons expects a str or a record with .seq as the sequence")
    return str(s), (None if isinstance(seq, str) else getattr(seq, "id", None))


def _triplets(text, as_reference, device):
    """the device's view of one sequence -> (row: uint32[64], windows, skipped, first_id, last_id)"""
    raw = text.encode("ascii")
    tables, windows, skipped, first, last = composition.record_tables(raw, np.array([0, len(raw)], dtype=np.uint64), 3, stride=3,
                                                                      canonical=bool(as_reference), device=device)
    return tables[0], int(windows[0]), int(skipped[0]), int(first[0]), int(last[0])


# ---- the host rules: what the reference derives from its list of codon ids, from the device's five outputs ----

def is_non_canonical(windows, skipped, first_id, last_id):
    """get_codons_in_order's flag (codons.py:213, :224-228): a triplet was skipped, or the first is no start codon, or the last no stop
    codon.  Without a skipped triplet the first and the last counted triplet are the sequence's first and last."""
    return bool(skipped > 0 or (windows > 0 and (first_id not in POSSIBLE_START_CODONS or last_id not in STOP_CODONS)))


def counts_from_row(row, windows, first_id, last_id, include_start_codons=False, include_stop_codons=False):
    """count_codons (codons.py:238-273) on the device's row: the list's element 0 (the first counted triplet, whatever it is) is left
    out unless include_start_codons, its last element unless include_stop_codons.  A list of one element is element 0 alone (:261-265
    come before :266): include_start_codons decides, and it leaves at most once."""
    counts = np.array(row, dtype=np.uint32)
    if windows > 0 and not include_start_codons:
        counts[first_id] -= 1
    if windows > 1 and not include_stop_codons:
        counts[last_id] -= 1
    return counts


def check_triplet_count(seqid, length, skipped):
    """codon_frequency_table's refusals (codons.py:306-315)"""
    if length % 3 != 0:
        raise ValueError("kmerdb_amd.codons.codon_frequency_table() expects the sequence length to be divisible by three")
    if skipped > 2:
        raise ValueError("For sequence '{0}', the number of codons ({1}) should be proportional to the length ({2}/3) of the sequence..."
                         .format(seqid, length // 3 - skipped, length))


def family_frequencies(counts, as_reference=False):
    """codon_frequencies_in_family (codons.py:320-330): every codon's count over its amino acid's family's; 0.0 for stops and empty families"""
    fam = _families(as_reference)
    out = np.zeros(64)
    for i in CODON_LIST:
        aa = codon_table[i]
        if aa is not None:
            total = int(counts[fam[aa]].sum())
            if total != 0:
                out[i] = float(counts[i]) / total
    return out


def _cds_verdict(length, windows, skipped, first_id, last_id, include_noncanonicals):
    """is_sequence_cds (codons.py:141-172) as a plain bool"""
    if length % 3 != 0:
        return False
    if not is_non_canonical(windows, skipped, first_id, last_id):
        return True
    # the reference answers only where the first codon of its list is no start codon (:165-170); a bad stop alone, or a skipped
    # triplet behind a good start, falls off the end of its function: None, which its caller treats as false
    return bool(include_noncanonicals) and first_id not in POSSIBLE_START_CODONS


# ---- the reference's functions ----

def is_sequence_cds(record, include_noncanonicals=False, as_reference=False, device=0):
    """Whether a sequence (a str or a record with .seq) is a coding sequence: length divisible by 3, a start codon first, a stop codon
    last, no triplet with an N.  A plain bool; with include_noncanonicals a sequence whose first codon is no start codon passes, as
    in the reference (codons.py:165-167)."""
    text, _ = _sequence(record)
    if type(include_noncanonicals) is not bool:
        raise TypeError("kmerdb_amd.codons.is_sequence_cds() expects the keyword argument 'include_noncanonicals' to be a bool")
    if len(text) % 3 != 0:
        return False
    _, windows, skipped, first_id, last_id = _triplets(text, as_reference, device)
    return _cds_verdict(len(text), windows, skipped, first_id, last_id, include_noncanonicals)


def codon_frequency_table(seq, seqid, include_stop_codons=False, include_start_codons=False, as_reference=False, device=0):
    """The reference's codon_frequency_table (codons.py:279-333) for one sequence -> (codon ids, counts: uint32[64], counts / counts.sum()
    as a list, the frequencies inside the synonymous families as a list)."""
    if type(seq) is not str:
        raise TypeError("kmerdb_amd.codons.codon_frequency_table() expects a str as its first positional argument")
    if type(seqid) is not str:
        raise TypeError("kmerdb_amd.codons.codon_frequency_table() expects a str as its second positional argument")
    if type(include_start_codons) is not bool:
        raise TypeError("kmerdb_amd.codons.codon_frequency_table() expects the keyword argument 'include_start_codons' to be a bool")
    if type(include_stop_codons) is not bool:
        raise TypeError("kmerdb_amd.codons.codon_frequency_table() expects the keyword argument 'include_stop_codons' to be a bool")
    if len(seq) % 3 != 0:
        raise ValueError("kmerdb_amd.codons.codon_frequency_table() expects the sequence length to be divisible by three")
    row, windows, skipped, first_id, last_id = _triplets(seq, as_reference, device)
    check_triplet_count(seqid, len(seq), skipped)
    counts = counts_from_row(row, windows, first_id, last_id, include_start_codons, include_stop_codons)
    with np.errstate(invalid="ignore", divide="ignore"):
        wrt_length = np.array(counts) / np.sum(counts)
    return list(CODON_LIST), counts, wrt_length.tolist(), family_frequencies(counts, as_reference).tolist()


def get_expected_codon_frequencies(L, counts):
    """codons.py:336-360: the expected codon counts of a sequence of L residues under the column sums of a table of codon counts (rows:
    genes, 64 columns), truncated to uint32 as the reference truncates them -> (expected counts, expected counts / their sum)."""
    if isinstance(L, bool) or not isinstance(L, (int, np.integer)):
        raise TypeError("kmerdb_amd.codons.get_expected_codon_frequencies() expects L to be an int")
    counts = np.asarray(counts)
    if counts.ndim != 2 or counts.shape[1] != 64:
        raise ValueError("kmerdb_amd.codons.get_expected_codon_frequencies() expects a table of 64 columns as its second positional argument")
    total = np.array(counts.sum(axis=0), dtype="float64")
    frac = total / int(total.sum())
    exp_cnts = np.array(frac * (int(L) / 3), dtype="uint32")
    with np.errstate(invalid="ignore", divide="ignore"):
        return exp_cnts, exp_cnts / exp_cnts.sum()


def codon_tables(fasta, include_start_codons=False, include_stop_codons=False, include_noncanonicals=False, ignore_invalid_cds=False,
                 as_reference=False, device=0, block_bytes=None):
    """The codon counts of every CDS of a FASTA file (the loop of kmerdb/__init__.py:239-289) -> (ids: list[str], counts: uint32[n, 64],
    non_canonical: bool[n]).  A record whose length is not divisible by 3 is left out with ignore_invalid_cds, else a ValueError
    (:247-254); more than two triplets with an N: ValueError (codons.py:313-315); a non-canonical record -- a skipped triplet, a first
    codon that is no start codon, a last one that is no stop codon -- ValueError unless include_noncanonicals (:257-259)."""
    for name, v in (("include_start_codons", include_start_codons), ("include_stop_codons", include_stop_codons),
                    ("include_noncanonicals", include_noncanonicals), ("ignore_invalid_cds", ignore_invalid_cds), ("as_reference", as_reference)):
        if type(v) is not bool:
            raise TypeError("kmerdb_amd.codons.codon_tables() expects the keyword argument '{0}' to be a bool".format(name))
    ids, rows, flags = [], [], []
    for rid, length, windows, skipped, first_id, last_id, table in composition.tables_file(fasta, 3, stride=3, canonical=as_reference, device=device,
                                                                                           block_bytes=block_bytes):
        if length % 3 != 0:
            msg = "Sequence '{0}' has a length {1} that is not evenly divisible into length-3 codons".format(rid, length)
            if ignore_invalid_cds:
                sys.stderr.write("WARNING: " + msg + "\n")
                continue
            raise ValueError(msg)
        check_triplet_count(rid, length, skipped)
        non_canonical = is_non_canonical(windows, skipped, first_id, last_id)
        if non_canonical and not include_noncanonicals:
            raise ValueError("Refusing to proceed due to non-canonical sequence '{0}' which has a non-canonical start or stop codon. "
                             "Use --include-noncanonicals to proceed otherwise.".format(rid))
        ids.append(rid)
        rows.append(counts_from_row(table, windows, first_id, last_id, include_start_codons, include_stop_codons))
        flags.append(non_canonical)
    return ids, (np.array(rows, dtype=np.uint32) if rows else np.zeros((0, 64), dtype=np.uint32)), np.array(flags, dtype=bool)


def format_table(ids, rows, columns, output_delimiter="\t"):
    """What pandas' DataFrame(data).transpose().to_csv(sep=..., index=True, header=columns) prints (kmerdb/__init__.py:291-299): an empty
    field and the column names, then a line per record -- its id, integers as such, floats as repr(float)."""
    lines = [output_delimiter.join([""] + [str(c) for c in columns]) + "\n"]
    for rid, row in zip(ids, rows):
        vals = row.tolist() if isinstance(row, np.ndarray) else list(row)
        lines.append(output_delimiter.join([str(rid)] + [repr(float(v)) if isinstance(v, float) else str(v) for v in vals]) + "\n")
    return "".join(lines)


def codons(fasta, as_frequencies=False, ignore_invalid_cds=False, include_noncanonicals=False, include_stop_codons=False,
           include_start_codons=False, no_stop_codons_in_table=False, output_delimiter="\t", as_reference=False, out=None, device=0):
    """The `codons` subcommand (kmerdb/__init__.py:214-299): the codon counts of every CDS, a line per record under a header of the 64
    codons in id order; with as_frequencies the frequencies inside the synonymous families; with no_stop_codons_in_table (counts only, as
    in the reference) the 61 columns that are no stop codon.  -> the number of records printed."""
    if type(fasta) is not str:
        raise TypeError("kmerdb_amd.codons.codons expects the FASTA file as a str filepath")
    if as_frequencies and no_stop_codons_in_table:
        # (the reference keeps the 64 frequencies and drops three of the names, :275-298, and pandas refuses to print that)
        raise ValueError("kmerdb_amd.codons: --as-frequencies prints all 64 columns; it cannot be combined with --no-stop-codons-in-table")
    out = sys.stdout if out is None else out
    ids, counts, _ = codon_tables(fasta, include_start_codons=include_start_codons, include_stop_codons=include_stop_codons,
                                  include_noncanonicals=include_noncanonicals, ignore_invalid_cds=ignore_invalid_cds, as_reference=as_reference,
                                  device=device)
    cols = [c for c in CODON_LIST if not (no_stop_codons_in_table and c in STOP_CODONS)]
    if as_frequencies:
        rows = [family_frequencies(c, as_reference) for c in counts]
    else:
        rows = [c[cols] for c in counts]
    out.write(format_table(ids, rows, [kmer.id_to_kmer(c, 3) for c in cols], output_delimiter))
    return len(ids)


def read_codon_table(path, delimiter="\t"):
    """a table as `codons` prints it -> (ids, float64[n, 64]); one of 61 columns gets zeros at the stop codons (kmerdb/__init__.py:325-337)"""
    ids, rows = [], []
    with open(path) as f:
        header = f.readline().rstrip("\n").split(delimiter)
        ncols = len(header) - 1
        if ncols not in (61, 64):
            raise ValueError("kmerdb_amd CUB | invalid matrix dimensions")
        for line in f:
            line = line.rstrip("\n")
            if not line:
                continue
            fields = line.split(delimiter)
            if len(fields) != ncols + 1:
                raise ValueError("kmerdb_amd CUB | invalid matrix dimensions")
            ids.append(fields[0])
            rows.append([float(x) for x in fields[1:]])
    table = np.array(rows, dtype=np.float64).reshape(len(rows), ncols)
    if ncols == 61:
        wide = np.zeros((len(rows), 64))
        wide[:, [c for c in CODON_LIST if codon_table[c] is not None]] = table
        table = wide
    return ids, table


def chi_square(observed_counts, expected_frequencies):
    """-> chisq of the observed counts / counts.sum() against the expected frequencies, over the 61 ids that are no stop codon, in
    float64 (kmerdb/__init__.py:388-400); None where an expected frequency is 0"""
    keep = [c for c in CODON_LIST if c not in STOP_CODONS]
    with np.errstate(invalid="ignore", divide="ignore"):
        obs = (np.array(observed_counts) / np.sum(observed_counts))[keep]
    exp = np.asarray(expected_frequencies, dtype=np.float64)[keep]
    if np.any(exp == 0):
        return None
    return float(((obs - exp) ** 2 / exp).sum())


def codon_usage_bias(table, sequences, delimiter="\t", output_delimiter="\t", include_start_codons=False, include_stop_codons=False,
                     ignore_invalid_cds=False, ddof=60, as_reference=False, out=None, device=0):
    """The `CUB` subcommand (kmerdb/__init__.py:302-421): a chi-square of every gene's codon usage against a `codons` table.  Per record
    of `sequences`: the expected frequencies of a sequence of its length under the table, the observed counts / counts.sum() from the
    device, chisq over the 61 codons that are no stop; pval = chi2.sf(chisq, 61 - 1 - ddof), nan where that leaves no degree of freedom
    -- the reference's ddof = 60 does (:400), and its Bonferroni factor is 1 (:417).  A record with an expected frequency of 0 is left
    out with a warning.  Prints `<delim>chisq<delim>pval`, then id, chisq, pval per record -> [(id, chisq, pval)]."""
    if type(table) is not str or type(sequences) is not str:
        raise TypeError("kmerdb_amd.codons.codon_usage_bias expects the table and the sequences as str filepaths")
    if isinstance(ddof, bool) or not isinstance(ddof, (int, np.integer)):
        raise TypeError("kmerdb_amd.codons.codon_usage_bias expects ddof to be an int")
    out = sys.stdout if out is None else out
    _, counts_table = read_codon_table(table, delimiter)
    dof = 61 - 1 - int(ddof)
    results = []
    for rid, length, windows, skipped, first_id, last_id, row in composition.tables_file(sequences, 3, stride=3, canonical=bool(as_reference),
                                                                                         device=device):
        try:
            check_triplet_count(rid, length, skipped)
        except ValueError:
            if ignore_invalid_cds:
                sys.stderr.write("WARNING: Sequence '{0}' had one or more criterion making it an invalid CDS (typically its length ({1}) was not "
                                 "divisible by three)\n".format(rid, length))
                continue
            raise
        observed = counts_from_row(row, windows, first_id, last_id, include_start_codons, include_stop_codons)
        _, expected = get_expected_codon_frequencies(length, counts_table)
        chisq = chi_square(observed, expected)
        if chisq is None:
            sys.stderr.write("WARNING: Sequence '{0}' had one or more 0 counts. Cannot produce a valid chi-square test...\n".format(rid))
            continue
        pval = float("nan")
        if dof > 0:
            from scipy.stats import chi2
            pval = float(chi2.sf(chisq, dof))
        results.append((rid, chisq, pval))
    out.write(output_delimiter.join(["", "chisq", "pval"]) + "\n")
    for rid, chisq, pval in results:
        out.write(output_delimiter.join([str(rid), repr(chisq), repr(pval)]) + "\n")
    return results
