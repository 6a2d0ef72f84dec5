"""Reads scored against a finished k-mer profile: the reference's markov_probability (kmerdb/probability.py:36-151) on the device.

The reference computes the log-probability of one sequence under the (k-1)-order Markov chain that a profile defines, one
index.read_line per window through a .kdbi index on disk; its command-line entry is commented out (kmerdb/__init__.py:2375-2388).
Here kdb_score_reads (csrc/kdb_score.hip.h) does one random 32-byte read of the count vector in HBM per window, for a whole batch of
records: score_reads is that call, score_file streams a FASTA/FASTQ file through it against a .kdb, markov_probability has the
reference's shape.  DESIGN.md section 14 has the definition.  There is no CPU fallback: without a device these raise.
"""
import ctypes
import math
import sys

import numpy as np

from . import _abi, _records, fileutil

COLUMNS = ("id", "length", "windows", "zero_windows", "min_count", "log10_p", "log_odds_ratio")
NO_COUNT = 2 ** 64 - 1                     # min_count of a record without a scored window


def log_odds_ratio(log10_p, k):
    """log10_p / log10(4^-k): the reference's `lor` (probability.py:146-147).

    The reference divides log10(px) + total, which is log10_p, by null_model = log10(um) + total2 with um = 1 / 4^k (:53) and
    total2 = Sum over the transitions of log10(sum_aij) (:131).  sum_aij adds mononucleotides[char] / total_nucleotides over the four
    suffix letters A, C, G, T (:97-98), and total_nucleotides is the sum of those same four values (:87): sum_aij is 1 and every
    log10(sum_aij) is 0.  So null_model = log10(4^-k), whatever the sequence and the mononucleotide table."""
    return float(log10_p) / math.log10(1.0 / 4 ** int(k))


def _check_scalars(k, total, pseudocount):
    for name, v in (("k", k), ("total", total), ("pseudocount", pseudocount)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise TypeError("kmerdb_amd.probability: {0} must be an int, not {1}".format(name, type(v).__name__))
    k, total, pseudocount = int(k), int(total), int(pseudocount)
    if not 1 <= k <= 17:
        raise ValueError("kmerdb_amd.probability: k={0} out of range 1..17".format(k))
    if total <= 0:
        raise ValueError("kmerdb_amd.probability: the profile's total must be positive (an empty profile gives no probabilities)")
    if pseudocount < 0:
        raise ValueError("kmerdb_amd.probability: the pseudocount must not be negative")
    if total + pseudocount * 4 ** k >= 2 ** 64 or 4 * pseudocount >= 2 ** 64:
        raise ValueError("kmerdb_amd.probability: total + pseudocount * 4^k and 4 * pseudocount must stay below 2^64")
    return k, total, pseudocount


def _vector_pointer(vector, k, device):
    """-> (device pointer, what keeps the memory alive)"""
    if isinstance(vector, bool):
        raise TypeError("kmerdb_amd.probability: vector must be a torch tensor on the device or a device pointer")
    if isinstance(vector, (int, np.integer)):
        if int(vector) == 0 or int(vector) % 16:
            raise ValueError("kmerdb_amd.probability: the vector's device pointer is NULL or not 16-byte aligned")
        return int(vector), None
    if not (hasattr(vector, "data_ptr") and hasattr(vector, "numel") and hasattr(vector, "is_cuda")):
        raise TypeError("kmerdb_amd.probability: vector must be a torch tensor on the device or a device pointer, not {0}".format(type(vector).__name__))
    if vector.element_size() != 8 or vector.is_floating_point() or not vector.is_contiguous() or vector.dim() != 1:
        raise ValueError("kmerdb_amd.probability: the vector must be a contiguous one-dimensional int64 / uint64 tensor")
    if int(vector.numel()) != 4 ** k:
        raise ValueError("kmerdb_amd.probability: the vector holds {0} bins, 4^k = {1} expected".format(int(vector.numel()), 4 ** k))
    if not vector.is_cuda or vector.device.index != int(device):
        raise ValueError("kmerdb_amd.probability: the vector must lie on device {0} (there is no CPU fallback)".format(device))
    return int(vector.data_ptr()), vector


def score_reads_raw(pointer, k, canonical, total, pseudocount, bases, offsets, continues=False, device=0, none_scored=False):
    """kdb_score_reads on a raw device pointer -> (log10_p, windows, zero_windows, min_count, kernel_ms)."""
    nreads = int(offsets.size) - 1
    log10_p = np.empty(nreads, dtype=np.float64)
    windows, zeros, mins = (np.empty(nreads, dtype=np.uint64) for _ in range(3))
    ms = ctypes.c_double(0.0)
    flags = (_abi.KDB_SCORE_CONTINUES | (_abi.KDB_SCORE_NONE_SCORED if none_scored else 0)) if continues else 0
    _abi.check(_abi.lib().kdb_score_reads(int(device), ctypes.c_void_p(int(pointer)), int(k), 1 if canonical else 0, int(total), int(pseudocount),
                                          bases.ctypes.data if bases.size else None, int(bases.size), offsets.ctypes.data, nreads,
                                          flags, log10_p.ctypes.data, windows.ctypes.data, zeros.ctypes.data, mins.ctypes.data, ctypes.byref(ms)))
    return log10_p, windows, zeros, mins, ms.value


def score_reads(bases, offsets, vector, k, canonical, total, pseudocount=0, continues=False, device=0, none_scored=False):
    """Score a batch of records against a profile -> (log10_p: float64[n], windows, zero_windows, min_count: uint64[n]).

    bases / offsets: the concatenated residues and the nreads + 1 record offsets, as Engine.submit takes them.  vector: the 4^k counts as
    a torch int64 / uint64 tensor on `device`, or a device pointer.  total: the profile's total_kmers.  continues: record 0 is the next
    piece of the previous call's last record (KDB_SCORE_CONTINUES); none_scored, with continues: no piece of that record has held a scored
    window so far, so its first one here is the record's first and takes the initial term (KDB_SCORE_NONE_SCORED).
    ValueError for what the engine refuses (a record shorter than k, a residue outside ACGTN); log10_p is -inf for a record with a k-mer the profile lacks (pseudocount 0), nan for one without a scored window."""
    k, total, pseudocount = _check_scalars(k, total, pseudocount)
    if none_scored and not continues:
        raise ValueError("kmerdb_amd.probability: none_scored is for a record that continues the previous call's last one")
    bases, offsets = _records.check_batch("probability", bases, offsets)
    pointer, keep = _vector_pointer(vector, k, device)
    from .distance import _require_device
    _require_device(device)
    if keep is not None:
        import torch
        torch.cuda.synchronize(int(device))               # (the upload, or whatever produced the tensor: the call runs on a stream of its own)
    out = score_reads_raw(pointer, k, canonical, total, pseudocount, bases, offsets, continues, device, none_scored)[:4]
    del keep
    return out


def profile_is_canonical(counts, k, metadata=None):
    """Whether a count vector holds canonical k-mers.  A header key "canonical" decides where a file has one; the .kdb format of the
    reference has none, and then the counts do: a canonical profile has nothing in a bin whose id is above its reverse complement's.
    Every bin is looked at up to k = 12, the first 65 536 occupied bins above that (about a quarter of a forward profile's occupied
    bins are such bins, from the first ids on)."""
    if metadata is not None and "canonical" in metadata:
        return bool(metadata["canonical"])
    counts = np.asarray(counts)
    k = int(k)
    if counts.size <= 4 ** 12:
        ids = np.flatnonzero(counts).astype(np.uint64)
    else:
        ids, at, step = [], 0, 1 << 24
        while at < counts.size and sum(x.size for x in ids) < 65536:
            ids.append(np.flatnonzero(counts[at:at + step]).astype(np.uint64) + np.uint64(at))
            at += step
        ids = np.concatenate(ids)[:65536]
    rc = np.zeros_like(ids)
    x = ids.copy()
    for _ in range(k):
        rc = (rc << np.uint64(2)) | (np.uint64(3) - (x & np.uint64(3)))
        x >>= np.uint64(2)
    return not bool(np.any(ids > rc))


def _open_profile(kdb):
    """-> (counts: uint64[4^k] on the host, k, total_kmers, canonical)"""
    if isinstance(kdb, str):
        kdb = fileutil.read_kdb(kdb)
    if not (hasattr(kdb, "metadata") and hasattr(kdb, "counts")):
        raise TypeError("kmerdb_amd.probability expects what fileutil.open(..., slurp=True) returns, or a .kdb filepath, as the profile")
    if getattr(kdb, "completed", True) is False:
        kdb.slurp()
    md = kdb.metadata
    k = int(md["k"])
    counts = np.ascontiguousarray(kdb.counts, dtype=np.uint64)
    total = int(md.get("total_kmers") or 0) or int(sum(int(f.get("total_kmers", 0)) for f in md.get("files", []) or []))       # (probability.py:52)
    return counts, k, total, profile_is_canonical(counts, k, md)


def _upload(counts, device):
    from .distance import _require_device
    _require_device(device)
    import torch
    return torch.from_numpy(counts.view(np.int64)).to("cuda:{0}".format(int(device)))


class _Row:
    __slots__ = ("id", "length", "windows", "zeros", "min_count", "log10_p", "last_piece")

    def __init__(self, rid, length, windows, zeros, min_count, log10_p):
        self.id, self.length, self.windows, self.zeros, self.min_count, self.log10_p, self.last_piece = rid, length, windows, zeros, min_count, log10_p, length

    def join(self, piece_len, windows, zeros, min_count, log10_p, k):
        """the next piece of the same record: it repeats the last k - 1 residues of the piece before"""
        self.length += piece_len - min(k - 1, self.last_piece)
        self.last_piece = piece_len
        if windows:
            self.log10_p = log10_p if not self.windows else self.log10_p + log10_p            # (in piece order)
        self.windows += windows
        self.zeros += zeros
        self.min_count = min(self.min_count, min_count)

    def astuple(self, k):
        return (self.id, self.length, self.windows, self.zeros, self.min_count, self.log10_p, log_odds_ratio(self.log10_p, k))


def score_file(seqfile, kdb_path, pseudocount=0, device=0, block_bytes=None):
    """Every record of a FASTA/FASTQ file against a .kdb profile: yields (id, length, windows, zero_windows, min_count, log10_p,
    log_odds_ratio) per record, in file order.  k, the totals and whether the profile is canonical come from the .kdb; its counts are
    uploaded once.  A FASTA record longer than a reader block arrives in pieces that repeat k - 1 residues: they are scored with
    KDB_SCORE_CONTINUES (and KDB_SCORE_NONE_SCORED while the record has no scored window yet) and joined here -- windows and zero_windows
    added, the minimum of min_count, log10_p added in piece order."""
    from . import reader
    if type(seqfile) is not str or type(kdb_path) is not str:
        raise TypeError("kmerdb_amd.probability.score_file expects the sequence file and the .kdb as str filepaths")
    counts, k, total, canonical = _open_profile(kdb_path)
    k, total, pseudocount = _check_scalars(k, total, pseudocount)
    rd = reader.BlockReader(seqfile, want_ids=True, block_bytes=block_bytes, overlap=k - 1)
    vector = _upload(counts, device)
    pending = None
    for block in rd:
        bases, offsets, ids = block
        cont = bool(getattr(block, "cont", False))
        # (a record whose pieces so far hold no scored window -- an N run longer than a block -- still owes its initial term)
        log10_p, windows, zeros, mins = score_reads(bases, offsets, vector, k, canonical, total, pseudocount, continues=cont, device=device,
                                                    none_scored=cont and pending is not None and pending.windows == 0)
        lens = np.diff(offsets.astype(np.int64))
        first = 0
        if cont and pending is not None:
            pending.join(int(lens[0]), int(windows[0]), int(zeros[0]), int(mins[0]), float(log10_p[0]), k)
            first = 1
        for r in range(first, len(lens)):
            if pending is not None:
                yield pending.astuple(k)
            pending = _Row(ids[r], int(lens[r]), int(windows[r]), int(zeros[r]), int(mins[r]), float(log10_p[r]))
    if pending is not None:
        yield pending.astuple(k)


def format_row(row, output_delimiter="\t"):
    """one output line of the `probability` subcommand: floats as repr prints them"""
    return output_delimiter.join(repr(float(x)) if isinstance(x, float) else str(x) for x in row) + "\n"


def probabilities(seqfile, kdb_path, pseudocount=0, output_delimiter="\t", out=None, device=0, block_bytes=None):
    """The `probability` subcommand: a header line, then score_file's rows; -> the number of records."""
    out = sys.stdout if out is None else out
    out.write(output_delimiter.join(COLUMNS) + "\n")
    n = 0
    for row in score_file(seqfile, kdb_path, pseudocount=pseudocount, device=device, block_bytes=block_bytes):
        out.write(format_row(row, output_delimiter))
        n += 1
    return n


def markov_probability(seq, kdb, pseudocount=0, device=0):
    """The reference's markov_probability (probability.py:36-151) for one sequence: -> {"seq", "log_odds_ratio", "p_of_seq", "log10_p"}.

    seq: a str, or anything with .seq (a Bio.SeqRecord).  kdb: what fileutil.open(path, slurp=True) returns, or a .kdb filepath; no index
    is needed.  log10_p = log10(px) + Sum log10(ast) in the reference's names (:75, :130-133), p_of_seq = 10 ** log10_p (the reference
    multiplies the factors instead, :140-148, and underflows sooner), log_odds_ratio as log_odds_ratio() derives it.  TypeError /
    ValueError where the reference raises them (:43-49, :57-58); ValueError also where its math.log10(0) raises: a window the profile
    does not hold, at pseudocount 0 -- and for a sequence without a single N-free window."""
    s = seq if isinstance(seq, str) else getattr(seq, "seq", None)
    if s is None:
        raise TypeError("kmerdb_amd.probability.markov_probability expects a str or a record with .seq as its first positional argument")
    if not isinstance(kdb, str) and not (hasattr(kdb, "metadata") and hasattr(kdb, "counts")):
        raise TypeError("kmerdb_amd.probability.markov_probability expects a KDBReader (fileutil.open(..., slurp=True)) or a .kdb filepath as its second positional argument")
    text = str(s).encode("ascii")
    k = int(fileutil._read_header(kdb)["k"]) if isinstance(kdb, str) else int(kdb.metadata["k"])
    if len(text) < k:
        raise ValueError("kmerdb_amd.probability.markov_probability expects the sequence to be at least k={0} in length".format(k))
    counts, k, total, canonical = _open_profile(kdb)
    vector = _upload(counts, device)
    log10_p, windows, zeros, _ = score_reads(text, np.array([0, len(text)], dtype=np.uint64), vector, k, canonical, total, pseudocount, device=device)
    if int(windows[0]) == 0:
        raise ValueError("kmerdb_amd.probability.markov_probability: the sequence has no window of k={0} residues without N".format(k))
    if int(zeros[0]) and int(pseudocount) == 0:
        raise ValueError("math domain error: {0} k-mer(s) of the sequence have a count of 0 in the profile (the reference's math.log10(0), "
                         "probability.py:75 / :133); a pseudocount makes them finite".format(int(zeros[0])))
    lp = float(log10_p[0])
    return {"seq": seq, "log_odds_ratio": log_odds_ratio(lp, k), "p_of_seq": 10.0 ** lp, "log10_p": lp}
