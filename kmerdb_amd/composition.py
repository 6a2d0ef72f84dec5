"""One small k-mer table per record, counted on the device: kdb_record_tables (csrc/kdb_tables.hip.h).

record_tables is that call on a batch of records; tables_file streams a FASTA/FASTQ file through it and joins the pieces of records
longer than a reader block; composition prints the k-mer composition of every record (k = 4, canonical: the tetranucleotide vector that
metagenomic binners start from).  kmerdb_amd.codons builds the reference's codon tables on the same call (k = 3, stride 3).
A window starts every `stride` residues from the record's first; one that holds an N is skipped and the frame is kept.  Residues outside
upper-case ACGTN are refused.  There is no CPU fallback: without a device these raise.
"""
import ctypes
import sys

import numpy as np

from . import _abi, _records

MAX_K = _abi.KDB_TABLES_MAX_K
MAX_CALL_ENTRIES = 1 << 26                 # table entries (records x 4^k) tables_file asks of one call: 256 MiB of uint32
_MAX_ENTRIES = 1 << 31


def _check_scalars(k, stride, phase, continues):
    for name, v in (("k", k), ("stride", stride), ("phase", phase)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise TypeError("kmerdb_amd.composition: {0} must be an int, not {1}".format(name, type(v).__name__))
    k, stride, phase = int(k), int(stride), int(phase)
    if not 1 <= k <= MAX_K:
        raise ValueError("kmerdb_amd.composition: k={0} out of range 1..{1}".format(k, MAX_K))
    if not 1 <= stride <= k:
        raise ValueError("kmerdb_amd.composition: stride={0} out of range 1..k={1}".format(stride, k))
    if not 0 <= phase < stride:
        raise ValueError("kmerdb_amd.composition: phase={0} must lie in 0..stride-1".format(phase))
    if phase and not continues:
        raise ValueError("kmerdb_amd.composition: a phase is for a record that continues the previous call's last one")
    return k, stride, phase


def record_tables_raw(bases, offsets, k, stride, canonical, phase, continues, device=0):
    """kdb_record_tables on checked arguments -> (tables, windows, skipped, first_id, last_id, kernel_ms)."""
    nreads = int(offsets.size) - 1
    tables = np.empty((nreads, 4 ** k), dtype=np.uint32)
    windows, skipped = (np.empty(nreads, dtype=np.uint64) for _ in range(2))
    first, last = (np.empty(nreads, dtype=np.int32) for _ in range(2))
    ms = ctypes.c_double(0.0)
    _abi.check(_abi.lib().kdb_record_tables(int(device), int(k), int(stride), 1 if canonical else 0, int(phase), bases.ctypes.data if bases.size else None,
                                            int(bases.size), offsets.ctypes.data, nreads, _abi.KDB_TABLES_CONTINUES if continues else 0,
                                            tables.ctypes.data, windows.ctypes.data, skipped.ctypes.data, first.ctypes.data, last.ctypes.data,
                                            ctypes.byref(ms)))
    return tables, windows, skipped, first, last, ms.value


def record_tables(bases, offsets, k, stride=1, canonical=False, phase=0, continues=False, device=0):
    """A k-mer table per record of a batch -> (tables: uint32[n, 4^k], windows, skipped: uint64[n], first_id, last_id: int32[n]).

    bases / offsets: the concatenated residues and the nreads + 1 record offsets, as Engine.submit takes them.  The windows of a record
    start at 0, stride, 2 stride, ...; tables[r, id] counts those of id `id` (canonical: min(id, rc(id)), the row stays 4^k wide),
    windows[r] all of them, skipped[r] those that hold an N; first_id / last_id are the ids of the first and the last counted window
    (-1 without one).  continues / phase: record 0 is the next piece of the previous call's last record, begins with its last k - 1
    residues, and its first window starts at `phase` (KDB_TABLES_CONTINUES).  A record shorter than k is a row of zeros.
    ValueError for what the call refuses: a residue outside upper-case ACGTN, more than 2^31 table entries."""
    k, stride, phase = _check_scalars(k, stride, phase, continues)
    bases, offsets = _records.check_batch("composition", bases, offsets)
    if (int(offsets.size) - 1) * 4 ** k > _MAX_ENTRIES:
        raise ValueError("kmerdb_amd.composition: more than 2^31 table entries (records x 4^k) in one call")
    from .distance import _require_device
    _require_device(device)
    return record_tables_raw(bases, offsets, k, stride, canonical, phase, continues, device)[:5]


def window_count(length, k, stride, phase=0):
    """how many windows a record (or a piece) of `length` residues has, its first one at `phase`"""
    return (length - k - phase) // stride + 1 if length >= k + phase else 0


class _Row:
    """a record under way: what its pieces so far add up to, and where in it the next piece's first window starts"""
    __slots__ = ("id", "length", "windows", "skipped", "first_id", "last_id", "table", "piece_at", "piece_len", "next_window")

    def __init__(self, rid, length, windows, skipped, first_id, last_id, table, k, stride):
        self.id, self.length, self.windows, self.skipped, self.first_id, self.last_id = rid, length, windows, skipped, first_id, last_id
        self.table = table.astype(np.uint64)
        self.piece_at, self.piece_len = 0, length                             # the piece's first residue in the record, its length
        self.next_window = window_count(length, k, stride) * stride            # the record position of the first window not yet seen

    def next_piece(self, piece_len, k):
        """a piece of piece_len residues follows: it repeats the last k - 1 residues (all, if fewer) of the piece before -> its phase"""
        self.piece_at += self.piece_len - min(k - 1, self.piece_len)
        self.piece_len = piece_len
        self.length = self.piece_at + piece_len
        return self.next_window - self.piece_at

    def join(self, phase, windows, skipped, first_id, last_id, table, k, stride):
        self.next_window = self.piece_at + phase + window_count(self.piece_len, k, stride, phase) * stride
        self.windows += windows
        self.skipped += skipped
        if self.first_id < 0:
            self.first_id = first_id
        if last_id >= 0:
            self.last_id = last_id
        self.table += table

    def astuple(self):
        return (self.id, self.length, self.windows, self.skipped, self.first_id, self.last_id, self.table)


def tables_file(seqfile, k, stride=1, canonical=False, device=0, block_bytes=None):
    """Every record of a FASTA/FASTQ file: yields (id, length, windows, skipped, first_id, last_id, table: uint64[4^k]) per record, in
    file order.  A FASTA record longer than a reader block arrives in pieces that repeat k - 1 residues: they are counted with
    KDB_TABLES_CONTINUES, each with the phase that keeps the record's frame, and joined here in uint64.  A block of many records goes to
    the device in calls of at most MAX_CALL_ENTRIES table entries."""
    from . import reader
    if type(seqfile) is not str:
        raise TypeError("kmerdb_amd.composition.tables_file expects the sequence file as a str filepath")
    k, stride, _ = _check_scalars(k, stride, 0, False)
    rd = reader.BlockReader(seqfile, want_ids=True, block_bytes=block_bytes, overlap=k - 1)
    per_call = max(1, MAX_CALL_ENTRIES >> (2 * k))
    pending = None
    for block in rd:
        bases, offsets, ids = block
        cont = bool(getattr(block, "cont", False)) and pending is not None
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        nrec = int(offsets.size) - 1
        for a in range(0, nrec, per_call):
            b = min(nrec, a + per_call)
            lo, hi = int(offsets[a]), int(offsets[b])
            first_continues = cont and a == 0
            phase = pending.next_piece(int(offsets[1]) - int(offsets[0]), k) if first_continues else 0
            tables, windows, skipped, first, last = record_tables(bases[lo:hi], offsets[a:b + 1] - np.uint64(lo), k, stride, canonical, phase=phase,
                                                                  continues=first_continues, device=device)
            lens = np.diff(offsets[a:b + 1].astype(np.int64))
            for r in range(b - a):
                if r == 0 and first_continues:
                    pending.join(phase, int(windows[0]), int(skipped[0]), int(first[0]), int(last[0]), tables[0], k, stride)
                    continue
                if pending is not None:
                    yield pending.astuple()
                pending = _Row(ids[a + r], int(lens[r]), int(windows[r]), int(skipped[r]), int(first[r]), int(last[r]), tables[r], k, stride)
    if pending is not None:
        yield pending.astuple()


def printed_columns(k, canonical):
    """the ids whose columns `composition` prints: all 4^k, or, canonical, those with id <= rc(id)"""
    ids = np.arange(4 ** k, dtype=np.uint64)
    if not canonical:
        return ids
    rc, x = np.zeros_like(ids), ids.copy()
    for _ in range(k):
        rc = (rc << np.uint64(2)) | (np.uint64(3) - (x & np.uint64(3)))
        x >>= np.uint64(2)
    return ids[ids <= rc]


def composition(seqfile, k, canonical=True, as_frequencies=False, output_delimiter="\t", out=None, device=0, block_bytes=None):
    """The `composition` subcommand: a header line (id, length, windows, then the k-mer of every printed column), then one line per
    record -- counts, or with as_frequencies count / windows as repr(float) prints it, nan for a record without a window.  Canonical:
    only the columns with id <= rc(id) (136 at k = 4; the others are zero).  -> the number of records."""
    from . import kmer
    out = sys.stdout if out is None else out
    k, _, _ = _check_scalars(k, 1, 0, False)
    cols = printed_columns(k, canonical)
    out.write(output_delimiter.join(["id", "length", "windows"] + [kmer.id_to_kmer(int(c), k) for c in cols]) + "\n")
    n = 0
    for rid, length, windows, _, _, _, table in tables_file(seqfile, k, stride=1, canonical=canonical, device=device, block_bytes=block_bytes):
        row = table[cols]
        if as_frequencies:
            fields = [repr(float(c) / windows) if windows else "nan" for c in row.tolist()]
        else:
            fields = [str(c) for c in row.tolist()]
        out.write(output_delimiter.join([str(rid), str(length), str(windows)] + fields) + "\n")
        n += 1
    return n
