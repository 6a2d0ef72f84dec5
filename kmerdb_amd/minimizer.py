"""The (w,k)-minimizers of every record, selected on the device: kdb_minimizers (csrc/kdb_minimizers.hip.h).

minimizers is that call on a batch of records; minimizers_file streams a FASTA/FASTQ file through it and joins the pieces of records
longer than a reader block; minimizers_table prints one line per minimizer (the `minimizers` subcommand).  Of every run of w consecutive
start positions the leftmost one with the smallest key is selected; the key of a position is its k-mer id (canonical: the smaller of
both strands') or, order="hashed", that id under an invertible mix, which spreads the selected positions where the sequence is of low
complexity.  A window that holds an N has no key.  Residues outside upper-case ACGTN are refused.  The reference's `minimizers`
(kmerdb/minimizer.py) flags every window_size-th of 4^k - k + 1 positions whatever the sequence; that is not reproduced.  There is no
CPU fallback: without a device these raise.
"""
import ctypes
import sys

import numpy as np

from . import _abi, _records

MAX_K, MAX_W = _abi.KDB_MINIMIZER_MAX_K, _abi.KDB_MINIMIZER_MAX_W
ORDERS = {"lexicographic": _abi.KDB_MINIMIZER_LEX, "hashed": _abi.KDB_MINIMIZER_HASHED}
SMALL_BATCH = 1 << 22                      # residues up to which the lists are sized for a minimizer at every position: no second call


def _check_scalars(k, w, order):
    for name, v in (("k", k), ("w", w)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise TypeError("kmerdb_amd.minimizer: {0} must be an int, not {1}".format(name, type(v).__name__))
    k, w = int(k), int(w)
    if not 1 <= k <= MAX_K:
        raise ValueError("kmerdb_amd.minimizer: k={0} out of range 1..{1}".format(k, MAX_K))
    if not 1 <= w <= MAX_W:
        raise ValueError("kmerdb_amd.minimizer: w={0} out of range 1..{1}".format(w, MAX_W))
    if not isinstance(order, str):
        raise TypeError("kmerdb_amd.minimizer: order must be a str, not {0}".format(type(order).__name__))
    if order not in ORDERS:
        raise ValueError("kmerdb_amd.minimizer: order={0!r} is neither 'lexicographic' nor 'hashed'".format(order))
    return k, w, ORDERS[order]


def minimizers_raw(bases, offsets, k, w, canonical, order, cap, device=0):
    """kdb_minimizers on checked arguments, the lists sized for `cap` minimizers -> (counts, ids, pos, strand, total, kernel_ms); the
    lists are None where total > cap."""
    nreads = int(offsets.size) - 1
    counts = np.zeros(nreads, dtype=np.uint64)
    ids, pos, strand = np.empty(cap, dtype=np.uint64), np.empty(cap, dtype=np.uint32), np.empty(cap, dtype=np.uint8)
    total, ms = ctypes.c_uint64(0), ctypes.c_double(0.0)
    _abi.check(_abi.lib().kdb_minimizers(int(device), int(k), int(w), 1 if canonical else 0, int(order), bases.ctypes.data if bases.size else None,
                                         int(bases.size), offsets.ctypes.data, nreads, counts.ctypes.data if nreads else None,
                                         ids.ctypes.data if cap else None, pos.ctypes.data if cap else None, strand.ctypes.data if cap else None, cap,
                                         ctypes.byref(total), ctypes.byref(ms)))
    n = int(total.value)
    if n > cap:
        return counts, None, None, None, n, ms.value
    return counts, ids[:n], pos[:n], strand[:n], n, ms.value


def list_capacity(nbytes, w):
    """the entries the lists get at the first call: one per residue in a small batch (a bound: no position is selected twice), else
    5/4 of what random sequence selects, 2 / (w + 1) of the positions; a batch that selects more is called once more with its total"""
    if nbytes <= SMALL_BATCH:
        return nbytes
    return min(nbytes, max(SMALL_BATCH, (5 * nbytes) // (2 * (w + 1)) + 1024))


def minimizers(bases, offsets, k, w, canonical=True, order="lexicographic", device=0):
    """The minimizers of every record of a batch -> (counts: uint64[n], ids: uint64[t], pos: uint32[t], strand: uint8[t]).

    bases / offsets: the concatenated residues and the nreads + 1 record offsets, as Engine.submit takes them.  Record r's minimizers
    are the entries [S_r, S_r + counts[r]) of the three lists, S the exclusive prefix sums of the counts, by ascending position: the
    k-mer id (canonical: the smaller of both strands'), the start position inside the record, and 1 where the id is the reverse
    strand's.  ValueError for what the call refuses: a residue outside upper-case ACGTN."""
    k, w, order = _check_scalars(k, w, order)
    bases, offsets = _records.check_batch("minimizer", bases, offsets)
    from .distance import _require_device
    _require_device(device)
    counts, ids, pos, strand, total, _ = minimizers_raw(bases, offsets, k, w, canonical, order, list_capacity(int(bases.size), w), device)
    if ids is None:
        counts, ids, pos, strand, total2, _ = minimizers_raw(bases, offsets, k, w, canonical, order, total, device)
        if ids is None:
            raise _abi.KdbHipError("kdb_minimizers: two calls on one batch found {0} and {1} minimizers".format(total, total2))
    return counts, ids, pos, strand


class _Open:
    """a record under way: the minimizers of its pieces so far, at record positions"""
    __slots__ = ("id", "length", "piece_at", "piece_len", "pos", "ids", "strand")

    def __init__(self, rid, length, pos, ids, strand):
        self.id, self.length, self.piece_at, self.piece_len = rid, length, 0, length
        self.pos, self.ids, self.strand = [pos.astype(np.int64)], [ids], [strand]

    def next_piece(self, piece_len, overlap, k, w):
        """a piece of piece_len residues follows: it repeats the last `overlap` residues of the piece before"""
        if self.piece_len < k + w - 1 or self.piece_len < overlap:
            raise ValueError("kmerdb_amd.minimizer: a piece of record {0!r} holds fewer than w = {1} windows: block_bytes is too small for "
                             "this file".format(self.id, w))
        self.piece_at += self.piece_len - overlap
        self.piece_len = piece_len
        self.length = self.piece_at + piece_len

    def join(self, pos, ids, strand):
        self.pos.append(pos.astype(np.int64) + self.piece_at)
        self.ids.append(ids)
        self.strand.append(strand)

    def astuple(self):
        if len(self.pos) == 1:
            return (self.id, self.length, self.pos[0], self.ids[0], self.strand[0])
        # the last w - 1 positions of a piece are the first of the next: a position both selected counts once
        pos, first = np.unique(np.concatenate(self.pos), return_index=True)
        return (self.id, self.length, pos, np.concatenate(self.ids)[first], np.concatenate(self.strand)[first])


def minimizers_file(seqfile, k, w, canonical=True, order="lexicographic", device=0, block_bytes=None):
    """Every record of a FASTA/FASTQ file: yields (id, length, pos: int64[], ids: uint64[], strand: uint8[]) per record, in file order.
    A FASTA record longer than a reader block arrives in pieces that repeat k + w - 2 residues, w - 1 start positions: every run of w
    positions then lies whole in one piece or the next, so the record's minimizers are the union of the pieces', each position once."""
    from . import reader
    if type(seqfile) is not str:
        raise TypeError("kmerdb_amd.minimizer.minimizers_file expects the sequence file as a str filepath")
    k, w, _ = _check_scalars(k, w, order)
    if block_bytes is not None:
        if isinstance(block_bytes, bool) or not isinstance(block_bytes, (int, np.integer)):
            raise TypeError("kmerdb_amd.minimizer: block_bytes must be an int")
        if block_bytes < 4 * (k + w):
            raise ValueError("kmerdb_amd.minimizer: block_bytes={0} is too small for a piece to hold w = {1} windows of k = {2} "
                             "(at least {3})".format(block_bytes, w, k, 4 * (k + w)))
    overlap = k + w - 2
    rd = reader.BlockReader(seqfile, want_ids=True, block_bytes=block_bytes, overlap=overlap)
    pending = None
    for block in rd:
        bases, offsets, ids = block
        cont = bool(getattr(block, "cont", False)) and pending is not None
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        nrec = int(offsets.size) - 1
        if cont:
            pending.next_piece(int(offsets[1]) - int(offsets[0]), overlap, k, w)
        counts, mids, mpos, mstrand = minimizers(bases, offsets, k, w, canonical=canonical, order=order, device=device)
        ends = np.cumsum(counts.astype(np.int64))
        lens = np.diff(offsets.astype(np.int64))
        for r in range(nrec):
            a, b = int(ends[r]) - int(counts[r]), int(ends[r])
            if r == 0 and cont:
                pending.join(mpos[a:b], mids[a:b].copy(), mstrand[a:b].copy())
                continue
            if pending is not None:
                yield pending.astuple()
            pending = _Open(ids[r], int(lens[r]), mpos[a:b], mids[a:b].copy(), mstrand[a:b].copy())
    if pending is not None:
        yield pending.astuple()


def minimizers_table(seqfile, k, w, canonical=True, order="lexicographic", out=None, device=0, block_bytes=None):
    """The `minimizers` subcommand: one line per minimizer, `seq_id<TAB>pos<TAB>kmer_id<TAB>+|-`, by record and position
    -> the number of minimizers."""
    out = sys.stdout if out is None else out
    n = 0
    for rid, _, pos, ids, strand in minimizers_file(seqfile, k, w, canonical=canonical, order=order, device=device, block_bytes=block_bytes):
        rid = str(rid)
        out.write("".join("{0}\t{1}\t{2}\t{3}\n".format(rid, p, i, "-" if s else "+") for p, i, s in zip(pos.tolist(), ids.tolist(), strand.tolist())))
        n += int(pos.size)
    return n
