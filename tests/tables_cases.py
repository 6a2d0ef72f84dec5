"""The per-record k-mer tables of kdb_record_tables, restated in numpy from the definition in include/kdbhip.h (test infrastructure: the
product never imports this).

A record of `len` residues has the windows that start at p_i = phase + i stride for every i >= 0 with p_i + k <= len.  A window is
counted if its k residues are all of A, C, G, T and skipped if it holds an N.  The row has, per id, the number of counted windows
with that id (canonical: min(id, rc(id))); beside it the number of counted windows, of skipped ones, and the ids of the counted window
with the smallest and the largest p (-1 without one).  Residues are upper-case ACGTN: anything else is refused by the call, so
`record_table` raises on it.
"""
import numpy as np

CODE = np.full(256, -2, dtype=np.int64)
for _i, _c in enumerate(b"ACGT"):
    CODE[_c] = _i
CODE[ord("N")] = -1


def rc_ids(ids, k):
    """reverse complement of ids of k two-bit digits (A 0, C 1, G 2, T 3: the complement of d is 3 - d)"""
    ids = np.asarray(ids, dtype=np.int64)
    rc, x = np.zeros_like(ids), ids.copy()
    for _ in range(k):
        rc = (rc << 2) | (3 - (x & 3))
        x >>= 2
    return rc


def window_starts(length, k, stride, phase=0):
    return np.arange(phase, length - k + 1, stride, dtype=np.int64) if length >= k + phase else np.zeros(0, dtype=np.int64)


def record_table(rec, k, stride=1, canonical=False, phase=0):
    """-> (row: uint32[4^k], windows, skipped, first_id, last_id) of one record (bytes)"""
    codes = CODE[np.frombuffer(bytes(rec), dtype=np.uint8)]
    if np.any(codes == -2):
        raise ValueError("a residue outside ACGTN")
    p = window_starts(len(codes), k, stride, phase)
    row = np.zeros(4 ** k, dtype=np.uint32)
    if p.size == 0:
        return row, 0, 0, -1, -1
    w = codes[p[:, None] + np.arange(k)[None, :]]
    ok = np.all(w >= 0, axis=1)
    ids = (np.where(w >= 0, w, 0) * (4 ** np.arange(k - 1, -1, -1, dtype=np.int64))[None, :]).sum(axis=1)
    if canonical:
        ids = np.minimum(ids, rc_ids(ids, k))
    ids = ids[ok]
    row += np.bincount(ids, minlength=4 ** k).astype(np.uint32)
    return row, int(ids.size), int(p.size - ids.size), (int(ids[0]) if ids.size else -1), (int(ids[-1]) if ids.size else -1)


def batch_tables(records, k, stride=1, canonical=False, phase=0, continues=False):
    """what kdb_record_tables returns for the batch: (tables, windows, skipped, first_id, last_id); the phase is record 0's"""
    out = [record_table(r, k, stride, canonical, phase if (i == 0 and continues) else 0) for i, r in enumerate(records)]
    return (np.array([o[0] for o in out], dtype=np.uint32).reshape(len(records), 4 ** k), np.array([o[1] for o in out], dtype=np.uint64),
            np.array([o[2] for o in out], dtype=np.uint64), np.array([o[3] for o in out], dtype=np.int32), np.array([o[4] for o in out], dtype=np.int32))


def uniform_tables(block, k, stride=1, canonical=False):
    """batch_tables (phase 0) for records of one length, the rows of the uint8 array `block` (records x length): every window of every
    record in one array, the counts from one bincount over (record, id)"""
    block = np.asarray(block, dtype=np.uint8)
    n, length = block.shape
    codes = CODE.astype(np.int8)[block]                                       # (small types: the block may hold tens of megabytes)
    if np.any(codes == -2):
        raise ValueError("a residue outside ACGTN")
    p = window_starts(length, k, stride)
    none = np.full(n, -1, dtype=np.int32)
    if p.size == 0 or n == 0:
        return np.zeros((n, 4 ** k), dtype=np.uint32), np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint64), none, none.copy()
    ok = np.ones((n, p.size), dtype=bool)
    ids = np.zeros((n, p.size), dtype=np.int32)
    for j in range(k):
        c = codes[:, p + j]
        ok &= c >= 0
        ids = ids * 4 + np.maximum(c, 0)
    if canonical:
        ids = np.minimum(ids, rc_ids(ids, k).astype(np.int32))
    rows, cols = np.nonzero(ok)
    tables = np.bincount(rows * 4 ** k + ids[rows, cols], minlength=n * 4 ** k).astype(np.uint32).reshape(n, 4 ** k)
    windows = ok.sum(axis=1)
    at = np.arange(n)
    first = np.where(windows > 0, ids[at, np.argmax(ok, axis=1)], -1)
    last = np.where(windows > 0, ids[at, p.size - 1 - np.argmax(ok[:, ::-1], axis=1)], -1)
    return tables, windows.astype(np.uint64), (p.size - windows).astype(np.uint64), first.astype(np.int32), last.astype(np.int32)


def record_tables_stub(bases, offsets, k, stride=1, canonical=False, phase=0, continues=False, device=0):
    """the restatement behind the signature of kmerdb_amd.composition.record_tables: the CPU tests put it in the device call's place"""
    raw = bytes(bases)
    o = [int(x) for x in offsets]
    return batch_tables([raw[o[i]:o[i + 1]] for i in range(len(o) - 1)], k, stride, canonical, phase, continues)


def pack(records):
    """-> (bases: uint8[n], offsets: uint64[nreads + 1])"""
    bases = np.frombuffer(b"".join(bytes(r) for r in records), dtype=np.uint8).copy()
    offsets = np.zeros(len(records) + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum([len(r) for r in records])
    return bases, offsets


def random_record(rng, n, p_n=0.0):
    s = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=n)]
    if p_n > 0 and n:
        s = np.where(rng.random(n) < p_n, np.uint8(ord("N")), s)
    return s.astype(np.uint8).tobytes()


def length_for(nwin, k, stride):
    """the shortest record with nwin windows (phase 0)"""
    return 0 if nwin == 0 else (nwin - 1) * stride + k


def layout_edges(k, stride, piece):
    """the batches at the edges of kdb_record_tables' piece layout -> (record lengths, phase of record 0, windows of every record)"""
    one, two, ph = length_for(piece, k, stride), length_for(piece + 1, k, stride), stride - 1
    return [([0], 0, [0]), ([k - 1], 0, [0]), ([k - 1 + ph], ph, [0]), ([k + ph], ph, [1]),
            ([one], 0, [piece]), ([two], 0, [piece + 1]), ([one, two], 0, [piece, piece + 1]), ([two, one], 0, [piece + 1, piece]),
            ([k, k, one, two], 0, [1, 1, piece, piece + 1]),                                               # only the last record is cut
            ([one + ph, one], ph, [piece, piece]), ([two + ph, one], ph, [piece + 1, piece]),              # the phase is record 0's alone
            ([two, two], ph, [piece + (0 if ph else 1), piece + 1])]                                       # ... and can take its last window away


def ladder_records(k, stride, piece, seed, p_n=0.002):
    """Records at every edge of the kernel: 0, 1, k - 1, k, k + 1 residues, and 63, 64, 65, piece - 1, piece, piece + 1, 2 piece + 1
    windows (the last window's residues, then stride - 1 more that open no window), single-piece and multi-piece ones interleaved."""
    rng = np.random.Generator(np.random.PCG64(seed))
    small = [0, 1, k - 1, k, k + 1]
    wins = [63, 2 * piece + 1, 64, piece + 1, 65, piece - 1, piece, 2 * piece + 1, 3]
    recs = [random_record(rng, n) for n in small]
    for i, nw in enumerate(wins):
        recs.append(random_record(rng, length_for(nw, k, stride) + (stride - 1 if i % 2 else 0), p_n))
        if i % 3 == 0:
            recs.append(random_record(rng, small[i % len(small)]))
    return recs


def split_phase(cut, k, stride):
    """A record cut after `cut` residues into the piece [0, cut) and the piece that begins with its last min(k - 1, cut) residues:
    -> (where in the record the second piece begins, the phase of its first window).  The first piece holds the windows p with
    p + k <= cut; the next window of the record starts at the smallest multiple of the stride above cut - k."""
    begin = cut - min(k - 1, cut)
    nwin = (cut - k) // stride + 1 if cut >= k else 0
    return begin, nwin * stride - begin


def read_fasta(path):
    recs, rid, parts = [], None, []
    for line in open(path):
        line = line.strip()
        if line.startswith(">"):
            if rid is not None:
                recs.append((rid, "".join(parts)))
            rid, parts = line[1:].split()[0], []
        elif line:
            parts.append(line)
    recs.append((rid, "".join(parts)))
    return recs


def write_fasta(path, recs, wrap=60):
    with open(path, "w") as f:
        for rid, s in recs:
            f.write(">{0} words\n".format(rid) + "".join(s[i:i + wrap] + "\n" for i in range(0, len(s), wrap)))
    return str(path)
