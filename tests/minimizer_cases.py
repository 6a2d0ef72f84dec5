"""The (w,k)-minimizers of kdb_minimizers, restated in numpy from the definition in include/kdbhip.h (test infrastructure: the product
never imports this).

A record of `len` residues has the start positions 0 .. nwin - 1, nwin = len - k + 1 (0 if len < k).  A position has an id iff its
window's k residues are all of A, C, G, T: the forward id, or canonical the smaller of it and its reverse complement's (strand 1 where
that is the reverse complement's).  Its key is the id, or the id under the mix `h`; a position without an id has key +infinity.  With
we = min(w, nwin): of every run of we consecutive positions whose smallest key is finite the leftmost position holding that key is
selected.  This is the RUN form, brute force over the runs; the kernel uses another form.
"""
import numpy as np

LEX, HASHED = 0, 1
INF = np.uint64(2 ** 64 - 1)

CODE = np.full(256, -2, dtype=np.int64)
for _i, _c in enumerate(b"ACGT"):
    CODE[_c] = _i
CODE[ord("N")] = -1


def h(x, k):
    """the invertible mix on [0, 4^k), every step masked (Python integers)"""
    m = 4 ** k - 1
    x = (~x + (x << 21)) & m
    x ^= x >> 24
    x = (x + (x << 3) + (x << 8)) & m
    x ^= x >> 14
    x = (x + (x << 2) + (x << 4)) & m
    x ^= x >> 28
    x = (x + (x << 31)) & m
    return x


def h_array(ids, k):
    """h on a uint64 array: 64-bit wrap-around loses nothing, every sum is masked to 2k <= 62 bits"""
    m = np.uint64(4 ** k - 1)
    u = np.uint64
    x = np.asarray(ids, dtype=np.uint64).copy()
    with np.errstate(over="ignore"):
        x = (~x + (x << u(21))) & m
        x ^= x >> u(24)
        x = (x + (x << u(3)) + (x << u(8))) & m
        x ^= x >> u(14)
        x = (x + (x << u(2)) + (x << u(4))) & m
        x ^= x >> u(28)
        x = (x + (x << u(31))) & m
    return x


def rc_ids(ids, k):
    """reverse complement of ids of k two-bit digits (A 0, C 1, G 2, T 3: the complement of d is 3 - d)"""
    x = np.asarray(ids, dtype=np.uint64).copy()
    rc = np.zeros_like(x)
    for _ in range(k):
        rc = (rc << np.uint64(2)) | (np.uint64(3) - (x & np.uint64(3)))
        x >>= np.uint64(2)
    return rc


def positions(rec, k, canonical):
    """-> (has_id: bool[nwin], ids: uint64[nwin], strand: uint8[nwin]) of one record (bytes); ids and strand are 0 where there is no id"""
    codes = CODE[np.frombuffer(bytes(rec), dtype=np.uint8)]
    if np.any(codes == -2):
        raise ValueError("a residue outside ACGTN")
    nwin = max(0, len(codes) - k + 1)
    if nwin == 0:
        return np.zeros(0, dtype=bool), np.zeros(0, dtype=np.uint64), np.zeros(0, dtype=np.uint8)
    has = np.ones(nwin, dtype=bool)
    fwd = np.zeros(nwin, dtype=np.uint64)
    for j in range(k):
        c = codes[j:j + nwin]
        has &= c >= 0
        fwd = (fwd << np.uint64(2)) | np.where(c >= 0, c, 0).astype(np.uint64)
    ids, strand = fwd, np.zeros(nwin, dtype=np.uint8)
    if canonical:
        rc = rc_ids(fwd, k)
        strand = (rc < fwd).astype(np.uint8)
        ids = np.minimum(fwd, rc)
    return has, np.where(has, ids, np.uint64(0)), np.where(has, strand, 0).astype(np.uint8)


def keys_of(has, ids, k, order):
    return np.where(has, h_array(ids, k) if order == HASHED else ids, INF)


def select_runs(keys, w):
    """the run form: keys uint64 with INF for none -> the sorted selected positions"""
    nwin = int(keys.size)
    if nwin == 0:
        return np.zeros(0, dtype=np.int64)
    we = min(w, nwin)
    runs = np.lib.stride_tricks.sliding_window_view(keys, we)                # run s = keys[s : s + we], s = 0 .. nwin - we
    arg = np.argmin(runs, axis=1)                                            # (the first occurrence of the minimum: the leftmost)
    s = np.arange(runs.shape[0], dtype=np.int64)
    finite = runs[s, arg] != INF
    return np.unique(s[finite] + arg[finite])


def select_runs_plain(keys, w):
    """select_runs in plain Python, run by run (for the small cases)"""
    keys = [int(x) for x in keys]
    nwin = len(keys)
    if nwin == 0:
        return []
    we, chosen = min(w, nwin), set()
    for s in range(nwin - we + 1):
        run = keys[s:s + we]
        m = min(run)
        if m != int(INF):
            chosen.add(s + run.index(m))
    return sorted(chosen)


def record_minimizers(rec, k, w, canonical=True, order=LEX):
    """-> (pos: int64[], ids: uint64[], strand: uint8[]) of one record (bytes)"""
    has, ids, strand = positions(rec, k, canonical)
    pos = select_runs(keys_of(has, ids, k, order), w)
    return pos, ids[pos], strand[pos]


def batch_minimizers(records, k, w, canonical=True, order=LEX):
    """what kdb_minimizers returns for the batch: (counts: uint64[n], ids: uint64[t], pos: uint32[t], strand: uint8[t])"""
    out = [record_minimizers(r, k, w, canonical, order) for r in records]
    cat = lambda i, dt: np.concatenate([o[i] for o in out]).astype(dt) if out else np.zeros(0, dtype=dt)
    return np.array([o[0].size for o in out], dtype=np.uint64), cat(1, np.uint64), cat(0, np.uint32), cat(2, np.uint8)


def minimizers_stub(bases, offsets, k, w, canonical=True, order="lexicographic", device=0):
    """the restatement behind the signature of kmerdb_amd.minimizer.minimizers: the CPU tests put it in the device call's place"""
    raw = bytes(bases)
    o = [int(x) for x in offsets]
    return batch_minimizers([raw[o[i]:o[i + 1]] for i in range(len(o) - 1)], k, w, canonical, {"lexicographic": LEX, "hashed": HASHED}[order])


def batch_minimizers_flat(bases, offsets, k, w, canonical=True, order=LEX):
    """batch_minimizers for many short records at once, where every record has no start position or at least w of them (so that
    every run is w positions long): the keys of all residues in one array, the runs of w of the whole array, and of those the ones
    that lie inside one record's start positions."""
    bases, o = np.asarray(bases, dtype=np.uint8), np.asarray(offsets, dtype=np.int64)
    n, nrec = int(bases.size), int(o.size) - 1
    lens = np.diff(o)
    nwin = np.maximum(lens - k + 1, 0)
    assert np.all((nwin == 0) | (nwin >= w))
    rec_of = np.repeat(np.arange(nrec), lens)                                 # the record of every residue
    starts = np.flatnonzero(np.arange(n) - o[rec_of] < nwin[rec_of])          # the residues where a start position lies
    codes = np.concatenate([CODE[bases], np.full(k, -1, dtype=np.int64)])
    assert not np.any(codes == -2)
    has = np.ones(starts.size, dtype=bool)
    fwd = np.zeros(starts.size, dtype=np.uint64)
    for j in range(k):
        c = codes[starts + j]
        has &= c >= 0
        fwd = (fwd << np.uint64(2)) | np.where(c >= 0, c, 0).astype(np.uint64)
    ids, strand = fwd, np.zeros(starts.size, dtype=np.uint8)
    if canonical:
        rc = rc_ids(fwd, k)
        strand, ids = (rc < fwd).astype(np.uint8), np.minimum(fwd, rc)
    keys = keys_of(has, ids, k, order)
    # `starts` lists the start positions record after record: a run of w entries lies in one record iff its ends do
    counts = np.zeros(nrec, dtype=np.uint64)
    if starts.size < w:
        return counts, np.zeros(0, dtype=np.uint64), np.zeros(0, dtype=np.uint32), np.zeros(0, dtype=np.uint8)
    runs = np.lib.stride_tricks.sliding_window_view(keys, w)
    arg = np.argmin(runs, axis=1)
    s = np.arange(runs.shape[0], dtype=np.int64)
    rec_at = rec_of[starts]
    good = (rec_at[s] == rec_at[s + w - 1]) & (runs[s, arg] != INF)
    chosen = np.unique(s[good] + arg[good])
    counts = np.bincount(rec_at[chosen], minlength=nrec).astype(np.uint64)
    return counts, ids[chosen], (starts[chosen] - o[rec_at[chosen]]).astype(np.uint32), strand[chosen]


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


def length_for(nwin, k):
    """the record length with nwin start positions"""
    return 0 if nwin == 0 else nwin + k - 1


def ladder_lengths(k, w, piece):
    small = [0, 1, k - 1, k, k + 1, k + w - 2, k + w - 1, k + w]
    wins = [piece - 1, piece, piece + 1, piece + w - 1, 2 * piece, 2 * piece + 1, 3 * piece - 1]
    return small + [length_for(n, k) for n in wins]


def layout_edges(k, piece):
    """the batches at the edges of kdb_minimizers' piece layout -> (record lengths, start positions of every record)"""
    one, two = length_for(piece, k), length_for(piece + 1, k)
    return [([0], [0]), ([k - 1], [0]), ([one], [piece]), ([two], [piece + 1]), ([one, two], [piece, piece + 1]), ([two, one], [piece + 1, piece]),
            ([k, k, one, two], [1, 1, piece, piece + 1])]                                                  # only the last record is cut


def ladder_records(k, w, piece, seed, p_n=0.001):
    """records at every edge of the kernel, single-piece and multi-piece ones interleaved"""
    rng = np.random.Generator(np.random.PCG64(seed))
    lengths = ladder_lengths(k, w, piece)
    order = [8, 0, 12, 1, 9, 2, 3, 13, 4, 10, 5, 14, 6, 11, 7]
    return [random_record(rng, lengths[i], p_n if lengths[i] > 64 else 0.0) for i in order]


def record_with_keys_at(rng, n, k, low):
    """a random record of n start positions over C, G, T whose window at every position of `low` is poly-A, the smallest id (k >= 2
    and the positions at least k + 1 apart): forward and lexicographic, those windows are the only ones that begin with k As"""
    s = bytearray(np.frombuffer(b"CGT", dtype=np.uint8)[rng.integers(0, 3, size=length_for(n, k))].tobytes())
    for p in low:
        s[p:p + k] = b"A" * k
    return bytes(s)


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


def read_fastq(path):
    lines = [line.strip() for line in open(path)]
    return [(lines[i][1:].split()[0], lines[i + 1]) for i in range(0, len(lines) - 3, 4) if lines[i].startswith("@")]
