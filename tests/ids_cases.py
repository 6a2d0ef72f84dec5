"""Inputs and expected values for tests/test_gpu_ids_and_sweeps.py (checked themselves, on the CPU, by
tests/test_ids_cases_cpu.py).  Plain helpers, no fixtures: the window-id path (shred_kernel and the kernels around it)
is compared position by position with the oracle, on layouts that put record starts, N's and the end of the buffer on
every side of shred_kernel's tile and chunk edges.
"""
import numpy as np

T = 16384                 # residues per workgroup of shred_kernel (kdb_kernels.hip.h: TILE_BYTES)
CHUNK = 16                # residues per staged chunk; a tile also stages one halo chunk of the next tile
EDGE_REACH = 17           # |d| <= 17: one chunk and one residue on either side of an edge
NO_WINDOW = np.uint64(0xFFFFFFFFFFFFFFFF)
MAX_EXTRA = 300           # ragged records have k .. k + MAX_EXTRA residues
RAGGED_TOTAL = 3 * T + 39                       # two whole chunks and 7 residues behind the third edge: a partial last chunk
UNIFORM_LENGTHS = (5, 15, 16, 17, 31, 150, T - 1, T, T + 1)       # and k itself
SINGLE_LENGTHS = (15, 16, 17, T - 1, T, T + 1, 2 * T + 9)         # and k itself

_ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
_N = 78


class Layout:
    """One batch: residues, record offsets, and where its forced N's are."""

    def __init__(self, name, bases, offsets, forced_n=()):
        self.name = name
        self.bases = bases
        self.offsets = np.asarray(offsets, dtype=np.uint64)
        self.forced_n = tuple(forced_n)

    @property
    def total(self):
        return int(self.bases.size)

    @property
    def lengths(self):
        return np.diff(self.offsets.astype(np.int64))

    def __repr__(self):
        return "Layout({0}, {1} residues, {2} records)".format(self.name, self.total, len(self.offsets) - 1)


# ---------------------------------------------------------------------------------------------------------------
# A. expected ids
# ---------------------------------------------------------------------------------------------------------------

def expected_window_ids(bases, offsets, k, canon):
    """uint64[nbytes]: the id of the window that starts at each residue, NO_WINDOW where the reference emits none
    (the window holds an N, or runs past its record's end) -- what oracle.c_shred(record, k, canon, N_DROP) returns,
    record by record.  c_shred's own C function (kdbo_shred) is called on each record where it lies in the buffer, into
    one pair of output arrays: a batch of 30 000 records of a residue or two costs two Python-level copies per record
    otherwise.  Raises OracleError like c_shred."""
    import ctypes
    from oracle import kmer_oracle
    lib = kmer_oracle.lib()
    bases = np.ascontiguousarray(bases, dtype=np.uint8)
    offs = [int(x) for x in offsets]
    want = np.full(bases.size, NO_WINDOW, dtype=np.uint64)
    cap = max([e - s for s, e in zip(offs[:-1], offs[1:])] + [1])
    ids, pos = np.zeros(cap, dtype=np.uint64), np.zeros(cap, dtype=np.uint64)
    p_ids, p_pos = ids.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), pos.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))
    base = bases.ctypes.data if bases.size else 0
    u8p = ctypes.POINTER(ctypes.c_uint8)
    n = ctypes.c_uint64(0)
    for r, (s, e) in enumerate(zip(offs[:-1], offs[1:])):
        rc = lib.kdbo_shred(ctypes.cast(base + s, u8p), e - s, k, int(canon), kmer_oracle.N_DROP, p_ids, p_pos, cap, ctypes.byref(n))
        if rc != kmer_oracle.OK:
            raise kmer_oracle.OracleError(rc, r)
        want[s + pos[:n.value].astype(np.int64)] = ids[:n.value]
    return want


def describe_mismatch(got, want, offsets):
    """'' if equal, else where the first difference lies: position, record, distance to the nearest tile and chunk edge."""
    diff = np.flatnonzero(got != want)
    if diff.size == 0:
        return ""
    p = int(diff[0])
    offs = np.asarray(offsets, dtype=np.int64)
    r = int(np.searchsorted(offs, p, side="right")) - 1
    dt = p - T * int(round(p / T))
    dc = p - CHUNK * int(round(p / CHUNK))
    return ("{0} of {1} positions differ; first at {2}: got {3:#x}, want {4:#x}; record {5} = [{6}, {7}) (position {8} of it); "
            "{9:+d} from the nearest tile edge, {10:+d} from the nearest chunk edge"
            .format(diff.size, got.size, p, int(got[p]), int(want[p]), r, int(offs[r]), int(offs[r + 1]), p - int(offs[r]), dt, dc))


# ---------------------------------------------------------------------------------------------------------------
# B. layouts
# ---------------------------------------------------------------------------------------------------------------

def random_bases(rng, n, p_n=0.0):
    b = _ACGT[rng.integers(0, 4, size=n)].copy()
    if p_n:
        b[rng.random(n) < p_n] = _N
    return b


def cut_records(rng, lo, hi, k):
    """record starts that cut [lo, hi) into records of k .. k + MAX_EXTRA residues (hi - lo is 0 or at least k)."""
    assert hi == lo or hi - lo >= k, (lo, hi, k)
    starts, at = [], lo
    while at < hi:
        starts.append(at)
        rem = hi - at
        at = hi if rem <= k + MAX_EXTRA else at + int(rng.integers(k, min(k + MAX_EXTRA, rem - k) + 1))
    return starts


def straddle_lead(k, d):
    """how many residues of a layout's k-residue record lie before the third tile edge (0 for k = 1: it sits at the edge)."""
    return 1 + d % (k - 1) if k > 1 else 0


def ragged_layout(k, d, seed=0):
    """RAGGED_TOTAL residues in records of k .. k + MAX_EXTRA.  Records start at T + d and at 2 T - d; a record of exactly
    k residues straddles 3 T (and, for 0 < d < k, another one ends at T + d and so straddles T); N's at T + (17 - d) and
    2 T - (17 - d), and sprinkled at 0.3 % everywhere but in the record across 3 T."""
    assert 0 <= d <= EDGE_REACH and 1 <= k <= 17
    rng = np.random.Generator(np.random.PCG64(1000003 * k + 101 * d + seed))
    a = straddle_lead(k, d)
    points = {0, T + d, 2 * T - d, 3 * T - a, 3 * T - a + k, RAGGED_TOTAL}
    if 0 < d < k:
        points.add(T + d - k)
    points = sorted(points)
    starts = []
    for lo, hi in zip(points[:-1], points[1:]):
        starts += cut_records(rng, lo, hi, k)
    offsets = np.array(starts + [RAGGED_TOTAL], dtype=np.uint64)
    bases = random_bases(rng, RAGGED_TOTAL, 0.003)
    e = EDGE_REACH - d
    forced = (T + e, 2 * T - e)
    bases[list(forced)] = _N
    bases[3 * T - a:3 * T - a + k] = random_bases(rng, k)
    return Layout("ragged k={0} d={1}".format(k, d), bases, offsets, forced)


def short_ragged_layout(k, total, seed=0):
    """`total` residues (T - 1, T, T + 1: the buffer ends just before, at and just behind a tile edge), N's at 0.5 %."""
    rng = np.random.Generator(np.random.PCG64(7919 * k + total + seed))
    offsets = np.array(cut_records(rng, 0, total, k) + [total], dtype=np.uint64)
    return Layout("ragged k={0} total={1}".format(k, total), random_bases(rng, total, 0.005), offsets)


def ragged_family(k):
    return [ragged_layout(k, d) for d in range(EDGE_REACH + 1)] + [short_ragged_layout(k, t) for t in (T - 1, T, T + 1)]


def uniform_lengths(k):
    return sorted({k} | {L for L in UNIFORM_LENGTHS if L >= k})


def uniform_layout(k, L, seed=0):
    """records of L residues each, more than two tiles of them, N's at 0.5 %."""
    assert L >= k
    rng = np.random.Generator(np.random.PCG64(65537 * k + L + seed))
    nrec = 2 * T // L + 1
    offsets = np.arange(nrec + 1, dtype=np.uint64) * np.uint64(L)
    return Layout("uniform k={0} L={1}".format(k, L), random_bases(rng, nrec * L, 0.005), offsets)


def rebatch_ragged(layout, k):
    """The same residues with one record a residue longer, so that the batch no longer has one length and the engine
    marks its record starts.  The record behind gives the residue up; where it has only k (L = k) it is joined with
    the one after it instead, so that no record falls below k."""
    offs = layout.offsets.astype(np.int64)
    nrec = len(offs) - 1
    L = int(offs[1] - offs[0])
    b = max(1, nrec // 2)
    assert nrec >= 2 and b < nrec
    out = offs.copy()
    out[b] += 1
    if L - 1 < k:
        assert b + 1 < nrec
        out = np.delete(out, b + 1)
    return Layout(layout.name + " rebatched", layout.bases, out.astype(np.uint64))


def single_lengths(k):
    return sorted({k} | {L for L in SINGLE_LENGTHS if L >= k})


def single_record(k, L, seed=0):
    rng = np.random.Generator(np.random.PCG64(31337 * k + L + seed))
    return random_bases(rng, L, 0.005).tobytes()


# ---------------------------------------------------------------------------------------------------------------
# coverage of a family of layouts (asserted by the CPU tests)
# ---------------------------------------------------------------------------------------------------------------

def edge_distances(positions, total):
    """{d : |d| <= EDGE_REACH and some position lies at m T + d for a tile edge m T, m >= 1, of a buffer of `total` residues}."""
    out = set()
    pos = np.asarray(list(positions), dtype=np.int64)
    for m in range(1, (total + EDGE_REACH) // T + 1):
        d = pos - m * T
        out |= set(int(x) for x in d[np.abs(d) <= EDGE_REACH])
    return out


def coverage(layouts, k):
    """what a family of layouts reaches: record starts and N's by distance from a tile edge, chunk offsets of record
    starts, N-free records of exactly k residues across (k = 1: at) a tile edge, total lengths."""
    cov = {"start_d": set(), "n_d": set(), "start_chunk_offset": set(), "k_records_on_an_edge": 0, "totals": set()}
    for lay in layouts:
        offs = lay.offsets.astype(np.int64)
        starts = offs[:-1]
        cov["start_d"] |= edge_distances(starts, lay.total)
        cov["n_d"] |= edge_distances(np.flatnonzero(lay.bases == _N), lay.total)
        cov["start_chunk_offset"] |= set(int(x) for x in starts % CHUNK)
        cov["totals"].add(lay.total)
        for s, e in zip(offs[:-1], offs[1:]):
            if e - s != k or np.any(lay.bases[s:e] == _N):
                continue
            edge = (int(e) - 1) // T * T                    # the last tile edge at or before the record's last residue
            if edge >= T and (s < edge if k > 1 else s == edge):
                cov["k_records_on_an_edge"] += 1
    return cov


# ---------------------------------------------------------------------------------------------------------------
# files for the graph tests
# ---------------------------------------------------------------------------------------------------------------

def graph_records(kind, seed=0):
    """[(seq_id, seq)] without N: 'uniform' / 'ragged' reads of about 60 KB in all (FASTQ), or 'long': three records
    longer than a tile (FASTA)."""
    rng = np.random.Generator(np.random.PCG64(271828 + seed))
    if kind == "uniform":
        lens = [150] * 400
    elif kind == "ragged":
        lens = [int(x) for x in rng.integers(30, 271, size=400)]
    elif kind == "long":
        lens = [T + 1, T + 2 * CHUNK + 3, T + 4000]
    else:
        raise ValueError(kind)
    return [("{0}{1}".format(kind[0], i), random_bases(rng, n).tobytes().decode("ascii")) for i, n in enumerate(lens)]


def write_fastq(path, records):
    with open(path, "w") as f:
        for name, seq in records:
            f.write("@{0} test read\n{1}\n+\n{2}\n".format(name, seq, "I" * len(seq)))


def write_fasta(path, records, width=70):
    with open(path, "w") as f:
        for name, seq in records:
            f.write(">{0} test record\n".format(name))
            for i in range(0, len(seq), width):
                f.write(seq[i:i + width] + "\n")
