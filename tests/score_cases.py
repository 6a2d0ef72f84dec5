"""The oracle, the error bound and the inputs of tests/test_gpu_score.py (checked themselves, on the CPU, by tests/test_score_cpu.py).

Written from the definition of the score and from nothing in kmerdb_amd: ids by plain loops, the integer outputs
exactly, log10_p in 50-digit decimals.

The score.  v: the 4^k counts, a: the pseudocount, total' = total + a 4^k.  A window is scored iff it lies whole inside its record and
its k residues are all of A, C, G, T.  c(w) = v[id] + a (canonical: v[min(id, rc(id))] + a); D(w) = the sum of c over the four k-mers
that share w's first k - 1 residues.  The first scored window of a record contributes ln c - ln total', every later one ln c - ln D;
a window with c = 0 contributes -inf.  log10_p = (the sum) / ln 10, None here (nan on the device) without a scored window.

The bound (`bound`).  u = 2^-53.  A term t = ln c - ln D is computed from two integers converted to float64 (a relative error of u each,
so u each in the logarithm), two logarithms within 1 ulp of a value up to L (<= 2 u L each, the accuracy DESIGN section 13 assumes) and
one subtraction (<= u |t|): e_t = u (2 + 2 |ln c| + 2 |ln D| + |t|).  A term then passes through at most
    depth = PIECE / LANES        (a lane's terms of one piece, added in a row)
          + log2(LANES)          (the butterfly over the wave)
          + 2 x pieces           (every piece adds its first term and its sum to the record's)
          + 3 x joins            (KDB_SCORE_CONTINUES: a further call cuts a piece of its own, and the host adds the call's result)
additions, each with a relative error of u on a partial sum that is at most Sum |t| in size: depth x u x Sum |t|.  The division by ln 10 and the rounding of that constant add
2 u |log10_p|.  Second-order terms are covered by a factor 1 + 2^-20.  PIECE and LANES are read from include/kdbhip.h by the tests.
"""
import decimal
import functools
import math

import numpy as np

U = 2.0 ** -53
TOP = 2 ** 64 - 1
CTX = decimal.Context(prec=50)
LN10 = CTX.ln(decimal.Decimal(10))
_CODE = {65: 0, 67: 1, 71: 2, 84: 3}          # A C G T
_LN = {}


def ln(v):
    v = int(v)
    if v not in _LN:
        _LN[v] = CTX.ln(decimal.Decimal(v))
    return _LN[v]


def rc_id(i, k):
    """reverse complement of an id: its k two-bit digits reversed, each d replaced by 3 - d"""
    out = 0
    for _ in range(k):
        out = (out << 2) | (3 - (i & 3))
        i >>= 2
    return out


def window_ids(seq, k):
    """the id of the window at every start 0 .. len - k of one record, None where a residue is not one of ACGT"""
    seq = bytes(seq)
    out = []
    for p in range(len(seq) - k + 1):
        wid = 0
        for c in seq[p:p + k]:
            if c not in _CODE:
                wid = None
                break
            wid = wid * 4 + _CODE[c]
        out.append(wid)
    return out


def kmer_id(kmer):
    (wid,) = window_ids(kmer.encode() if isinstance(kmer, str) else kmer, len(kmer))
    return wid


def id_kmer(i, k):
    return "".join("ACGT"[(i >> (2 * (k - 1 - j))) & 3] for j in range(k))


class Score:
    """one record: log10_p (Decimal; float('-inf'); None without a scored window), the three exact integers, and what the bound needs"""

    def __init__(self):
        self.log10_p, self.windows, self.zero_windows, self.min_count = None, 0, 0, TOP
        self.all_windows = 0          # windows of the record, scored or not
        self.abs_sum = 0.0            # Sum |t| over the finite terms
        self.log_mass = 0.0           # Sum |ln c| + |ln D| over them
        self.terms = []               # (c, D) per scored window, D = total' for an initial term


def score_record(seq, v, k, canonical, total, a=0, continues=False):
    """the definition, by plain loops -> Score"""
    n = 4 ** k
    assert len(v) == n
    look = (lambda i: int(v[min(i, rc_id(i, k))])) if canonical else (lambda i: int(v[i]))
    total2 = int(total) + a * n
    out = Score()
    ids = window_ids(seq, k)
    out.all_windows = len(ids)
    acc, infinite, first = decimal.Decimal(0), False, not continues
    for wid in ids:
        if wid is None:
            continue
        raw = look(wid)
        c = raw + a
        d = total2 if first else sum(look((wid & ~3) + x) + a for x in range(4))
        first = False
        out.windows += 1
        out.zero_windows += raw == 0
        out.min_count = min(out.min_count, raw)
        out.terms.append((c, d))
        if c == 0:
            infinite = True
            continue
        with decimal.localcontext(CTX):
            t = ln(c) - ln(d)
            acc += t
        out.abs_sum += abs(float(t))
        out.log_mass += abs(float(ln(c))) + abs(float(ln(d)))
    if out.windows:
        with decimal.localcontext(CTX):
            out.log10_p = float("-inf") if infinite else acc / LN10
    return out


def score_reads_stub(bases, offsets, vector, k, canonical, total, pseudocount=0, continues=False, device=0, none_scored=False):
    """the restatement behind the signature of kmerdb_amd.probability.score_reads, `vector` the counts on the host: the CPU tests put it
    in the device call's place.  A continuing record 0 before which nothing was scored (none_scored) takes the initial term: that is
    score_record's plain form.  log10_p is the exact sum rounded once."""
    raw = bytes(bases)
    o = [int(x) for x in offsets]
    out = []
    for r in range(len(o) - 1):
        rec = raw[o[r]:o[r + 1]]
        goes_on = bool(continues) and r == 0
        if (len(rec) < k and not goes_on) or set(rec) - set(b"ACGTN"):
            raise ValueError("a record shorter than k, or a residue outside ACGTN")
        s = score_record(rec, vector, k, canonical, total, pseudocount, continues=goes_on and not none_scored)
        out.append((float("nan") if s.log10_p is None else float(s.log10_p), s.windows, s.zero_windows, s.min_count))
    return (np.array([x[0] for x in out], dtype=np.float64),) + tuple(np.array([x[i] for x in out], dtype=np.uint64) for i in (1, 2, 3))


def float64_log10_p(score):
    """the same formula in plain float64 numpy, terms in window order; nan / -inf as the device gives them"""
    if not score.terms:
        return float("nan")
    if any(c == 0 for c, _ in score.terms):
        return float("-inf")
    c = np.array([float(c) for c, _ in score.terms], dtype=np.float64)
    d = np.array([float(d) for _, d in score.terms], dtype=np.float64)
    return float(np.sum(np.log(c) - np.log(d)) / np.log(np.float64(10.0)))


def pieces_of(all_windows, piece):
    return max(1, -(-all_windows // piece))


def bound(score, piece, lanes, joins=0):
    """the largest |device log10_p - true log10_p| the roundings allow for a finite record (module docstring)"""
    assert score.log10_p is not None and score.log10_p != float("-inf")
    depth = piece // lanes + int(math.log2(lanes)) + 2 * pieces_of(score.all_windows, piece) + 3 * joins
    per_term = U * (2.0 * score.windows + 2.0 * score.log_mass + score.abs_sum)
    return ((per_term + depth * U * score.abs_sum) / math.log(10.0) + 2.0 * U * abs(float(score.log10_p))) * (1.0 + 2.0 ** -20)


def error(got, score):
    """|got - true| as a float, for a finite record"""
    with decimal.localcontext(CTX):
        return float(abs(decimal.Decimal(float(got)) - score.log10_p))


# ---------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------

def pack(records):
    """[bytes] -> (bases: uint8[n], offsets: uint64[len + 1])"""
    offsets = np.zeros(len(records) + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum([len(r) for r in records], dtype=np.uint64)
    return np.frombuffer(b"".join(records), dtype=np.uint8).copy(), offsets


def random_record(rng, n, p_n=0.0):
    b = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=n)].copy()
    if p_n:
        b[rng.random(n) < p_n] = 78
    return b.tobytes()


def forward_profile(records, k):
    """the forward counts of the records' scored windows -> (v: uint64[4^k], total)"""
    v = np.zeros(4 ** k, dtype=np.uint64)
    for r in records:
        for wid in window_ids(r, k):
            if wid is not None:
                v[wid] += np.uint64(1)
    return v, int(v.sum())


def canonical_profile(records, k):
    v, total = forward_profile(records, k)
    out = np.zeros_like(v)
    for i in np.flatnonzero(v):
        i = int(i)
        out[min(i, rc_id(i, k))] += v[i]
    return out, total


def symmetrised(v, k):
    """sym[i] = v[min(i, rc(i))]: forward scoring of it is canonical scoring of v"""
    return np.array([v[min(i, rc_id(i, k))] for i in range(4 ** k)], dtype=np.uint64)


def length_ladder(k, piece):
    """record lengths that give 1 (k residues), 2, 63, 64, 65, PIECE - 1, PIECE, PIECE + 1 and 2 PIECE + 1 windows"""
    return [w + k - 1 for w in (1, 2, 63, 64, 65, piece - 1, piece, piece + 1, 2 * piece + 1)]


def layout_edges(k, piece):
    """the batches at the edges of kdb_score_reads' piece layout -> (record lengths, continues, short records, pieces of every record)"""
    one, two = piece + k - 1, piece + k                # `piece` windows, and one more
    return [([0], False, 1, [1]), ([0], True, 0, [1]),
            ([k - 1], False, 1, [1]), ([k - 1], True, 0, [1]), ([k - 1, k - 1], True, 1, [1, 1]),          # (only record 0 may continue)
            ([one], False, 0, [1]), ([two], False, 0, [2]), ([one, two], False, 0, [1, 2]), ([two, one], False, 0, [2, 1]),
            ([k, k, one, two], False, 0, [1, 1, 1, 2])]                                                # only the last record is cut


def ladder_records(k, piece, seed, p_n=0.0):
    rng = np.random.default_rng(seed)
    return [random_record(rng, n, p_n) for n in length_ladder(k, piece)]


def n_records(k):
    """N at position 0, at the last position, and spaced so that no window is N-free"""
    rng = np.random.default_rng(77 + k)
    body = random_record(rng, 3 * k + 5)
    every = bytearray(random_record(rng, 4 * k + 3))
    every[k - 1::k] = b"N" * len(every[k - 1::k])
    return [b"N" + body, body + b"N", bytes(every), b"N" * k, body]


def ragged_records(k, seed, n=40, p_n=0.01):
    rng = np.random.default_rng(seed)
    return [random_record(rng, int(rng.integers(k, k + 300)), p_n) for _ in range(n)]


def spread_vector(k, seed):
    """counts of every size: zeros, small counts, a few near 2^40 and at the top"""
    rng = np.random.default_rng(seed)
    n = 4 ** k
    v = rng.poisson(5.0, n).astype(np.uint64)
    v[rng.random(n) < 0.1] = 0
    big = rng.integers(0, n, max(1, n // 50))
    v[big] = rng.integers(2 ** 39, 2 ** 41, big.size).astype(np.uint64)
    return v


N_ACCURACY_CASES = 8


@functools.lru_cache(maxsize=2)
def accuracy_cases(piece):
    """[(name, k, canonical, v, total, a, records)]: finite records for the log10_p bound -- every length of the ladder and the N layouts
    against the forward profile counted from those same records, a canonical profile, a vector of counts of every size under a
    pseudocount, and four neighbouring bins at 2^64 - 1 (D needs 66 bits)."""
    cases = []
    for k in (1, 2, 3, 8):
        records = ladder_records(k, piece, 100 + k, p_n=0.002) + n_records(k)
        v, total = forward_profile(records, k)
        cases.append(("own forward profile k=%d" % k, k, False, v, total, 0, records))
    k = 5
    records = ragged_records(k, 5) + ladder_records(k, piece, 55)[-2:]
    v, total = canonical_profile(records, k)
    cases.append(("own canonical profile k=5", k, True, v, total, 0, records))
    k = 6
    v = spread_vector(k, 6)
    cases.append(("counts of every size, pseudocount 1, k=6", k, False, v, int(v.sum()), 1, ragged_records(k, 66) + ladder_records(k, piece, 67)[-1:]))
    k = 3
    v = np.arange(1, 65, dtype=np.uint64)
    v[20:24] = np.uint64(TOP)
    v[40:44] = np.array([TOP, TOP - 1, 1, TOP], dtype=np.uint64)
    spelled = [id_kmer(i, k).encode() for i in (20, 21, 22, 23, 40, 41, 42, 43)]
    records = spelled + [b"".join(spelled), id_kmer(20, k).encode() * 30]
    cases.append(("four bins at the top, k=3", k, False, v, TOP, 0, records))
    cases.append(("four bins at the top under a pseudocount, k=3", k, False, v, TOP - 64 * 5, 5, records))
    assert len(cases) == N_ACCURACY_CASES
    return cases


# ---------------------------------------------------------------------------------------------------------------
# the decode's edges at k = 14 .. 17: the last of the five 32-bit words a window arrives in, at every byte alignment
# ---------------------------------------------------------------------------------------------------------------
_NEXT = {"A": "C", "C": "G", "G": "T", "T": "A"}
DECODE_EDGE_ROLES = ("alone", "last", "r13", "r12", "n_after", "n_last", "n_after_more", "inside", "ends_buffer")


def decode_edge_kmers(k):
    """{name: k-mer}: K ends in T behind eight residues that are not T (so no residue 1 .. 7 places before the last equals the last);
    `last`, `r13`, `r12`: K with its last residue, residue 13 and residue 12 (from 0) replaced -- at k = 14 residue 13 is the last"""
    assert 14 <= k <= 17
    K = "TGCATGCA"[:k - 9] + "CAGGACGA" + "T"
    swap = lambda s, i: s[:i] + _NEXT[s[i]] + s[i + 1:]
    return {"K": K, "last": swap(K, k - 1), "r13": swap(K, 13), "r12": swap(K, 12)}


def decode_edge_records(k, alignment, seed=0, start=0):
    """-> (records, {role: index of its record}): every record with a role starts at a byte offset of the packed buffer that is
    `alignment` modulo 8 (a filler record before each sees to that; `start`: the bytes of the records a caller packs before these), and
    its window of interest is the one at its start:
        alone, last, r13, r12   the k-mers of decode_edge_kmers, one window each
        n_after                 K N: the N lies one past the window's end, the window is scored (and the next one is not)
        n_last                  K with N for its last residue: no window
        n_after_more            K N K: two scored windows around k that are not
        inside                  K `last` K: the three k-mers and the junk between them, at every alignment from here on
        ends_buffer             K as the last record of the buffer: its window ends where the buffer does"""
    rng = np.random.default_rng(1000 * k + 10 * alignment + seed)
    kmers = decode_edge_kmers(k)
    K = kmers["K"]
    body = {"alone": K, "last": kmers["last"], "r13": kmers["r13"], "r12": kmers["r12"], "n_after": K + "N", "n_last": K[:-1] + "N",
            "n_after_more": K + "N" + K, "inside": K + kmers["last"] + K, "ends_buffer": K}
    records, roles, at = [], {}, start
    for role in DECODE_EDGE_ROLES:
        n = k + (alignment - at - k) % 8
        records.append(random_record(rng, n))
        at += n
        assert at % 8 == alignment
        roles[role] = len(records)
        records.append(body[role].encode())
        at += len(body[role])
    return records, roles
