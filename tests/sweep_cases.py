"""A model of where the analysis sweeps put a bin -- kdb_gram, kdb_pairstats / kdb_pairfloat, kdb_size_factors / kdb_scale_counts -- and
inputs built from it that reach what one grid stride never reaches: accumulators that live across loop iterations, the wave-uniform guards,
the carry of every reduction level, and the off-diagonal template instantiations (tests/test_sweep_cases_cpu.py proves on the CPU that every
case is where it claims to be; tests/test_gpu_sweeps_deep.py runs the cases on the device).  Plain numpy and Python integers.

The map, as kdb_gram.hip.h, kdb_pairstats.hip.h and kdb_sizefactors.hip.h have it.  A workgroup is four waves; a wave steps through chunks
of 128 bins, lane l holding bins 2 l and 2 l + 1 of its chunk (one 16-byte load: .x and .y); the workgroups of a row number gx.  For a
body bin b:
    chunk = b // 128      lane = (b % 128) // 2      half = b % 2
    wave = chunk % 4      workgroup = (chunk // 4) % gx      iteration = chunk // (4 gx)
gx = min(ceil(chunks / 4), cap), the caps stated in include/kdbhip.h: KDB_GRAM_GRID_MAX for kdb_gram and kdb_pairstats below
KDB_GRAM_GRID_MANY_ROWS rows, KDB_GRAM_GRID_MAX_MANY_ROWS from there on; KDB_PAIRFLOAT_GRID_MAX; KDB_SIZEFACTORS_GRID_MAX.  A row is one
launch row (blockIdx.y): a pair of blocks of four vectors in kdb_gram, a block against itself or against two (or one) vectors of a later
block in kdb_pairstats, one pair in kdb_pairfloat.  gram, pairstats and pairfloat sweep the whole chunks only: the bins from
(nbins // 128) * 128 on are a tail kernel's, one more partial of the row (nparts = gx + 1).  The size-factor kernels have no tail kernel:
their last, partial chunk goes through the body."""
import collections
import os
import re
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_gpu_gram as _tg  # noqa: E402        (the recipes of the tests written beside the kernels: imported, not copied)
import test_gpu_pairstats as _tp  # noqa: E402
import test_gpu_sizefactors as _ts  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_constant(name):
    text = open(os.path.join(ROOT, "include", "kdbhip.h")).read()
    return int(re.search(r"#define\s+%s\s+(\d+)" % name, text).group(1))


CHUNK = 128                                        # bins of a wave's step
WAVES = 4                                          # waves of a workgroup
B = header_constant("KDB_GRAM_BLOCK")
HALF = header_constant("KDB_PAIRSTATS_HALF")
WG_BINS = header_constant("KDB_GRAM_WG_BINS")
GRID_MAX = header_constant("KDB_GRAM_GRID_MAX")
GRID_MAX_MANY = header_constant("KDB_GRAM_GRID_MAX_MANY_ROWS")
MANY_ROWS = header_constant("KDB_GRAM_GRID_MANY_ROWS")
FLOAT_GRID_MAX = header_constant("KDB_PAIRFLOAT_GRID_MAX")
SF_GRID_MAX = header_constant("KDB_SIZEFACTORS_GRID_MAX")
assert WG_BINS == WAVES * CHUNK == header_constant("KDB_PAIRSTATS_WG_BINS") == header_constant("KDB_SIZEFACTORS_WG_BINS")
assert B == header_constant("KDB_PAIRSTATS_BLOCK") == 4 and HALF == 2

TOP = 2 ** 64 - 1
TAIL = 77                                          # bins behind the last whole chunk in every deep shape
Where = collections.namedtuple("Where", "chunk lane half wave workgroup iteration")


def deep_nbins(cap):
    """the smallest kind of shape that strides: every workgroup one iteration, the first a second one, and a tail"""
    return cap * WG_BINS + WG_BINS + TAIL


# ---------------------------------------------------------------------------------------------------------------
# the layout
# ---------------------------------------------------------------------------------------------------------------
class Layout:
    """where the bins of one sweep go; tail: the sweep has a tail kernel (else its partial chunk goes through the body)"""

    def __init__(self, nbins, cap, tail=True):
        self.nbins, self.has_tail = nbins, tail
        self.nchunks = nbins // CHUNK if tail else (nbins + CHUNK - 1) // CHUNK
        self.body = self.nchunks * CHUNK if tail else nbins                # bins below it go through the body's loop
        self.gx = max(1, min((self.nchunks + WAVES - 1) // WAVES, cap))
        self.nparts = self.gx + 1
        self.iterations = max(1, (self.nchunks + WAVES * self.gx - 1) // (WAVES * self.gx))

    def where(self, b):
        """-> Where of a body bin, None for a bin of the tail kernel"""
        assert 0 <= b < self.nbins
        if b >= self.body:
            return None
        chunk = b // CHUNK
        return Where(chunk, (b % CHUNK) // 2, b % 2, chunk % WAVES, (chunk // WAVES) % self.gx, chunk // (WAVES * self.gx))

    def bin(self, iteration, workgroup, wave, lane, half):
        assert 0 <= workgroup < self.gx and 0 <= wave < WAVES and 0 <= lane < 64 and half in (0, 1)
        b = ((iteration * self.gx + workgroup) * WAVES + wave) * CHUNK + 2 * lane + half
        assert b < self.body, "no such bin in this shape"
        return b

    def chunk_bins(self, chunk):
        return slice(chunk * CHUNK, min((chunk + 1) * CHUNK, self.body))

    def iteration_of(self, bins):
        """vectorised; -1 for the tail kernel's bins"""
        bins = np.asarray(bins, dtype=np.int64)
        return np.where(bins < self.body, bins // CHUNK // (WAVES * self.gx), -1)

    def second_stride(self):
        """the body bins of iteration 1 and later"""
        return np.arange(min(WAVES * self.gx * CHUNK, self.body), self.body)


# ---------------------------------------------------------------------------------------------------------------
# the row grouping: which template instantiation serves which pair
# ---------------------------------------------------------------------------------------------------------------
Row = collections.namedtuple("Row", "inst a b")       # inst = (NA, NB, DIAG); a, b: the vectors of the row's two sides
Served = collections.namedtuple("Served", "inst row slot passes")


def gram_rows(n):
    """kdb_gram's rows in launch order: the full diagonal blocks, the pairs of full blocks, then the short last block and the full
    blocks against it"""
    nblk = (n + B - 1) // B
    last = n - (nblk - 1) * B
    nfull = nblk if last == B else nblk - 1
    block = lambda b: tuple(range(b * B, min(n, b * B + B)))
    rows = [Row((B, B, True), block(b), block(b)) for b in range(nfull)]
    rows += [Row((B, B, False), block(bi), block(bj)) for bi in range(nfull) for bj in range(bi + 1, nfull)]
    if nfull < nblk:
        rows.append(Row((last, last, True), block(nfull), block(nfull)))
        rows += [Row((B, last, False), block(bi), block(nfull)) for bi in range(nfull)]
    return rows


def pair_rows(n):
    """kdb_pairstats' rows in launch order: the diagonal blocks, every earlier block against HALF vectors of a later one, then against
    the single vectors that are left"""
    nblk = (n + B - 1) // B
    size = lambda b: min(B, n - b * B)
    rows = [Row((size(b), size(b), True), tuple(range(b * B, b * B + size(b))), tuple(range(b * B, b * B + size(b)))) for b in range(nblk)]
    for want in (HALF, 1):
        for bj in range(1, nblk):
            for h in range(0, size(bj), HALF):
                nb = min(HALF, size(bj) - h)
                if nb != want:
                    continue
                for bi in range(bj):
                    rows.append(Row((B, nb, False), tuple(range(bi * B, bi * B + B)), tuple(range(bj * B + h, bj * B + h + nb))))
    return rows


def _served(rows, i, j):
    assert i < j
    hits = [(r, row) for r, row in enumerate(rows) if i in row.a and j in row.b]
    assert len(hits) == 1, "a pair has one row"
    r, row = hits[0]
    return r, row, (row.a.index(i), row.b.index(j))


def gram_served(n, i, j):
    """the instantiation, row and slot of pair i < j; passes: the (J0, NJ) of the second block's pass that holds j (off the diagonal)"""
    r, row, slot = _served(gram_rows(n), i, j)
    na, nb, diag = row.inst
    if diag:
        passes = None
    elif nb < B:
        passes = (0, min(nb, 2)) if slot[1] < 2 else (2, nb - 2)
    else:
        passes = (slot[1], 1)
    return Served(row.inst, r, slot, passes)


def pair_served(n, i, j):
    r, row, slot = _served(pair_rows(n), i, j)
    return Served(row.inst, r, slot, None)


def grid_cap(nrows):
    return GRID_MAX if nrows < MANY_ROWS else GRID_MAX_MANY


def gram_layout(n, nbins):
    return Layout(nbins, grid_cap(len(gram_rows(n))))


def pair_layout(n, nbins):
    return Layout(nbins, grid_cap(len(pair_rows(n))))


def float_layout(nbins):
    return Layout(nbins, FLOAT_GRID_MAX)


def sf_layout(nbins):
    return Layout(nbins, SF_GRID_MAX, tail=False)


# ---------------------------------------------------------------------------------------------------------------
# the expected integers, in limbs: a second formulation beside the object arrays of the tests written beside the kernels
# ---------------------------------------------------------------------------------------------------------------
_M16, _M32 = np.uint64(0xFFFF), np.uint64(0xFFFFFFFF)


def _limbs(v):
    return [((v >> np.uint64(16 * k)) & _M16) for k in range(4)]


def gram_expected(vs):
    """(S, G) as Python ints: 16-bit limbs, so that a dot product of limbs stays below 2^32 nbins and fits a word"""
    assert all(v.dtype == np.uint64 and v.size < 2 ** 31 for v in vs)
    n = len(vs)
    limbs = [_limbs(v) for v in vs]
    S = [sum(int(l.sum()) << (16 * k) for k, l in enumerate(ls)) for ls in limbs]
    G = [[0] * n for _ in range(n)]
    for i in range(n):
        for j in range(i, n):
            G[i][j] = G[j][i] = sum(int(np.dot(limbs[i][k], limbs[j][l])) << (16 * (k + l)) for k in range(4) for l in range(4))
    return S, G


def pair_expected(vs):
    """kdb_pairstats' integers: |x - y| without a wrap, summed in two 32-bit halves"""
    assert all(v.dtype == np.uint64 and v.size < 2 ** 31 for v in vs)
    n = len(vs)
    wide = lambda d: int((d & _M32).sum()) + (int((d >> np.uint64(32)).sum()) << 32)
    out = {"S": [wide(v) for v in vs], "nnz": [int(np.count_nonzero(v)) for v in vs]}
    for key in _tp.KEYS[2:]:
        out[key] = [[0] * n for _ in range(n)]
    for i in range(n):
        out["both"][i][i] = out["nnz"][i]
        for j in range(i + 1, n):
            x, y = vs[i], vs[j]
            d = np.where(x > y, x - y, y - x)
            vals = {"L1": wide(d), "Linf": int(d.max()), "ne": int(np.count_nonzero(d)), "both": int(np.count_nonzero((x != 0) & (y != 0)))}
            for key, v in vals.items():
                out[key][i][j] = out[key][j][i] = v
    return out


# ---------------------------------------------------------------------------------------------------------------
# a. kdb_gram: the guard between the short and the full multiply
# ---------------------------------------------------------------------------------------------------------------
GUARD_NS = (5, 6, 7, 8)                            # <4,1..4,false> and <1..4,1..4,true>
GUARD_VALUE = 2 ** 32 + 5


def gram_guard_case(n):
    """Every (vector, half) has a wave of its own -- chunk 2 v + half -- that holds exactly one value of 2^32 + 5, in that vector and that
    half of a lane; every other vector is small and non-zero at that bin, so a wave that took the 32-bit multiply there changes G.  All
    other values are below 2^32 (odd vectors up to 2^31: the short products' low words carry).  2 n + 4 chunks and 77 tail bins.
    -> (vectors, [(vector, half, bin)])"""
    nbins = (2 * n + 4) * CHUNK + TAIL
    rng = np.random.default_rng(4000 + n)
    vs = [(rng.integers(0, 2 ** 31, nbins) if v % 2 else rng.poisson(3.0, nbins) * rng.integers(0, 2, nbins)).astype(np.uint64) for v in range(n)]
    lay = gram_layout(n, nbins)
    placed = []
    for v in range(n):
        for half in (0, 1):
            chunk = 2 * v + half
            b = chunk * CHUNK + 2 * ((11 * chunk + 5) % 64) + half
            assert lay.where(b).chunk == chunk
            for w in range(n):
                vs[w][b] = np.uint64(GUARD_VALUE if w == v else 1 + (3 * w + chunk) % 13)
            placed.append((v, half, b))
    return vs, placed


# ---------------------------------------------------------------------------------------------------------------
# b. kdb_gram and kdb_pairstats across the stride, many rows
# ---------------------------------------------------------------------------------------------------------------
STRIDE_NS = (9, 10, 11, 12)                        # off the diagonal: <4,1,false>, <4,2,false>, <4,3,false>, <4,4,false> (and <4,4,false> always)
STRIDE_NBINS = deep_nbins(GRID_MAX_MANY)
CLASSES = ("small", "big32", "one_big", "big32b", "zeros", "late")
PLANT_FIRST = (37, 2, 21, 1)                       # (workgroup, wave, lane, half) in iteration 0: 2^32 + 5 + v, the least 64-bit operand
PLANT_FIRST_BIG = (200, 1, 50, 0)                  # in iteration 0: 2^61 + 3 v -- a product of 2^122 in one lane
PLANT_SECOND = (0, 3, 33, 0)                       # in iteration 1: 2^61 + v


def stride_class(n, v):
    """the rotation: with it every pair slot of every off-diagonal instantiation, kdb_gram's and kdb_pairstats', has a row, at some n of
    STRIDE_NS, whose two vectors are neither zeros nor late (test_sweep_cases_cpu.py counts them)"""
    return CLASSES[(n - v) % len(CLASSES)]


def stride_case(n):
    """n vectors of STRIDE_NBINS bins: workgroup 0 takes two iterations, the others one, and there is a tail.  The value classes of
    test_gpu_gram's test_values_zeros_carries_and_both_multiply_paths, by its recipe, rotated through the vector positions by n, and a
    sixth, `late`, whose only non-zero bins are second-iteration bins.  Every vector but the zeros holds 2^61 + v in one second-iteration
    bin, and every vector but the zeros and the late one 2^32 + 5 + v and 2^61 + 3 v in two first-iteration bins of other workgroups:
    where two such vectors meet, a lane's sum passes 2^64 (2^122) in the first iteration and again in the second.  Every sum stays below
    2^63.  -> (vectors, classes, the three planted bins)"""
    assert n in STRIDE_NS
    nbins = STRIDE_NBINS
    lay = gram_layout(n, nbins)
    assert lay.gx == pair_layout(n, nbins).gx == GRID_MAX_MANY
    rng = np.random.default_rng(5000 + n)
    counts = lambda: (rng.poisson(3.0, nbins) * rng.integers(0, 2, nbins)).astype(np.uint64)
    p0, p0b, p1 = lay.bin(0, *PLANT_FIRST), lay.bin(0, *PLANT_FIRST_BIG), lay.bin(1, *PLANT_SECOND)
    second = lay.second_stride()
    vs, classes = [], []
    for v in range(n):
        cls = stride_class(n, v)
        if cls == "zeros":
            x = np.zeros(nbins, dtype=np.uint64)
        elif cls == "big32":
            x = np.where(rng.integers(0, 2, nbins) == 1, np.uint64(2 ** 32 - 1), rng.integers(0, 2 ** 32, nbins, dtype=np.uint64)).astype(np.uint64)
        elif cls == "big32b":
            x = np.where(rng.integers(0, 3, nbins) > 0, np.uint64(2 ** 32 - 1), np.uint64(12345)).astype(np.uint64)
        elif cls == "one_big":
            x = counts()
            x[WG_BINS + 130 + 17] = np.uint64(2 ** 32 + 5)
        elif cls == "small":
            x = counts()
        else:
            x = np.zeros(nbins, dtype=np.uint64)
            x[second] = counts()[second] + np.uint64(1)
        if cls != "zeros":
            x[p1] = np.uint64(2 ** 61 + v)
            if cls != "late":
                x[p0], x[p0b] = np.uint64(2 ** 32 + 5 + v), np.uint64(2 ** 61 + 3 * v)
        vs.append(x)
        classes.append(cls)
    return vs, classes, (p0, p0b, p1)


# ---------------------------------------------------------------------------------------------------------------
# c. kdb_pairstats: the carry of L1 at every level, and S >= 2^64 inside one lane
# ---------------------------------------------------------------------------------------------------------------
PLACEMENTS = ("lane", "iterations", "lanes", "waves", "workgroups")
LADDER_NS = (7, 6)                                 # 7: <4,4,true>, <3,3,true>, <4,2,false> (both j), <4,1,false>; 6: <2,2,true>
LADDER_A, LADDER_B = (0, 4), (1, 5, 6)             # the vectors that hold 2^64 - 1 in bin a, in bin b; the others are noise


def ladder_nbins(n):
    return deep_nbins(grid_cap(len(pair_rows(n))))


def ladder_bins(lay, placement):
    """the two bins whose values meet at the named level first: in the lane's own sum within one chunk, in the lane's sum across two
    iterations, in the wave's shuffles, in the workgroup's LDS fold, in the combine kernel.  No lane 0: what a reduction drops from the
    lanes it shuffles in would else go unseen."""
    return {"lane": (lay.bin(0, 9, 2, 13, 0), lay.bin(0, 9, 2, 13, 1)),
            "iterations": (lay.bin(0, 0, 1, 29, 0), lay.bin(1, 0, 1, 29, 1)),
            "lanes": (lay.bin(0, 5, 2, 9, 1), lay.bin(0, 5, 2, 40, 0)),
            "waves": (lay.bin(0, 17, 1, 22, 0), lay.bin(0, 17, 3, 22, 1)),
            "workgroups": (lay.bin(0, 3, 0, 7, 1), lay.bin(0, lay.gx - 56, 2, 7, 0))}[placement]


def ladder_case(n, placement):
    """Vectors LADDER_A hold 2^64 - 1 in bin a and nothing else, LADDER_B the same in bin b (a sum may not reach 2^64: such a vector has
    no room for noise); the other vectors are small noise.  Every pair of one from each set has L1 = 2^65 - 2, Linf = 2^64 - 1, ne = 2,
    both = 0, and its two values meet where `placement` says; the pairs with a noise vector have L1 = 2^64 - 1 + noise.
    -> (vectors, a, b)"""
    nbins = ladder_nbins(n)
    lay = pair_layout(n, nbins)
    a, b = ladder_bins(lay, placement)
    rng = np.random.default_rng(6000 + 10 * n + PLACEMENTS.index(placement))
    vs = []
    for v in range(n):
        if v in LADDER_A or v in LADDER_B:
            x = np.zeros(nbins, dtype=np.uint64)
            x[a if v in LADDER_A else b] = np.uint64(TOP)
        else:
            x = (rng.poisson(3.0, nbins) * rng.integers(0, 2, nbins)).astype(np.uint64)
        vs.append(x)
    return vs, a, b


REFUSALS = ("lane", "iterations")
REFUSAL_N = 2


def refusal_case(placement):
    """[ones, v]: v holds 2^63 twice -- in the two bins of one lane and chunk, or in one lane's bins of two successive iterations -- and
    nothing else: S = 2^64 forms inside one lane's accumulator.  -> (vectors, the two bins)"""
    nbins = deep_nbins(grid_cap(len(pair_rows(REFUSAL_N))))
    lay = pair_layout(REFUSAL_N, nbins)
    assert lay.gx == gram_layout(REFUSAL_N, nbins).gx
    a, b = {"lane": (lay.bin(0, 11, 3, 41, 0), lay.bin(0, 11, 3, 41, 1)), "iterations": (lay.bin(0, 0, 2, 18, 1), lay.bin(1, 0, 2, 18, 0))}[placement]
    v = np.zeros(nbins, dtype=np.uint64)
    v[a] = v[b] = np.uint64(2 ** 63)
    return [np.ones(nbins, dtype=np.uint64), v], (a, b)


# ---------------------------------------------------------------------------------------------------------------
# d. kdb_pairfloat
# ---------------------------------------------------------------------------------------------------------------
FLOAT_DEEP_NBINS = deep_nbins(FLOAT_GRID_MAX)      # nparts = 513: the combine kernel's lanes take nine partials each
FLOAT_MID_NBINS = 100 * WG_BINS + TAIL             # nparts = 101: its loop runs twice in some lanes, once in the others
LONE_SECOND = ((0, 0), (2, 1))                     # the (vector, half) whose lone wave is a second-iteration chunk


def float_case(nbins):
    """test_gpu_pairstats' _float_vectors at nbins, with six waves emptied in all three vectors and given one non-zero word each: one per
    (vector, half).  For a pair i < j those of i are a wave whose only non-zero word is x.x, and one for x.y; those of j are y.x and y.y.
    At FLOAT_DEEP_NBINS the waves of LONE_SECOND are second-iteration chunks, so each pair has one of its four there.
    -> (vectors, {(vector, half): bin})"""
    lay = float_layout(nbins)
    vs = _tp._float_vectors(nbins, nbins)
    lone = {}
    free = iter(range(3, lay.gx, max(1, lay.gx // 7)))
    for v in range(3):
        for half in (0, 1):
            if lay.iterations > 1 and (v, half) in LONE_SECOND:
                b = lay.bin(1, 0, 1 + LONE_SECOND.index((v, half)), 17 + 5 * v, half)
            else:
                b = lay.bin(0, next(free), (v + half) % WAVES, 17 + 5 * v, half)
            lone[(v, half)] = b
    for (v, half), b in lone.items():
        chunk = lay.chunk_bins(lay.where(b).chunk)
        for x in vs:
            x[chunk] = 0
    for (v, half), b in lone.items():
        vs[v][b] = np.uint64(3 + v)
    assert int(vs[0][nbins // 3]) == 2 ** 40          # (the recipe's large count is not in an emptied wave)
    return vs, lone


# ---------------------------------------------------------------------------------------------------------------
# e. kdb_size_factors and kdb_scale_counts
# ---------------------------------------------------------------------------------------------------------------
SF_NBINS = deep_nbins(SF_GRID_MAX)
SF_MODES = ("first", "last", "between")


def grouped_case_deep(mode, seed):
    """test_gpu_sizefactors' _grouped_case at SF_NBINS with one change: the group of equal ratios that holds the median -- both groups,
    where the two middle ranks lie in different ones -- is made of exactly the eligible bins beyond the first grid stride, and every
    other group lies inside the first stride.  x is 8 and y is 8 * 2^t on the eligible bins, with t from T_VALUES in four groups.
    -> (x, y, the sorted t list, the eligible bins of the second stride)"""
    nbins = SF_NBINS
    lay = sf_layout(nbins)
    rng = np.random.default_rng(seed)
    inel = rng.random(nbins) < 0.25
    inel[0] = False
    inel[1] = inel[-1] = True
    if mode == "between" and (nbins - int(inel.sum())) % 2 == 1:
        inel[nbins // 2] = not inel[nbins // 2]
    m = nbins - int(inel.sum())
    lo, hi = (m - 1) // 2, m // 2
    second = lay.second_stride()
    deep = second[~inel[second]]                                           # the eligible bins of the second stride
    g = deep.size
    if mode == "first":
        cuts = [m // 5, lo, lo + g]                                        # the lower middle rank is the first of the deep group
    elif mode == "last":
        cuts = [m // 5, hi + 1 - g, hi + 1]                                # the upper middle rank is the last of it
    else:
        cuts = [hi - g // 2, hi, hi + (g - g // 2)]                        # two deep groups, the middle ranks on either side of the cut
    assert 1 <= cuts[0] < cuts[1] < cuts[2] <= m - 1
    ts = [_ts.T_VALUES[sum(1 for c in cuts if c <= i)] for i in range(m)]
    deep_ranks = range(cuts[1], cuts[2]) if mode != "between" else range(cuts[0], cuts[2])
    assert len(deep_ranks) == g and lo in deep_ranks and hi in deep_ranks
    rest = ts[:deep_ranks[0]] + ts[deep_ranks[-1] + 1:]
    value = lambda t: 8 * 2 ** t if t >= 0 else 8 >> -t
    x, y = np.full(nbins, 8, dtype=np.uint64), np.zeros(nbins, dtype=np.uint64)
    first_eligible = np.flatnonzero(~inel)
    first_eligible = first_eligible[first_eligible < second[0]]
    y[first_eligible] = [value(t) for t in rng.permutation(rest)]
    y[deep] = [value(ts[i]) for i in rng.permutation(list(deep_ranks))]
    zero_in_x = inel & (rng.random(nbins) < 0.5)
    x[zero_in_x] = 0
    y[inel & ~zero_in_x] = 0
    y[zero_in_x] = rng.integers(0, 3, int(zero_in_x.sum())).astype(np.uint64) * np.uint64(16)
    return x, y, ts, deep


SCALE_EDGE = (2 ** 53 - 1, 2 ** 53, 2 ** 53 + 1, 2 ** 53 + 3, 1, 3, 5, 7, 0, 2 ** 62 + 1, 2 ** 40 + 1)       # _scale_counts' edge values


def scale_case_deep(seed):
    """test_gpu_sizefactors' _scale_counts at SF_NBINS -- its edge values close the vector, in the partial chunk, which the second
    iteration of workgroup 1 takes -- and the same values again in a whole chunk of workgroup 0's second iteration, one per lane
    and in either half.  -> (v, the bins of the second copy)"""
    lay = sf_layout(SF_NBINS)
    v = _ts._scale_counts(SF_NBINS, seed)
    assert tuple(int(e) for e in v[-len(SCALE_EDGE):]) == SCALE_EDGE
    bins = [lay.bin(1, 0, 1, 20 + k, k % 2) for k in range(len(SCALE_EDGE))]
    v[bins] = np.array(SCALE_EDGE, dtype=np.uint64)
    return v, bins


def overflow_bins():
    """where a count of 2^64 - 1 (a quotient of 2^63 or more at s <= 2) must be found: the last bin of the partial chunk, a bin of a
    whole second-iteration chunk, bin 0"""
    lay = sf_layout(SF_NBINS)
    return {"last bin of the partial chunk": SF_NBINS - 1, "second iteration": lay.bin(1, 0, 2, 31, 1), "bin 0": 0}
