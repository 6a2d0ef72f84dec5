"""A model of where kdb_spectrum and kdb_rank_transform put a bin, and inputs built from it that reach what one grid stride never
reaches: the second and third iteration of both kernels' chunk loops in every value tier, partial merges of tally(), the wave-uniform
fast path decided by a single value in each of its four operands, the overflow list at and past the first sweep's guess, a binary
search over a million distinct values, and ranks of 2^32 and more (tests/test_spectrum_cases_cpu.py proves on the CPU that every case
is where it claims to be; tests/test_gpu_spectrum_deep.py runs the cases on the device).  Plain numpy and Python integers.

The map, as csrc/kdb_spectrum.hip.h has it.  A workgroup is four waves; a wave steps through chunks of 256 bins with two 16-byte loads
per lane: lane l holds bins 2 l and 2 l + 1 of its chunk (a.x, a.y: slots 0, 1) and bins 128 + 2 l and 128 + 2 l + 1 (b.x, b.y: slots
2, 3).  For a bin b below body = (nbins // 256) * 256:
    chunk = b // 256      wave = chunk % 4      workgroup = (chunk // 4) % grid      iteration = chunk // (4 grid)
    r = b % 256           lane = (r % 128) // 2                                      slot = 2 (r // 128) + r % 2
grid = min(KDB_SPECTRUM_GRID_MAX, ceil(nchunks / 4)).  The bins from body on are the tail: workgroup 0 after its loop, thread t the bin
body + t.  A value goes by its size: below NPRIV a counter per lane, below LDS_BINS the workgroup's LDS histogram, below DENSE the global
table, from DENSE on the overflow list; rank_map_kernel reads the ranks of values below RANK_LDS from LDS, below DENSE from the global
table and finds the others by binary search."""
import collections
import functools
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_constant(name):
    text = open(os.path.join(ROOT, "include", "kdbhip.h")).read()
    return int(re.search(r"#define\s+%s\s+(\d+)" % name, text).group(1))


CHUNK = 256                                        # bins of a wave's step
WAVES = 4                                          # waves of a workgroup
SLOTS = ("a.x", "a.y", "b.x", "b.y")
DENSE = header_constant("KDB_SPECTRUM_DENSE")
WG_BINS = header_constant("KDB_SPECTRUM_WG_BINS")
GRID_MAX = header_constant("KDB_SPECTRUM_GRID_MAX")
GUESS = header_constant("KDB_SPECTRUM_LIST_GUESS")
NPRIV, LDS_BINS, RANK_LDS = 16, 4096, 2048         # the tier edges of csrc/kdb_spectrum.hip.h (constants of the kernels, not of the interface)
assert WG_BINS == WAVES * CHUNK

TOP = 2 ** 64 - 1
TAIL = 77
STRIDE2 = 2 * GRID_MAX * WG_BINS + WG_BINS + TAIL  # every workgroup two iterations, workgroup 0 a third, and a tail
Where = collections.namedtuple("Where", "chunk wave workgroup iteration lane slot")


class Layout:
    """where the bins of one sweep of either kernel go"""

    def __init__(self, nbins, cap=GRID_MAX):
        self.nbins = nbins
        self.nchunks = nbins // CHUNK
        self.body = self.nchunks * CHUNK
        self.grid = max(1, min(cap, (self.nchunks + WAVES - 1) // WAVES))
        self.iterations = max(1, (self.nchunks + WAVES * self.grid - 1) // (WAVES * self.grid))

    def where(self, b):
        """-> Where of a body bin, None for a bin of the tail"""
        assert 0 <= b < self.nbins
        if b >= self.body:
            return None
        chunk, r = b // CHUNK, b % CHUNK
        return Where(chunk, chunk % WAVES, (chunk // WAVES) % self.grid, chunk // (WAVES * self.grid), (r % 128) // 2, 2 * (r // 128) + r % 2)

    def chunk_of(self, iteration, workgroup, wave):
        assert 0 <= workgroup < self.grid and 0 <= wave < WAVES
        chunk = (iteration * self.grid + workgroup) * WAVES + wave
        assert chunk < self.nchunks, "no such chunk in this shape"
        return chunk

    def bin(self, iteration, workgroup, wave, lane, slot):
        assert 0 <= lane < 64 and 0 <= slot < 4
        return self.chunk_of(iteration, workgroup, wave) * CHUNK + 128 * (slot // 2) + 2 * lane + slot % 2

    def slot_bins(self, chunk, slot):
        """the 64 bins that the lanes 0 .. 63 hold in one slot of a chunk, in lane order"""
        return chunk * CHUNK + 128 * (slot // 2) + 2 * np.arange(64) + slot % 2

    def iteration_of(self, bins):
        """vectorised; -1 for the tail's bins"""
        bins = np.asarray(bins, dtype=np.int64)
        return np.where(bins < self.body, bins // CHUNK // (WAVES * self.grid), -1)

    def later_bins(self):
        """the bins of iteration 1 and later, and the tail's"""
        return np.arange(min(WAVES * self.grid * CHUNK, self.body), self.nbins)


LAY = Layout(STRIDE2)


# ---------------------------------------------------------------------------------------------------------------
# what is expected
# ---------------------------------------------------------------------------------------------------------------
def expected_spectrum(v):
    """-> (values ascending, how many bins hold each), both uint64"""
    values, mult = np.unique(v, return_counts=True)
    return values.astype(np.uint64), mult.astype(np.uint64)


def expected_ranks(v):
    """2 below + eq + 1 of every bin"""
    _, inv, cnt = np.unique(v, return_inverse=True, return_counts=True)
    below = np.concatenate([[0], np.cumsum(cnt)[:-1]])
    return (2 * below + cnt + 1)[inv.reshape(-1)].astype(np.uint64)


def segment_ranks(values, lengths):
    """the same for a vector given as runs: values[i] repeated lengths[i] times -> (the doubled mid-rank of every run as Python integers,
    the spectrum as ([value], [multiplicity]))"""
    mult = collections.Counter()
    for x, n in zip(values, lengths):
        mult[int(x)] += int(n)
    rank, below = {}, 0
    for x in sorted(mult):
        rank[x] = 2 * below + mult[x] + 1
        below += mult[x]
    return [rank[int(x)] for x in values], (sorted(mult), [mult[x] for x in sorted(mult)])


# ---------------------------------------------------------------------------------------------------------------
# the cases: name -> (vector, claims); claims is what tests/test_spectrum_cases_cpu.py checks with the map
# ---------------------------------------------------------------------------------------------------------------
def background(rng, n=STRIDE2):
    """a read set's sparsity, every value below NPRIV: most bins empty, small counts elsewhere"""
    return np.minimum(rng.poisson(2.0, n) * (rng.integers(0, 8, n) == 0), NPRIV - 1).astype(np.uint64)


TIER_VALUES = {                                    # a few values of every tier above the per-lane counters
    "lds": [NPRIV, 100, LDS_BINS - 1],
    "global": [LDS_BINS, 5000, DENSE - 1],
    "list": [DENSE, 2 ** 32 + 5, TOP],
}
PLANT_WORKGROUPS = (0, 1, 517 % GRID_MAX, GRID_MAX - 1)


def _plant_later(v, values, rng):
    """every value in iteration 1 of several workgroups, in iteration 2 (workgroup 0's third) and in the tail; scattered over iteration 1
    as well -> {value: [bins placed by hand]}"""
    placed = {}
    for i, x in enumerate(values):
        bins = []
        for n, wg in enumerate(PLANT_WORKGROUPS):
            for rep in range(3):
                bins.append(LAY.bin(1, wg, (i + n) % WAVES, (11 * i + 5 * rep + n) % 64, (i + rep) % 4))
        for wave in range(WAVES):
            bins.append(LAY.bin(2, 0, wave, (7 * i + wave) % 64, (i + wave) % 4))
        bins.append(LAY.body + (5 * i) % TAIL)
        bins.append(LAY.body + (5 * i + 66) % TAIL)                          # (a lane of the tail's second wave among them)
        v[bins] = np.uint64(x)
        placed[x] = bins
    later = LAY.later_bins()
    free = np.setdiff1d(later, np.concatenate(list(placed.values())))
    pick = rng.choice(free, free.size // 50, replace=False)
    v[pick] = np.array(values, dtype=np.uint64)[rng.integers(0, len(values), pick.size)]
    return placed


def case_second_iteration():
    rng = np.random.default_rng(1101)
    v = background(rng)
    values = [x for tier in ("lds", "global", "list") for x in TIER_VALUES[tier]]
    return v, {"placed": _plant_later(v, values, rng), "values": values}


def case_table_edges_later():
    rng = np.random.default_rng(1102)
    v = background(rng)
    values = [RANK_LDS - 1, RANK_LDS, RANK_LDS + 1, DENSE - 1, DENSE, NPRIV, LDS_BINS - 1, LDS_BINS]
    return v, {"placed": _plant_later(v, values, rng), "values": values}


# what a merge claim says of the 64 lanes of one slot of one chunk, found again from the vector by merge_facts()
Merge = collections.namedtuple("Merge", "iteration workgroup wave slot tier shared")


def merge_facts(v, chunk, slot):
    """of the lanes that take tally()'s middle branch (NPRIV <= value < DENSE) in this slot: (how many, the first of them, how many hold
    the first one's value, that value), and how many lanes take the first and the third branch"""
    vals = v[LAY.slot_bins(chunk, slot)]
    mid = np.flatnonzero((vals >= NPRIV) & (vals < DENSE))
    first = int(mid[0]) if mid.size else None
    shared = int(np.count_nonzero(vals[mid] == vals[first])) if mid.size else 0
    return mid.size, first, shared, (int(vals[first]) if mid.size else None), int(np.count_nonzero(vals < NPRIV)), int(np.count_nonzero(vals >= DENSE))


SHARED_COUNTS = (2, 3, 17, 32, 62, 63)


def case_partial_merges():
    """waves of which a proper subset of 2 .. 63 lanes holds the first lane's value, in the LDS tier and in the global tier, in iteration 0
    and 1; and mixed waves whose lanes spread over all three branches of tally(), the first lane of the middle branch not lane 0"""
    rng = np.random.default_rng(1103)
    v = background(rng)
    merges, mixed = [], []
    sets = {"lds": np.arange(NPRIV, NPRIV + 25), "global": np.arange(LDS_BINS, LDS_BINS + 25)}
    n = 0
    for tier in ("lds", "global"):
        for iteration in (0, 1):
            for shared in SHARED_COUNTS:
                wg, wave, slot = (37 * n + 3) % GRID_MAX, n % WAVES, (n // 2) % 4
                pool = sets[tier]
                x0 = pool[n % pool.size]
                vals = rng.choice(pool[pool != x0], 64)
                same = np.concatenate([[0], 1 + rng.choice(63, shared - 1, replace=False)])
                vals[same] = x0
                v[LAY.slot_bins(LAY.chunk_of(iteration, wg, wave), slot)] = vals.astype(np.uint64)
                merges.append(Merge(iteration, wg, wave, slot, tier, shared))
                n += 1
    both = np.concatenate([sets["lds"], sets["global"]])
    for iteration in (0, 1):
        for first_lane in (1, 5, 40):
            for x0 in (int(sets["lds"][3]), int(sets["global"][3])):
                wg, wave, slot = (37 * n + 3) % GRID_MAX, n % WAVES, n % 4
                vals = np.empty(64, dtype=np.uint64)
                kind = rng.integers(0, 3, 64)                                # 0: below NPRIV, 1: the middle branch, 2: the list
                kind[:first_lane] = rng.choice([0, 2], first_lane)
                kind[first_lane] = 1
                kind[[61, 62, 63]] = [0, 1, 2]                               # (no branch is empty)
                vals[kind == 0] = rng.integers(0, NPRIV, np.count_nonzero(kind == 0)).astype(np.uint64)
                vals[kind == 1] = rng.choice(both[both != x0], np.count_nonzero(kind == 1)).astype(np.uint64)
                vals[kind == 2] = rng.choice(np.array([DENSE, DENSE + 1, 2 ** 40, TOP], dtype=np.uint64), np.count_nonzero(kind == 2))
                mid = np.flatnonzero(kind == 1)
                vals[mid[::3]] = np.uint64(x0)                               # the first of them and every third: a proper subset
                v[LAY.slot_bins(LAY.chunk_of(iteration, wg, wave), slot)] = vals
                mixed.append(Merge(iteration, wg, wave, slot, "lds" if x0 < LDS_BINS else "global", first_lane))
                n += 1
    return v, {"merges": merges, "mixed": mixed}


Single = collections.namedtuple("Single", "iteration workgroup wave lane slot value")
SINGLE_VALUES = (NPRIV, NPRIV + 1, 100, LDS_BINS, DENSE - 1, DENSE, 2 ** 40)


def _singles():
    out, n = [], 0
    for iteration in (0, 1):
        for wave in range(WAVES):
            for slot in range(4):
                out.append(Single(iteration, (29 * n + 1) % GRID_MAX, wave, (7 * n + 37) % 64, slot, SINGLE_VALUES[n % len(SINGLE_VALUES)]))
                n += 1
    for iteration in (0, 1):                                                 # NPRIV - 1 alone among zeros: still the fast path
        for wave in range(WAVES):
            for slot in range(4):
                out.append(Single(iteration, (29 * n + 1) % GRID_MAX, wave, (7 * n + 37) % 64, slot, NPRIV - 1))
                n += 1
    return out


def case_one_large_value(moved=0):
    """one value >= NPRIV in a wave whose other 255 values are below it, in each of the four slots in turn, waves 0 .. 3, iterations 0
    and 1; NPRIV - 1 alone among 255 zeros likewise.  moved=1: the same vector with every such value one slot further (the same lane)."""
    rng = np.random.default_rng(1104)
    v = background(rng)
    singles = _singles()
    assert len({(s.iteration, s.workgroup, s.wave) for s in singles}) == len(singles)
    for s in singles:
        chunk = LAY.chunk_of(s.iteration, s.workgroup, s.wave)
        if s.value < NPRIV:
            v[chunk * CHUNK:(chunk + 1) * CHUNK] = 0
        b = LAY.bin(s.iteration, s.workgroup, s.wave, s.lane, s.slot)
        v[b] = np.uint64(s.value)
        if moved:                                                            # (swapped with its neighbour: the same multiset of values)
            b2 = LAY.bin(s.iteration, s.workgroup, s.wave, s.lane, (s.slot + moved) % 4)
            v[[b, b2]] = v[[b2, b]]
    return v, {"singles": [s._replace(slot=(s.slot + moved) % 4) for s in singles]}


LIST_LENGTHS = (GUESS, GUESS + 1, GUESS + WG_BINS + 5)


def case_list_length(n_large):
    """exactly n_large values of DENSE and more, scattered over the whole vector: about every second bin, so nearly every wave reserves
    list entries for some of its lanes and the first sweep's list ends inside a wave's reservation"""
    rng = np.random.default_rng(1105)
    v = background(rng)
    at = rng.choice(STRIDE2, n_large, replace=False)
    pool = np.array([DENSE, DENSE + 1, DENSE + 2, 2 ** 32 - 1, 2 ** 32, 2 ** 40, TOP] + list(range(70000, 70400)), dtype=np.uint64)
    v[at] = pool[rng.integers(0, pool.size, n_large)]
    return v, {"n_large": n_large}


def case_many_distinct():
    """more than GUESS distinct values of DENSE and more: pairs that differ only above bit 32, pairs that differ only in the low 32 bits,
    2^64 - 1 and DENSE itself, some of them several times"""
    rng = np.random.default_rng(1106)
    v = background(rng)
    low = np.unique(rng.integers(DENSE, 2 ** 32, GUESS // 2 + 4000, dtype=np.uint64))
    high = rng.integers(1, 2 ** 31, low.size, dtype=np.uint64) << np.uint64(32)
    same_high = (np.uint64(7) << np.uint64(32)) + np.unique(rng.integers(0, 2 ** 32, 6000, dtype=np.uint64))
    distinct = np.unique(np.concatenate([low, low + high, same_high, np.array([DENSE, TOP, 2 ** 32, 2 ** 32 - 1], dtype=np.uint64)]))
    again = np.concatenate([rng.choice(distinct, 20000), np.repeat(rng.choice(distinct, 300), 3), np.array([DENSE, TOP, TOP], dtype=np.uint64)])
    large = np.concatenate([distinct, again])
    v[rng.choice(STRIDE2, large.size, replace=False)] = large
    return v, {"distinct": distinct.size, "low": low, "high_pairs": low + high, "same_high": same_high}


CASES = {
    "a_second_iteration_in_every_tier": case_second_iteration,
    "b_partial_merges": case_partial_merges,
    "c_one_large_value_per_wave": functools.partial(case_one_large_value, 0),
    "c_one_large_value_per_wave_moved_a_slot": functools.partial(case_one_large_value, 1),
    "d_list_length_guess": functools.partial(case_list_length, LIST_LENGTHS[0]),
    "d_list_length_guess_plus_1": functools.partial(case_list_length, LIST_LENGTHS[1]),
    "d_list_length_guess_plus_a_workgroup": functools.partial(case_list_length, LIST_LENGTHS[2]),
    "e_many_distinct_large_values": case_many_distinct,
    "f_table_edges_in_later_iterations": case_table_edges_later,
}


@functools.lru_cache(maxsize=2)
def case(name):
    """-> (vector, claims); the vector is not to be written to"""
    v, claims = CASES[name]()
    assert v.dtype == np.uint64 and v.shape == (STRIDE2,)
    v.setflags(write=False)
    return v, claims


# ---------------------------------------------------------------------------------------------------------------
# the wide cases: x[b] = T[b >> 20], built on the device
# ---------------------------------------------------------------------------------------------------------------
SEGMENT = 1 << 20
WIDE_LAST = WG_BINS + TAIL                         # bins of the last, short segment
WIDE_SEGMENTS = (2048, 4095)                       # whole segments: 2^31 + 1101 bins (16 GiB) and 2^32 - 2^20 + 1101 bins (32 GiB)


def wide_table(nfull):
    """-> (T: nfull + 1 segment values, lengths).  Not monotone, with repeats, in all four tiers, at the RANK_LDS and DENSE edges, some
    values of 2^32 and more.  Few segments hold listed values (the host sorts the list: 2^23 entries, not 2^30), one LDS-tier value holds
    42 % of the bins right across the middle of the ranks, and the last, short segment holds the largest value alone."""
    rng = np.random.default_rng(2049)
    listed = [DENSE, DENSE, DENSE + 1, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 1, 2 ** 40, 2 ** 63 + 5]
    n_low, n_lds_low, n_heavy, n_lds_high = (28 * nfull) // 100, (2 * nfull) // 100, (42 * nfull) // 100, (3 * nfull) // 100
    n_dense = nfull - n_low - n_lds_low - n_heavy - n_lds_high - len(listed)
    parts = [rng.choice([0, 1, 2, 7, NPRIV - 1], n_low), rng.choice([NPRIV, NPRIV + 1, 40], n_lds_low), np.full(n_heavy, 100),
             rng.choice([101, RANK_LDS - 2, RANK_LDS - 1], n_lds_high),
             rng.choice([RANK_LDS, RANK_LDS + 1, LDS_BINS - 1, LDS_BINS, LDS_BINS + 1, 5000, DENSE - 2, DENSE - 1], n_dense)]
    t = np.concatenate([np.asarray(p, dtype=np.uint64) for p in parts] + [np.array(listed, dtype=np.uint64)])
    rng.shuffle(t)
    t = np.concatenate([t, np.array([TOP], dtype=np.uint64)])
    lengths = [SEGMENT] * nfull + [WIDE_LAST]
    assert t.size == nfull + 1
    return t, lengths
