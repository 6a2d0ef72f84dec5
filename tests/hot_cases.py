"""A model of the counting kernels' lane layout, and inputs built from it, for the "same id in many lanes" shortcuts
(tests/test_hot_cases_cpu.py asserts on the CPU that every case reaches the branch it names; tests/test_gpu_hot_ids.py runs the
cases on the engine).  Plain numpy; ids come from the oracle (ids_cases.expected_window_ids -> oracle.c_shred), never from a
second implementation.

The layout, as kmerdb_amd/csrc/kdb_scatter.hip.h has it (kdb_smallk.hip.h: the same with 1024 threads):
  * a tile is THREADS chunks of 16 residues of which the first THREADS - 1 own windows (:62-66, :774, :807, :888): lane j of tile t
    owns the 16 windows that start at t * (THREADS - 1) * 16 + 16 j + u, u = 0..15; the tile's last chunk owns none;
  * workgroup b of a grid of G takes tiles b, b + G, ... (:885) and keeps ONE table of SC_HOT = 64 (id, count) slots for all of
    them (:303-304, :791), emptied at the end of the kernel (:1147-1148);
  * 64 consecutive lanes are a wave.  The gate (:1070, kdb_kernels.hip.h:663-668): the forward 2-bit code of the first min(k, 16)
    residues of lane 0's chunk -- whatever the residues are: N and bytes past the end of the buffer encode as A (:182,
    kdb_kernels.hip.h:412) -- is shared by >= 16 of the wave's 64 lanes, dead ones included; the tile's last lane looks at chunk 0
    (:887);
  * behind the gate, window slot by window slot (:1075-1097): the live lanes (:1071, windows_bad16: no residue outside ACGT, no
    record start strictly inside, not past the record's end) whose id equals that of the FIRST LIVE lane form the group; a group
    of >= 16 leaves the rings and goes to the workgroup's table, or, where its slot there belongs to another id, straight to the
    vector (hot_add: a direct atomic, or a pair in the side list under `overlap`).
N mode changes nothing here: in EXPAND mode a window with an N is expanded elsewhere and is as dead to the shortcut as in DROP mode.
"""
import numpy as np

import ids_cases

NO_WINDOW = ids_cases.NO_WINDOW
SC_HOT = 64                       # slots of a workgroup's table
HOT_MIN = 16                      # lanes that make a group hot
WIDTHS = (512, 1024)              # threads of a scatter workgroup: 64-byte-line forms; 128-byte pieces, k = 13 in one level, k <= 8
DEFAULT_GRID = {512: 512, 1024: 256}      # SC_GRID, SC1_GRID (= SMALLK_GRID)
FIRST_TILE = 8176                 # (512 - 1) * 16: below it wave w is residues [1024 w, 1024 w + 1024) for both widths
_ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
_N = 78
_COMP = np.zeros(256, dtype=np.uint8)
_COMP[list(b"ACGT")] = list(b"TGCA")


class Case:
    """One batch and what it is meant to reach."""

    def __init__(self, name, bases, offsets, **notes):
        self.name = name
        self.bases = np.ascontiguousarray(bases, dtype=np.uint8)
        self.offsets = np.asarray(offsets, dtype=np.uint64)
        assert int(self.offsets[0]) == 0 and int(self.offsets[-1]) == self.bases.size and np.all(np.diff(self.offsets.astype(np.int64)) > 0)
        self.notes = notes

    @property
    def records(self):
        o = self.offsets.astype(np.int64)
        return [self.bases[int(s):int(e)].tobytes() for s, e in zip(o[:-1], o[1:])]

    @property
    def uniform(self):
        return len(set(np.diff(self.offsets.astype(np.int64)).tolist())) == 1

    def __repr__(self):
        return "Case({0}, {1} residues, {2} records)".format(self.name, self.bases.size, len(self.offsets) - 1)


# ---------------------------------------------------------------------------------------------------------------
# the lane model
# ---------------------------------------------------------------------------------------------------------------
class LaneModel:
    """ids, live, lead_lane, lead_id, size, gate of every (tile, wave, window slot); see the module docstring."""

    def __init__(self, bases, ids, k, threads):
        assert threads in WIDTHS
        n = int(bases.size)
        stride = threads - 1
        self.k, self.threads, self.tile_pos = k, threads, stride * 16
        self.ntiles = max(1, ((n + 15) // 16 + stride - 1) // stride)            # tile_geometry (kdb_scatter_host.hip.h:133-139)
        nt, nw = self.ntiles, threads // 64
        flat = np.full(nt * self.tile_pos, NO_WINDOW, dtype=np.uint64)
        flat[:n] = ids
        x = np.full((nt, threads, 16), NO_WINDOW, dtype=np.uint64)              # (the tile's last chunk owns no windows)
        x[:, :stride, :] = flat.reshape(nt, stride, 16)
        self.ids = np.ascontiguousarray(x.reshape(nt, nw, 64, 16).transpose(0, 1, 3, 2))      # [tile, wave, slot, lane]
        self.live = self.ids != NO_WINDOW
        self.any_live = self.live.any(axis=-1)
        self.lead_lane = self.live.argmax(axis=-1)                               # the first live lane (0 where none is live)
        self.lead_id = np.take_along_axis(self.ids, self.lead_lane[..., None], axis=-1)[..., 0]
        self.group = self.live & (self.ids == self.lead_id[..., None])
        self.size = self.group.sum(axis=-1)
        # the gate: codes of the first min(k, 16) residues of every chunk, as one number per chunk
        kk = min(k, 16)
        nchunks = nt * stride + 1
        raw = np.zeros(nchunks * 16, dtype=np.uint8)
        raw[:n] = bases
        code = ((raw ^ (raw >> 1)) >> 1) & 3                                     # kdb_scatter.hip.h:182
        wts = np.uint64(4) ** np.arange(kk - 1, -1, -1, dtype=np.uint64)
        key = (code.reshape(nchunks, 16)[:, :kk].astype(np.uint64) * wts).sum(axis=1)
        chunk = np.arange(nt)[:, None] * stride + np.arange(threads)[None, :]
        chunk[:, stride] = np.arange(nt) * stride                                # the last lane loads the hood of chunk 0
        self.key = key[chunk].reshape(nt, nw, 64)
        self.gate = (self.key == self.key[..., :1]).sum(axis=-1) >= HOT_MIN
        self.hot = self.gate[..., None] & (self.size >= HOT_MIN)                 # [tile, wave, slot]

    def counted(self):
        """windows the kernels count (DROP mode): the model's own total."""
        return int(self.live.sum())

    def hot_groups(self):
        """-> (tile, wave, slot, id, n) arrays of the groups that take the shortcut."""
        t, w, u = np.nonzero(self.hot)
        return t, w, u, self.lead_id[t, w, u], self.size[t, w, u]

    def hot_multiset(self):
        """{(id, n): how many groups}."""
        _, _, _, ids, n = self.hot_groups()
        pairs, cnt = np.unique(np.stack([ids, n.astype(np.uint64)], axis=1), axis=0, return_counts=True) if ids.size else (np.zeros((0, 2), np.uint64), [])
        return {(int(a), int(b)): int(c) for (a, b), c in zip(pairs, cnt)}

    def ring_ids(self):
        """ids of the counted windows that do NOT take the shortcut (what reaches the rings and the pages)."""
        return self.ids[self.live & ~(self.hot[..., None] & self.group)]

    def grid(self, sc_grid=0):
        g = sc_grid if sc_grid else DEFAULT_GRID[self.threads]
        return min(g, self.ntiles)                                               # sub_batch: L.G (kdb_scatter_host.hip.h:148)

    def per_workgroup(self, sc_grid=0):
        """-> list over workgroups of {hot id: groups}."""
        G = self.grid(sc_grid)
        t, _, _, ids, _ = self.hot_groups()
        out = [dict() for _ in range(G)]
        wg = t % G
        order = np.lexsort((ids, wg))
        wg, ids = wg[order], ids[order]
        pairs, cnt = np.unique(np.stack([wg.astype(np.uint64), ids], axis=1), axis=0, return_counts=True) if ids.size else (np.zeros((0, 2), np.uint64), [])
        for (b, i), c in zip(pairs, cnt):
            out[int(b)][int(i)] = int(c)
        return out

    def distinct_hot_ids(self, sc_grid=0):
        return [len(d) for d in self.per_workgroup(sc_grid)]

    def direct_adds_at_least(self, sc_grid=0):
        """A lower bound, whatever the hash, on the groups that cannot use the table: a slot keeps its id until the kernel ends, so
        at most SC_HOT ids of a workgroup ever own one; every group of every other id is added directly (a pair of the side list
        under `overlap`).  The best case for the table is that the SC_HOT most frequent ids own the slots."""
        total = 0
        for d in self.per_workgroup(sc_grid):
            c = sorted(d.values(), reverse=True)
            total += sum(c[SC_HOT:])
        return total

    def slot_counts(self, t, w, u):
        """{id: live lanes that hold it} of one slot."""
        row = self.ids[t, w, u][self.live[t, w, u]]
        i, c = np.unique(row, return_counts=True)
        return {int(a): int(b) for a, b in zip(i, c)}


def window_ids(case, k, canon):
    return ids_cases.expected_window_ids(case.bases, case.offsets, k, canon)


def lane_model(case, k, canon, threads, ids=None):
    return LaneModel(case.bases, window_ids(case, k, canon) if ids is None else ids, k, threads)


# ---------------------------------------------------------------------------------------------------------------
# building blocks
# ---------------------------------------------------------------------------------------------------------------
def _rng(*seed):
    return np.random.Generator(np.random.PCG64(list(seed)))


def random_bases(rng, n):
    return _ACGT[rng.integers(0, 4, size=n)].copy()


def revcomp(b):
    return _COMP[np.asarray(b, dtype=np.uint8)][::-1].copy()


def is_primitive(unit):
    p = len(unit)
    return not any(p % d == 0 and np.array_equal(np.tile(unit[:d], p // d), unit) for d in range(1, p))


def _cyclic_canonical(unit, L):
    """the canonical L-mers (as byte strings) at the len(unit) phases of the periodic sequence."""
    p = len(unit)
    s = np.tile(unit, (L + p - 1) // p + 1)
    out = []
    for i in range(p):
        w = s[i:i + L]
        out.append(min(w.tobytes(), revcomp(w).tobytes()))
    return out


def primitive_unit(rng, p, distinct_at=0, pin=None):
    """A random unit of period exactly p.  distinct_at = L: the canonical L-mers at its p phases all differ (and so do those of any
    longer window, in either strand mode): no two phases can fall into one group by chance.  pin = {position: letter}."""
    if p == 1:
        return np.frombuffer(b"A", dtype=np.uint8).copy()
    if p == 2 and not pin:
        return np.frombuffer(b"AC", dtype=np.uint8).copy()
    while True:
        u = random_bases(rng, p)
        for i, c in (pin or {}).items():
            u[i] = c
        if not is_primitive(u):
            continue
        if distinct_at and len(set(_cyclic_canonical(u, distinct_at))) < p:
            continue
        return u


def periodic(unit, n, phase=0):
    p = len(unit)
    return np.tile(unit, (n + phase) // p + 2)[phase:phase + n].copy()


def other_letter(c, rng=None):
    return int(_ACGT[(int(np.flatnonzero(_ACGT == c)[0]) + 1) % 4])


def _offsets(n, starts=()):
    return np.array(sorted({0, n} | set(int(s) for s in starts)), dtype=np.uint64)


# ---------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------
THRESHOLD_G = (15, 16, 17)


def threshold(k, ragged=False, seed=0):
    """Waves 1, 3 and 5 of the first tile: the first G lanes hold one period-16 unit, G = 15, 16, 17, the other lanes random bases
    (the lane behind the unit starts with another letter than the unit, so every window of lane G - 1 that reaches into it leaves
    the group: slots with G and with G - 1 members in one wave)."""
    assert 2 <= k <= 16
    rng = _rng(101, k, seed)
    b = random_bases(rng, 8000)
    for w, G in zip((1, 3, 5), THRESHOLD_G):
        u = primitive_unit(rng, 16, distinct_at=min(k, 8))
        at = 1024 * w
        b[at:at + 16 * G] = periodic(u, 16 * G)
        b[at + 16 * G] = other_letter(u[0])
    return Case("threshold k=%d%s" % (k, " ragged" if ragged else ""), b, _offsets(8000, (500, 2500) if ragged else ()), waves=(1, 3, 5))


def exact_groups(k, n, seed=0):
    """One wave (wave 1 of a record of 4096 residues) whose gate passes and whose groups all have EXACTLY n members, n = 15 or 16 --
    for the deferred histogram pass's store form, which only survives a batch that adds nothing to the vector directly:
      n = 16: lanes 0..15 hold a period-16 unit: the slots whose windows stay inside lane 15 have 16 members (the others 15);
      n = 15: the same, but lane 15 has an N where the unit has an A among its first k residues -- the N encodes as A, so 16 lanes share
              lane 0's key and the gate passes, while lane 15 is dead in the slots the N reaches and differs in the others (k >= 9)."""
    assert 9 <= k <= 16 and n in (15, 16)
    rng = _rng(103, k, n, seed)
    b = random_bases(rng, 4096)
    u = primitive_unit(rng, 16, distinct_at=8, pin={k - 1: ord("A")})
    b[1024:1024 + 256] = periodic(u, 256)
    b[1024 + 256] = other_letter(u[0])
    if n == 15:
        b[1024 + 15 * 16 + k - 1] = _N
    return Case("exact %d k=%d" % (n, k), b, _offsets(4096))


def dead_leader(k, seed=0):
    """One wave (wave 1 of a record of 4096 residues) whose ONLY hot groups sit in slots where lane 0 is dead and the id that its residues
    would give differs from the group's -- for the form of the deferred pass: the kernel that takes the first LIVE lane adds those groups
    to the vector directly, one that took lane 0 would find no group and leave the vector clean.
    Lanes 0..20 hold a period-16 unit with A at positions 2 and k - 1 and another letter at 15.  Lane 0 has N's at k - 1 and at 15: all its
    sixteen windows are dead, its key is the unit's (an N encodes as A), and from slot 16 - k on its would-be id reads A where the unit
    does not.  Lanes 1..20 have an N at position 2: dead in slots 0..2, and so is every window that reaches position 2 of the next lane
    (slots >= 19 - k).  Slots 3 .. 18 - k: lanes 1..19 alive with one id, lane 1 first."""
    assert 13 <= k <= 15
    rng = _rng(105, k, seed)
    b = random_bases(rng, 4096)
    u = primitive_unit(rng, 16, distinct_at=8, pin={2: ord("A"), k - 1: ord("A"), 15: ord("C")})
    b[1024:1024 + 21 * 16] = periodic(u, 21 * 16)
    b[1024 + 21 * 16] = other_letter(u[0])
    b[1024 + k - 1] = _N
    b[1024 + 15] = _N
    for j in range(1, 21):
        b[1024 + 16 * j + 2] = _N
    return Case("dead_leader k=%d" % k, b, _offsets(4096))


def n_as_a(case):
    """the case with every N replaced by A: what the kernels' 2-bit code makes of it (kdb_scatter.hip.h:182) -- for the id a dead lane would have."""
    b = case.bases.copy()
    b[b == _N] = ord("A")
    return Case(case.name + " N->A", b, case.offsets)


def leader(k, ragged=False, seed=0):
    """Three waves of the first tile.
    wave 1: all 64 lanes hold one period-16 unit, but lane 0 is dead in some slots -- an N where the unit has an A inside the first k
            residues (the key is unchanged); the ragged form has a record start inside lane 0's chunk as well.  Lane 1 leads.
    wave 2: lanes 0..7 random, lanes 8..63 one unit: lane 0's key is its own, the gate fails, nothing may be shortcut.
    wave 3: the even lanes hold one unit; of the odd lanes 1, 3 and 5 hold X and the others Y (X and Y begin with different
            letters).  Slot 0 and every slot whose window stays inside its chunk: 32 lanes with lane 0's id.  A window that reaches
            into the next chunk: lane 0 leads lanes 0, 2, 4 -- a minority -- while 29 lanes share another id."""
    rng = _rng(107, k, seed)
    b = random_bases(rng, 8000)
    kk = min(k, 16)
    u1 = primitive_unit(rng, 16, distinct_at=min(k, 8), pin={kk - 1: ord("A")})
    b[1024:2048] = periodic(u1, 1024)
    b[1024 + kk - 1] = _N
    starts = [600, 1024 + 8, 2300] if ragged else []
    if ragged:
        b[1024 + kk - 1] = u1[kk - 1]                    # (the ragged form kills lane 0's windows with the record start alone)
    u2 = primitive_unit(rng, 16, distinct_at=min(k, 8))
    b[2048 + 128:3072] = periodic(u2, 1024 - 128)
    ua, y = primitive_unit(rng, 16, distinct_at=min(k, 8)), primitive_unit(rng, 16, distinct_at=min(k, 8))
    x = random_bases(rng, 16)
    x[0] = other_letter(y[0])
    for j in range(64):
        b[3072 + 16 * j:3072 + 16 * j + 16] = ua if j % 2 == 0 else (x if j in (1, 3, 5) else y)
    return Case("leader k=%d%s" % (k, " ragged" if ragged else ""), b, _offsets(8000, starts))


PERIODS = (1, 2, 3, 4, 6, 8, 12, 16, 32, 64, 5, 128)
# what the leader's group of a whole wave of period p holds (a wave with the tile's last lane: one fewer)
PERIOD_SIZES = {1: {64}, 2: {64}, 4: {64}, 8: {64}, 16: {64}, 3: {21, 22}, 6: {21, 22}, 12: {21, 22}, 32: {32}, 64: {16}, 5: set(), 128: set()}
PERIOD_LEN = 40000                # more than two tiles of either width: the waves' alignment drifts by 16 residues per tile


def periods(k, ragged=False, seed=0):
    """One record per period, each several tiles long.  The units' phases differ in their canonical 5-mers (6-mers for period 128),
    so lanes share an id exactly where the period says.  Records 1, 3 and 16 hold an N in the middle of the stretch."""
    rng = _rng(109, seed)                                 # (the same residues at every k)
    recs, where = [], {}
    for i, p in enumerate(PERIODS):
        u = primitive_unit(rng, p, distinct_at=0 if p <= 2 else (6 if p == 128 else 5))
        r = periodic(u, PERIOD_LEN + (17 * i + 1 if ragged else 0), phase=int(rng.integers(0, p)))
        if p in (1, 3, 16):
            r[len(r) // 2 + 5] = _N
        where[p] = (sum(len(x) for x in recs), len(r))
        recs.append(r)
    b = np.concatenate(recs)
    offs = np.concatenate([[0], np.cumsum([len(r) for r in recs])])
    return Case("periods k=%d%s" % (k, " ragged" if ragged else ""), b, offs, where=where)


def period_sizes(model, case, p):
    """-> the set of sizes of the hot groups in the waves that lie wholly inside the record of period p and hold no N."""
    start, length = case.notes["where"][p]
    tp, nw = model.tile_pos, model.threads // 64
    sizes = set()
    t, w, u, _, n = model.hot_groups()
    first = t * tp + w * 1024
    n_at = np.flatnonzero(case.bases[start:start + length] == _N) + start
    inside = (first >= start) & (first + 1024 + 16 + model.k <= start + length)
    for a in n_at:
        inside &= ~((first <= a) & (a < first + 1024 + 16 + model.k))
    return set(int(x) for x in n[inside]), int(inside.sum())


def interior_waves(model, case, p):
    """-> (tile, wave) of the waves wholly inside the record of period p, with no N."""
    start, length = case.notes["where"][p]
    out = []
    n_at = np.flatnonzero(case.bases[start:start + length] == _N) + start
    for t in range(model.ntiles):
        for w in range(model.threads // 64):
            first = t * model.tile_pos + w * 1024
            if first >= start and first + 1024 + 16 + model.k <= start + length and not any(first <= a < first + 1024 + 16 + model.k for a in n_at):
                out.append((t, w))
    return out


SEGMENT = 16384


def many_ids(n_units, seed=0, n_random=2000):
    """n_units records of 16 KiB, each a different period-16 unit: sixteen hot ids per unit, all 64 lanes of every wave in one group.
    Behind them n_random random reads of 100 bases, which fall into the hot ids' buckets (the counts that a direct atomic beside a
    histogram pass would race with)."""
    rng = _rng(113, n_units, seed)
    segs = [periodic(primitive_unit(rng, 16, distinct_at=8), SEGMENT) for _ in range(n_units)]
    lens = [SEGMENT] * n_units + [100] * n_random
    b = np.concatenate(segs + [random_bases(rng, 100 * n_random)])
    return Case("many_ids %d units" % n_units, b, np.concatenate([[0], np.cumsum(lens)]), n_units=n_units, n_random=n_random)


MANY_SMALL = 6                    # units that put more than SC_HOT ids into the one workgroup of sc_grid = 1
MANY_DEFAULT = 1400               # units for the default grids: 256 workgroups of 16 KiB tiles or 512 of 8 KiB tiles see >= 5 units each
SIDE_OLD_CAP = 1 * SC_HOT + 65536                        # what the side list held at sc_grid = 1 whatever the batch
SIDE_UNITS = 384                  # 6 MiB


def side_overflow(seed=0):
    return many_ids(SIDE_UNITS, seed=seed + 1, n_random=2000)


def both_strands(k, ragged=False, seed=0):
    """Waves whose lanes hold a unit and its reverse complement: wave 1 = 16 lanes of poly-A, then 16 of poly-T; wave 3 = 16 lanes of
    (AC)n, then 16 lanes of the period-2 sequence that begins with the reverse complement of (AC)n's first k residues.  Lane 15's
    windows that reach into lane 16 leave the forward group (15 members) but pair up with lanes 16.. on the other strand."""
    rng = _rng(127, k, seed)
    b = random_bases(rng, 8000)
    b[1024:1024 + 256] = ord("A")
    b[1024 + 256:1024 + 512] = ord("T")
    b[1024 + 512] = ord("C")
    ac = periodic(np.frombuffer(b"AC", dtype=np.uint8), 256 + k)
    partner = revcomp(ac[:k])                              # what lane 16's first window must read
    b[3072:3072 + 256] = ac[:256]
    b[3072 + 256:3072 + 512] = periodic(partner[:2], 256)
    b[3072 + 512] = other_letter(partner[0])
    return Case("both_strands k=%d%s" % (k, " ragged" if ragged else ""), b, _offsets(8000, (700, 2600) if ragged else ()))


HIGH_T = b"CATGGTACCTGAAGTC"      # a fixed 16-mer


def high_bits(seed=0):
    """k = 17: records of 32 residues x . T . T[0:15], x = A or G by turns -- two chunks each.  The even lanes' window 0 is x . T: ids
    equal in their low 32 bits (T) and different above (x); 16 lanes of each in a wave, and the first 16 residues (the gate's key)
    shared by the 16 lanes of lane 0's letter.  Windows 1..15 do not hold x: 32 lanes with one id.  The odd lanes own no window.
    Waves 0 and 2 begin with an A record, wave 1 with a G record; random records of 32 residues follow."""
    rng = _rng(131, seed)
    t = np.frombuffer(HIGH_T, dtype=np.uint8)
    recs = []
    for w in range(3):
        for i in range(32):
            x = b"AG"[(i + w) % 2]
            recs.append(np.concatenate([[x], t, t[:15]]).astype(np.uint8))
    recs += [random_bases(rng, 32) for _ in range(300)]
    b = np.concatenate(recs)
    return Case("high_bits", b, np.arange(len(recs) + 1) * 32)


PLANTED_READS = 150000


def planted(k, seed=0):
    """One k-mer once per read, at a random offset, in 150 000 random reads of 100 bases: never 16 lanes of a wave with it in one slot,
    so all its windows go through the rings into the pages of one bucket (counts above 65535 in one bin; page_hist_kernel's
    dominant-key branch with other keys beside it)."""
    rng = _rng(137, k, seed)
    b = random_bases(rng, PLANTED_READS * 100)
    kmer = random_bases(rng, k)
    at = rng.integers(0, 100 - k + 1, size=PLANTED_READS) + np.arange(PLANTED_READS) * 100
    b[(at[:, None] + np.arange(k)[None, :]).ravel()] = np.tile(kmer, PLANTED_READS)
    return Case("planted k=%d" % k, b, np.arange(PLANTED_READS + 1) * 100, kmer=kmer.tobytes())


def all_hot(k, waves=3):
    """poly-A whose counted windows fill whole waves exactly: every window takes the shortcut, nothing reaches a ring or a page."""
    return Case("all_hot k=%d" % k, np.full(1024 * waves + k - 1, ord("A"), dtype=np.uint8), _offsets(1024 * waves + k - 1))


# ---------------------------------------------------------------------------------------------------------------
# seeded mixed batches
# ---------------------------------------------------------------------------------------------------------------
K_CLASSES = {"lds": (5, 8), "one_level": (9, 12), "k13": (13,), "two_level": (14, 16)}
REPEAT_PERIODS = (1, 2, 3, 4, 6, 8, 12, 16, 32, 64)
REPEAT_SEEDS = tuple(range(12))                            # per k class


def repeat_draw(rng, kclass):
    """-> (desc, Case): random reads, periodic reads, point mutations, occasional N's, uniform or ragged lengths, duplicated reads; at
    most 2 MB.  desc holds k, strand and N mode, engine options and the cutting into pieces in the form tests/fuzz_gpu.py draws them (its
    check_case runs them); kdb_reset between pieces is left out: what counts here is the whole batch."""
    k = int(rng.choice(K_CLASSES[kclass]))
    canon = bool(rng.integers(0, 2))
    expand = bool(rng.integers(0, 3) == 0)
    uniform = bool(rng.integers(0, 2))
    nreads = int(rng.choice([40, 200, 600]))
    L = int(rng.choice([300, 1200, 2600]))
    lens = np.full(nreads, L) if uniform else rng.integers(max(k, 40), L + 1, size=nreads)
    recs = []
    for n in lens.tolist():
        kind = rng.integers(0, 10)
        if kind < 4 or not recs and kind >= 8:
            r = random_bases(rng, n)
        elif kind < 8:
            p = int(rng.choice(REPEAT_PERIODS))
            r = periodic(primitive_unit(rng, p), n, phase=int(rng.integers(0, p)))
            if rng.integers(0, 2):                          # a periodic stretch inside a random read
                a = int(rng.integers(0, n))
                r[:a] = random_bases(rng, a)
            nm = int(rng.choice([0, 0, 1, 3]))              # point mutations
            for at in rng.integers(0, n, size=nm).tolist():
                r[at] = _ACGT[rng.integers(0, 4)]
        else:                                               # a duplicate of an earlier read (cut or padded to this length)
            src = recs[int(rng.integers(0, len(recs)))]
            r = np.concatenate([src, random_bases(rng, max(0, n - len(src)))])[:n].copy()
        if rng.integers(0, 12) == 0:
            r[int(rng.integers(0, n))] = _N
        recs.append(r)
    opts = {}
    if rng.integers(0, 3) == 0:
        opts["stage_bytes"] = int(rng.choice([4096, 65536, 1 << 20]))
        opts["stage_reads"] = int(rng.choice([3, 64, 4096]))
    if k >= 13 and rng.integers(0, 2):
        opts["defer_flush"] = int(rng.integers(0, 2))
    if rng.integers(0, 4) == 0:
        opts["sc_grid"] = int(rng.choice([1, 7, 64]))
    if k >= 8 and rng.integers(0, 3) == 0:
        opts["sc_lo_bits"] = int(rng.choice([1, 3, 6, 9, 12, 14, 15]))
    if k >= 8 and rng.integers(0, 4) == 0:
        opts["sc_contig_pages"] = 1
    if k <= 8 and rng.integers(0, 4) == 0:
        opts["smallk_old"] = 1
    if k == 13 and rng.integers(0, 3) == 0:
        opts["one_level_max_k"] = 12
    if 8 <= k <= 12 and rng.integers(0, 4) == 0:
        opts["sc_wide_lines"] = 0
    if k >= 13 and rng.integers(0, 4) == 0:
        opts["l1_wide_lines"] = 0
    if k >= 13 and rng.integers(0, 4) == 0:
        opts["l2_wide_lines"] = 0
    if 13 <= k <= 15 and rng.integers(0, 4) == 0:
        opts["l1_one_round"] = 0
    if canon and k <= 12 and rng.integers(0, 3) == 0:
        opts["strand_merge"] = 0
    if 9 <= k <= 13 and not expand and rng.integers(0, 3) == 0:
        opts["overlap"] = 1
    if k >= 13 and rng.integers(0, 2):
        opts["accum_bytes"] = int(rng.choice([0, 1 << 20]))
    if k >= 14 and rng.integers(0, 3) == 0:
        opts["arena_batches"] = int(rng.choice([1, 2]))
        opts["arena_grow"] = int(rng.choice([0, 1, 2]))
    algo = int(rng.choice([0, 1, 2, 2, 2]))
    nsub = int(rng.choice([1, 1, 2, 4]))
    cuts = sorted(set([0, nreads] + [int(x) for x in rng.integers(0, nreads + 1, size=nsub - 1)]))
    # per piece: 0 host submit, 1 handed over in HBM, 2 host submit followed by a sync
    how = [int(x) for x in rng.choice([0, 0, 1, 1, 2], size=len(cuts) - 1)]
    b = np.concatenate(recs)
    desc = dict(k=k, canon=canon, expand=expand, algo=algo, uniform=uniform, nreads=nreads, bases=int(b.size), opts=opts, cuts=cuts, how=how, reset_at=0)
    return desc, Case("repeat %s" % kclass, b, np.concatenate([[0], np.cumsum([len(r) for r in recs])]))


def fixed_repeat(kclass, seed):
    return repeat_draw(_rng(139, sorted(K_CLASSES).index(kclass), seed), kclass)


def kernel_view(desc):
    """-> (canon, threads) of the kernel that counts a repeat_draw case's windows, or None where the model does not describe it: the
    direct-atomics kernel (algo 1) and the kernels behind smallk_old have tiles of 16 KiB."""
    k, o = desc["k"], desc["opts"]
    if desc["algo"] == 1 or o.get("smallk_old"):
        return None
    staged = desc["canon"] and k <= 12 and o.get("strand_merge", 1) and not o.get("overlap") and not o.get("smallk_old")
    if k <= 8:
        threads = 1024
    elif k <= 12:
        threads = 1024 if o.get("sc_wide_lines", 1) else 512
    elif k == 13 and o.get("one_level_max_k", 13) == 13:
        threads = 1024
    else:
        threads = 1024 if o.get("l1_wide_lines", 1) else 512
    return (desc["canon"] and not staged), threads
