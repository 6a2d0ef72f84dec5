"""tests/hot_cases.py proven on the CPU: every case reaches the branch of the counting kernels' same-id shortcut that it names, for
workgroups of 512 and of 1024 threads, and the model's own total of counted windows is the oracle's.  No GPU."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hot_cases as hc  # noqa: E402

KS = (5, 8, 9, 12, 13, 14, 16)                    # what tests/test_gpu_hot_ids.py runs the layout cases at
WIDTHS = hc.WIDTHS


def models(oracle, case, k, canon):
    """-> the models for both widths; the model's total is checked against oracle.c_count on the way."""
    ids = hc.window_ids(case, k, canon)
    want_total = oracle.c_count(case.bases, case.offsets, k, canon, oracle.N_DROP)[1] if k <= 13 else int(np.count_nonzero(ids != hc.NO_WINDOW))
    if k > 13:                                     # (no 4^k vector on the CPU: the oracle's shred, record by record, is what window_ids ran)
        assert want_total == sum(len(r) - k + 1 - _dead(r, k) for r in case.records)
    out = []
    for th in WIDTHS:
        m = hc.lane_model(case, k, canon, th, ids)
        assert m.counted() == want_total, (case, k, canon, th)
        out.append(m)
    return out


def _dead(rec, k):
    """windows of an N-free-or-not record that hold an N (counted from the record itself)."""
    a = np.frombuffer(rec, dtype=np.uint8) == 78
    if not a.any():
        return 0
    c = np.concatenate([[0], np.cumsum(a)])
    return int(np.count_nonzero(c[k:] - c[:-k]))


@pytest.mark.parametrize("ragged", [False, True])
@pytest.mark.parametrize("k", KS)
def test_threshold_has_groups_of_15_16_and_17(oracle, k, ragged):
    case = hc.threshold(k, ragged)
    assert case.bases.size < hc.FIRST_TILE and case.uniform != ragged
    for canon in (False, True):
        for m in models(oracle, case, k, canon):
            seen = {}
            for w, G in zip(case.notes["waves"], hc.THRESHOLD_G):
                sizes = set(int(x) for x in m.size[0, w])
                assert {G, G - 1} <= sizes, (k, canon, w, sizes)
                assert bool(m.gate[0, w]) == (G >= 16)
                seen[G] = set(int(x) for x in m.size[0, w][m.hot[0, w]])
            assert seen[15] == set() and 16 in seen[16] and 15 not in seen[16] and {16, 17} <= seen[17]
            assert {15, 16, 17} <= set(int(x) for x in m.size[0].ravel())


@pytest.mark.parametrize("n", [15, 16])
@pytest.mark.parametrize("k", [13, 14])
def test_exact_groups(oracle, k, n):
    case = hc.exact_groups(k, n)
    for m in models(oracle, case, k, True):
        assert m.gate[0, 1] and not m.gate[0, 0] and not m.gate[0, 2]
        sizes = set(int(x) for x in m.size[0, 1])
        if n == 15:
            assert sizes == {15} and not m.hot.any()            # the gate passes, no group reaches 16: nothing is added directly
        else:
            assert sizes == {15, 16}
            _, _, _, _, hot_n = m.hot_groups()
            assert hot_n.size and set(hot_n.tolist()) == {16}    # every hot group has exactly 16 members


@pytest.mark.parametrize("k", [13, 14])
def test_dead_leader_has_hot_groups_only_where_lane_0_is_dead_and_differs(oracle, k):
    case = hc.dead_leader(k)
    would_be = hc.window_ids(hc.n_as_a(case), k, True)          # the ids that the residues give with their N's read as A
    for m in models(oracle, case, k, True):
        assert m.gate[0, 1] and not m.live[0, 1, :, 0].any()
        t, w, u, ids, n = m.hot_groups()
        assert set(u.tolist()) == set(range(3, 19 - k)) and set(w.tolist()) == {1} and set(t.tolist()) == {0}
        assert np.all(m.lead_lane[0, 1][u] == 1) and np.all(n >= 19)
        for slot, gid in zip(u.tolist(), ids.tolist()):
            assert int(would_be[1024 + slot]) != gid and int(would_be[1024 + 16 + slot]) == gid


@pytest.mark.parametrize("ragged", [False, True])
@pytest.mark.parametrize("k", KS)
def test_leader_cases(oracle, k, ragged):
    case = hc.leader(k, ragged)
    assert case.bases.size < hc.FIRST_TILE and case.uniform != ragged
    for canon in (False, True):
        for m in models(oracle, case, k, canon):
            # wave 1: lane 0 dead, lane 1 leads a hot group
            assert m.gate[0, 1]
            dead0 = ~m.live[0, 1, :, 0]
            assert dead0.any() and np.all(m.lead_lane[0, 1][dead0] == 1) and np.all(m.size[0, 1][dead0] >= 16) and np.all(m.hot[0, 1][dead0])
            assert np.all(m.lead_lane[0, 1][~dead0] == 0)
            # wave 2: the gate fails although 56 lanes share an id in every slot
            assert not m.gate[0, 2] and not m.hot[0, 2].any()
            assert all(max(m.slot_counts(0, 2, u).values()) >= 40 for u in range(16))
            # wave 3: lane 0 leads; a hot group in slot 0, a minority beside a group of 16 or more in a later slot
            assert m.gate[0, 3] and np.all(m.lead_lane[0, 3] == 0) and m.hot[0, 3, 0] and m.size[0, 3, 0] >= 32
            minority = [u for u in range(16) if m.size[0, 3, u] < 16 and max(m.slot_counts(0, 3, u).values()) >= 16]
            assert minority and not any(m.hot[0, 3, u] for u in minority), (k, canon, minority)


@pytest.mark.parametrize("ragged", [False, True])
@pytest.mark.parametrize("k", KS)
def test_periods_give_the_group_sizes_of_their_period(oracle, k, ragged):
    case = hc.periods(k, ragged)
    assert case.uniform != ragged
    for canon in (False, True):
        for m in models(oracle, case, k, canon):
            assert m.ntiles >= 2 * len(hc.PERIODS)
            for p in hc.PERIODS:
                if p == 128 and k < 6:
                    continue                       # (the unit's phases differ in their 6-mers; eight of its 5-mers may coincide)
                want = hc.PERIOD_SIZES[p]
                sizes, nhot = hc.period_sizes(m, case, p)
                waves = hc.interior_waves(m, case, p)
                assert len(waves) >= 20
                # a wave with the tile's last lane has one member fewer; the leader's class decides between 21 and 22
                allowed = want | {s - 1 for s in want} | ({20} if 21 in want else set())
                if not want:
                    assert nhot == 0 and not any(m.gate[t, w] for t, w in waves), (k, canon, p)
                    continue
                assert want <= sizes <= allowed, (k, canon, p, sizes)
                assert all(m.gate[t, w] for t, w in waves)
                if p == 64:
                    # exactly 16 lanes hot, the other 48 (three more phase classes of 16) through the rings in the same slot
                    assert sizes == {16}
                    t, w = waves[0]
                    assert sorted(m.slot_counts(t, w, 0).values()) in ([16, 16, 16, 16], [15, 16, 16, 16])
                # the alignment drifts: the waves' first residues differ in their phase from tile to tile
            starts = {(t * m.tile_pos) % 1024 for t in range(m.ntiles)}
            assert len(starts) >= 4


@pytest.mark.parametrize("k", [9, 12, 13, 15])
def test_many_ids_overfill_the_table_of_one_workgroup(oracle, k):
    case = hc.many_ids(hc.MANY_SMALL)
    for canon in (False, True):
        for m in models(oracle, case, k, canon):
            assert m.distinct_hot_ids(sc_grid=1) and m.distinct_hot_ids(sc_grid=1)[0] >= hc.SC_HOT + 1      # pigeonhole: a slot conflict whatever the hash
            assert m.direct_adds_at_least(sc_grid=1) >= 16
            # the random reads fall into the hot ids' buckets (one-level: id bits 9.., two-level: bits 12..)
            hot_ids = np.array(sorted(m.per_workgroup(1)[0]), dtype=np.uint64)
            rnd = hc.window_ids(hc.Case("r", case.bases[hc.MANY_SMALL * hc.SEGMENT:], case.offsets[hc.MANY_SMALL:] - case.offsets[hc.MANY_SMALL]), k, canon)
            rnd = rnd[rnd != hc.NO_WINDOW]
            lo, nb = (9, 2 * k - (16 if k == 13 else 15)) if k <= 13 else (12, 2 * k - 15)
            bucket = lambda x: (x >> np.uint64(lo)) & np.uint64((1 << nb) - 1)      # noqa: E731
            assert np.isin(bucket(hot_ids), bucket(rnd)).mean() >= 0.9


@pytest.mark.parametrize("k", [9, 12, 13, 15])
def test_many_ids_overfill_every_workgroup_of_the_default_grids(oracle, k):
    case = hc.many_ids(hc.MANY_DEFAULT)
    for m in models(oracle, case, k, False):
        per = m.distinct_hot_ids()
        assert len(per) == hc.DEFAULT_GRID[m.threads] and min(per) >= hc.SC_HOT + 1, (m.threads, min(per))
        assert m.direct_adds_at_least() >= len(per)


def test_side_overflow_exceeds_the_old_capacity_by_a_quarter(oracle):
    case = hc.side_overflow()
    assert 6 * 2 ** 20 <= case.bases.size <= 7 * 2 ** 20
    for canon in (False, True):
        for m in models(oracle, case, 12, canon):
            pairs = m.direct_adds_at_least(sc_grid=1)
            print("side_overflow canon=%d threads=%d: at least %d pairs, the list held %d" % (canon, m.threads, pairs, hc.SIDE_OLD_CAP))
            assert 4 * pairs >= 5 * hc.SIDE_OLD_CAP


@pytest.mark.parametrize("ragged", [False, True])
@pytest.mark.parametrize("k", KS)
def test_both_strands_fold_into_one_group(oracle, k, ragged):
    """(The canonical group of a leader holds its forward group, so "forward >= 16, canonical < 16" cannot exist; the converse asserted
    here is a slot that is hot on the forward strand alone already and whose canonical group is larger still.)"""
    case = hc.both_strands(k, ragged)
    assert case.bases.size < hc.FIRST_TILE
    fwd, can = models(oracle, case, k, False), models(oracle, case, k, True)
    for f, c in zip(fwd, can):
        only_canon = both = 0
        for w in (1, 3):
            assert f.gate[0, w] and c.gate[0, w]
            for u in range(16):
                assert c.size[0, w, u] >= f.size[0, w, u]
                only_canon += bool(c.size[0, w, u] >= 16 and f.size[0, w, u] < 16 and f.lead_lane[0, w, u] == c.lead_lane[0, w, u])
                both += bool(f.size[0, w, u] >= 16 and c.size[0, w, u] > f.size[0, w, u])
        assert only_canon >= 1 and both >= 1, (k, only_canon, both)


def test_high_bits_ids_differ_above_bit_31_only(oracle):
    case = hc.high_bits()
    assert case.uniform
    for canon in (False,):
        for m in models(oracle, case, 17, canon):
            for w in (0, 1, 2):
                ids, live = m.ids[0, w, 0], m.live[0, w, 0]
                assert m.gate[0, w] and int(live.sum()) == 32 and not live[1::2].any()
                assert m.lead_lane[0, w, 0] == 0 and m.size[0, w, 0] == 16 and m.hot[0, w, 0]
                lead = int(m.lead_id[0, w, 0])
                others = ids[live & (ids != np.uint64(lead))]
                assert others.size == 16 and len(set(others.tolist())) == 1
                assert int(others[0]) & 0xFFFFFFFF == lead & 0xFFFFFFFF and int(others[0]) >> 32 != lead >> 32
                assert np.all(m.size[0, w, 1:] == 32)
        for m in models(oracle, case, 16, canon):      # the twin: 32-bit ids that differ in their leading base
            assert m.gate[0, 0] and m.size[0, 0, 0] == 16 and m.hot[0, 0, 0]


@pytest.mark.parametrize("k", [12, 13])
def test_planted_kmer_is_never_hot(oracle, k):
    case = hc.planted(k)
    want = int(oracle.c_shred(case.notes["kmer"], k, False, oracle.N_DROP)[0][0])
    counts, total = oracle.c_count(case.bases, case.offsets, k, False, oracle.N_DROP)
    assert counts[want] >= hc.PLANTED_READS and counts[want] > 65535
    ids = hc.window_ids(case, k, False)
    for th in WIDTHS:
        m = hc.lane_model(case, k, False, th, ids)
        assert m.counted() == total
        _, _, _, hot_ids, _ = m.hot_groups()
        assert not np.any(hot_ids == np.uint64(want))
        assert int(np.count_nonzero(m.ring_ids() == np.uint64(want))) == int(counts[want])


@pytest.mark.parametrize("k", [13, 14])
def test_all_hot_leaves_nothing_for_the_rings(oracle, k):
    case = hc.all_hot(k)
    for m in models(oracle, case, k, True):
        assert m.ring_ids().size == 0 and m.hot_multiset() == {(0, 64): 16 * 3}


@pytest.mark.parametrize("kclass", sorted(hc.K_CLASSES))
def test_repeat_draw_seeds_cover_what_they_say(oracle, kclass):
    small = big = two = described = 0
    ks = set()
    for seed in hc.REPEAT_SEEDS:
        desc, case = hc.fixed_repeat(kclass, seed)
        assert case.bases.size <= 2 * 10 ** 6 and desc["k"] in hc.K_CLASSES[kclass]
        ks.add(desc["k"])
        view = hc.kernel_view(desc)
        if view is None:
            continue                               # (a kernel with another tile layout: its draws count for nothing here)
        described += 1
        canon, threads = view
        m = hc.lane_model(case, desc["k"], canon, threads)
        t, w, _, ids, n = m.hot_groups()
        small += bool(np.any((n >= 16) & (n <= 20)))
        big += bool(np.any(n == 64))
        wave = t.astype(np.int64) * 64 + w
        per_wave = {}
        for a, b in zip(wave.tolist(), ids.tolist()):
            per_wave.setdefault(a, set()).add(b)
        two += bool(any(len(s) >= 2 for s in per_wave.values()))
    print(kclass, "draws that the model describes:", described, "batches with groups of 16..20:", small, "of 64:", big, "with two hot ids in a wave:", two, "k:", sorted(ks))
    assert small >= 2 and big >= 2 and two >= 2 and ks == set(hc.K_CLASSES[kclass])
