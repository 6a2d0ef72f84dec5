"""CPU: the restatement of the minimizer definition (tests/minimizer_cases.py) against answers worked out by hand, and the properties that
follow from the definition.  The GPU tests compare kdb_minimizers with this restatement; here it is itself under test."""
import numpy as np
import pytest

import minimizer_cases as mc


def _lists(rec, k, w, canonical, order):
    pos, ids, strand = mc.record_minimizers(rec, k, w, canonical, order)
    return pos.tolist(), ids.tolist(), strand.tolist()


def test_acgtacgt_by_hand():
    # forward ids of ACG CGT GTA TAC ACG CGT: 6 27 44 49 6 27; runs of two: (6,27) (27,44) (44,49) (49,6) (6,27) -> 0 1 2 4 4
    assert _lists(b"ACGTACGT", 3, 2, False, mc.LEX) == ([0, 1, 2, 4], [6, 27, 44, 6], [0, 0, 0, 0])
    # canonical: CGT is ACG's other strand, TAC is GTA's: ids 6 6 44 44 6 6, strands 0 1 0 1 0 1; ties go left
    assert _lists(b"ACGTACGT", 3, 2, True, mc.LEX) == ([0, 1, 2, 4], [6, 6, 44, 6], [0, 1, 0, 0])
    # h at k = 3 (m = 63): h(6) = 21, h(27) = 20, h(44) = 7, h(49) = 22 (6: ~6 & 63 = 57; 57 + 456 + 14592 = 15105 = 1 mod 64; 1 + 4 + 16 = 21)
    assert [mc.h(x, 3) for x in (6, 27, 44, 49)] == [21, 20, 7, 22]
    # forward keys 21 20 7 22 21 20: (21,20) (20,7) (7,22) (22,21) (21,20) -> 1 2 2 4 5
    assert _lists(b"ACGTACGT", 3, 2, False, mc.HASHED) == ([1, 2, 4, 5], [27, 44, 6, 27], [0, 0, 0, 0])
    # canonical keys 21 21 7 7 21 21: (21,21) (21,7) (7,7) (7,21) (21,21) -> 0 2 2 3 4
    assert _lists(b"ACGTACGT", 3, 2, True, mc.HASHED) == ([0, 2, 3, 4], [6, 44, 44, 6], [0, 0, 1, 0])


def test_poly_a_selects_the_first_position_of_every_run():
    for k, w, n in [(3, 2, 10), (5, 4, 30), (1, 7, 7), (4, 19, 100)]:
        nwin = n - k + 1
        we = min(w, nwin)
        for order in (mc.LEX, mc.HASHED):
            pos, ids, strand = _lists(b"A" * n, k, w, False, order)
            assert pos == list(range(nwin - we + 1)) and set(ids) == {0} and set(strand) == {0}
        # canonical: poly-A is the smaller strand of poly-T
        pos, ids, strand = _lists(b"T" * n, k, w, True, mc.LEX)
        assert pos == list(range(nwin - we + 1)) and set(ids) == {0} and set(strand) == {1}


def test_an_n_in_the_middle():
    # ACGTANCGTACG, k = 3: the windows at 3, 4, 5 hold the N; keys 6 27 44 - - - 27 44 49 6
    # runs of three: (6,27,44) (27,44,-) (44,-,-) (-,-,-) (-,-,27) (-,27,44) (27,44,49) (44,49,6) -> 0 1 2 . 6 6 6 9
    assert _lists(b"ACGTANCGTACG", 3, 3, False, mc.LEX) == ([0, 1, 2, 6, 9], [6, 27, 44, 27, 6], [0, 0, 0, 0, 0])
    assert _lists(b"NNNNN", 3, 2, True, mc.LEX) == ([], [], [])
    assert _lists(b"ACNGT", 3, 2, True, mc.HASHED) == ([], [], [])


def test_fewer_positions_than_w_is_one_run():
    assert _lists(b"ACGTA", 3, 5, False, mc.LEX) == ([0], [6], [0])                  # 6 27 44: one run of three
    assert _lists(b"TTTAAA", 3, 200, False, mc.LEX) == ([3], [0], [0])               # 63 60 48 0
    assert _lists(b"AC", 3, 2, False, mc.LEX) == ([], [], []) and _lists(b"", 1, 1, True, mc.LEX) == ([], [], [])
    assert _lists(b"ACG", 3, 1, False, mc.LEX) == ([0], [6], [0])


@pytest.mark.parametrize("k", [1, 2, 3, 4, 5, 6])
def test_h_is_a_bijection(k):
    n = 4 ** k
    images = [mc.h(x, k) for x in range(n)]
    assert sorted(images) == list(range(n))
    assert mc.h_array(np.arange(n, dtype=np.uint64), k).tolist() == images


def test_h_array_equals_h_at_large_k():
    rng = np.random.Generator(np.random.PCG64(31))
    for k in (8, 15, 16, 17, 21, 31):
        ids = rng.integers(0, 4 ** k, size=200, dtype=np.uint64)
        ids[:3] = [0, 4 ** k - 1, 4 ** k // 2]
        assert mc.h_array(ids, k).tolist() == [mc.h(int(x), k) for x in ids]


def test_the_vectorised_runs_are_the_plain_runs():
    rng = np.random.Generator(np.random.PCG64(32))
    for trial in range(300):
        n, w = int(rng.integers(0, 40)), int(rng.integers(1, 12))
        keys = rng.integers(0, 5, size=n).astype(np.uint64)                          # (many ties)
        keys[rng.random(n) < 0.25] = mc.INF
        assert mc.select_runs(keys, w).tolist() == mc.select_runs_plain(keys, w), (keys.tolist(), w)


def _select_per_position(keys, w):
    """the per-position form the kernel uses: L = the positions left of p, in a row, with a larger key, R = those right of p with a key
    at least as large, both inside the record and at most we - 1; p is selected iff its key is finite and L + R + 1 >= we"""
    keys = [int(x) for x in keys]
    nwin, inf = len(keys), int(mc.INF)
    we, chosen = min(w, nwin), []
    for p in range(nwin):
        if keys[p] == inf:
            continue
        left = right = 0
        while left < we - 1 and p - left - 1 >= 0 and keys[p - left - 1] > keys[p]:
            left += 1
        while right < we - 1 and p + right + 1 < nwin and keys[p + right + 1] >= keys[p]:
            right += 1
        if left + right + 1 >= we:
            chosen.append(p)
    return chosen


def test_the_per_position_form_is_the_run_form():
    rng = np.random.Generator(np.random.PCG64(37))
    for trial in range(3000):
        n, w = int(rng.integers(0, 48)), int(rng.integers(1, 14))
        keys = rng.integers(0, int(rng.integers(1, 9)), size=n).astype(np.uint64)       # (one to eight key values: ties everywhere)
        keys[rng.random(n) < rng.choice([0.0, 0.2, 0.6])] = mc.INF
        assert _select_per_position(keys, w) == mc.select_runs_plain(keys, w), (keys.tolist(), w)


def test_the_flat_batch_form_is_the_record_form():
    rng = np.random.Generator(np.random.PCG64(36))
    records = []
    for i in range(400):
        kind = i % 7
        records.append(b"" if kind == 3 else b"N" * 25 if kind == 5 else mc.random_record(rng, int(rng.integers(20, 41)), 0.03))
    bases, offsets = mc.pack(records)
    for k, w, canonical, order in [(7, 5, True, mc.HASHED), (3, 18, False, mc.LEX), (16, 5, True, mc.LEX)]:
        want = mc.batch_minimizers(records, k, w, canonical, order)
        got = mc.batch_minimizers_flat(bases, offsets, k, w, canonical, order)
        assert all(g.dtype == x.dtype and g.tolist() == x.tolist() for g, x in zip(got, want))
        assert int(want[0].sum()) > 400 and int((want[0] == 0).sum()) >= 2 * 57


def test_every_run_with_a_finite_key_holds_a_selected_position():
    rng = np.random.Generator(np.random.PCG64(33))
    for k, w, canonical, order in [(3, 5, True, mc.LEX), (8, 10, False, mc.HASHED), (15, 19, True, mc.HASHED), (2, 3, False, mc.LEX)]:
        rec = mc.random_record(rng, 600, 0.05)
        has, ids, _ = mc.positions(rec, k, canonical)
        pos, _, _ = mc.record_minimizers(rec, k, w, canonical, order)
        chosen = np.zeros(has.size, dtype=bool)
        chosen[pos] = True
        assert not np.any(chosen & ~has)
        we = min(w, has.size)
        runs = 0
        for s in range(has.size - we + 1):
            if has[s:s + we].any():
                runs += 1
                assert chosen[s:s + we].any(), (k, w, s)
        assert runs > 100


def test_w_one_selects_every_position_with_an_id():
    rng = np.random.Generator(np.random.PCG64(34))
    rec = mc.random_record(rng, 500, 0.03)
    for k, canonical, order in [(1, False, mc.LEX), (4, True, mc.HASHED), (17, True, mc.LEX)]:
        has, ids, strand = mc.positions(rec, k, canonical)
        pos, got_ids, got_strand = mc.record_minimizers(rec, k, 1, canonical, order)
        assert pos.tolist() == np.flatnonzero(has).tolist() and 0 < pos.size < has.size
        assert got_ids.tolist() == ids[has].tolist() and got_strand.tolist() == strand[has].tolist()


def test_random_sequence_selects_about_two_in_w_plus_one():
    rng = np.random.Generator(np.random.PCG64(35))
    rec = mc.random_record(rng, 200000)
    for w in (5, 10, 19):
        pos, _, _ = mc.record_minimizers(rec, 15, w, True, mc.HASHED)
        assert abs(pos.size / (len(rec) - 14) - 2.0 / (w + 1)) < 0.01


def test_a_residue_outside_acgtn_is_refused():
    for bad in (b"ACGTRACGT", b"acgt", b"ACG T"):
        with pytest.raises(ValueError):
            mc.record_minimizers(bad, 3, 2)
