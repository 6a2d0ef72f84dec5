"""tests/spectrum_cases.py proven on the CPU: the map agrees with the kernels' loops written out, the constants with the header, every
case is where it claims to be, and the expected ranks agree between two formulations.  No GPU."""
import itertools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import spectrum_cases as sc  # noqa: E402

LAY = sc.LAY


def _sorted_mid_ranks_doubled(v):
    """the second formulation: sort; a value's bins share the positions left + 1 .. right of the sorted vector, whose mean, doubled, is
    left + right + 1"""
    s = np.sort(v, kind="stable")
    return (np.searchsorted(s, v, side="left") + np.searchsorted(s, v, side="right") + 1).astype(np.uint64)


# ---- the constants and the map ----

def test_the_constants_are_the_headers():
    from kmerdb_amd import _abi
    for name in ("KDB_SPECTRUM_DENSE", "KDB_SPECTRUM_WG_BINS", "KDB_SPECTRUM_GRID_MAX", "KDB_SPECTRUM_LIST_GUESS"):
        assert getattr(_abi, name) == sc.header_constant(name)
    assert (sc.DENSE, sc.WG_BINS, sc.GRID_MAX, sc.GUESS) == (65536, 1024, 1024, 2 ** 20)
    assert (sc.NPRIV, sc.LDS_BINS, sc.RANK_LDS) == (16, 4096, 2048)
    assert sc.STRIDE2 == 2098253 and LAY.grid == sc.GRID_MAX and LAY.iterations == 3 and LAY.nbins - LAY.body == sc.TAIL


def _loops_written_out(nchunks, grid):
    """{chunk: (workgroup, wave, iteration)} by running every wave's loop as both kernels write it"""
    out = {}
    for wg in range(grid):
        for wave in range(sc.WAVES):
            chunk, it = wg * sc.WAVES + wave, 0
            while chunk < nchunks:
                assert chunk not in out
                out[chunk] = (wg, wave, it)
                chunk += grid * sc.WAVES
                it += 1
    return out


def _lane_loads_written_out(r):
    """(lane, slot) of the bin r of a chunk: p[lane] is the pair 2 lane, 2 lane + 1; p[lane + 64] the pair 128 + 2 lane, + 1"""
    for lane in range(64):
        for slot, at in enumerate((2 * lane, 2 * lane + 1, 2 * (lane + 64), 2 * (lane + 64) + 1)):
            if at == r:
                return lane, slot


@pytest.mark.parametrize("nbins,cap", [(1, 4), (255, 4), (256, 4), (77 + 256 * 9, 2), (256 * 23, 3), (2 * 5 * 1024 + 1024 + 77, 5), (4 ** 10 + 1, sc.GRID_MAX),
                                       (sc.STRIDE2, sc.GRID_MAX)])
def test_the_map_is_the_kernels_loop(nbins, cap):
    lay = sc.Layout(nbins, cap)
    assert lay.grid == max(1, min(-(-lay.nchunks // 4), cap))
    loops = _loops_written_out(lay.nchunks, lay.grid)
    assert sorted(loops) == list(range(lay.nchunks))                       # every chunk once
    assert lay.iterations == max([it for _, _, it in loops.values()] + [0]) + 1
    step = max(1, nbins // 3000)
    for b in itertools.chain(range(0, nbins, step), range(max(0, nbins - 600), nbins)):
        w = lay.where(b)
        if w is None:
            assert b >= (nbins // 256) * 256 and b - lay.body < 256            # thread b - body of workgroup 0
            continue
        assert (w.workgroup, w.wave, w.iteration) == loops[w.chunk]
        assert (w.lane, w.slot) == _lane_loads_written_out(b % 256)
        assert lay.bin(w.iteration, w.workgroup, w.wave, w.lane, w.slot) == b
        assert b in lay.slot_bins(w.chunk, w.slot) and lay.slot_bins(w.chunk, w.slot)[w.lane] == b
        assert lay.iteration_of([b])[0] == w.iteration
    later = lay.later_bins()
    assert later.size == max(0, nbins - min(4 * lay.grid * 256, lay.body))
    assert all(lay.where(int(b)) is None or lay.where(int(b)).iteration >= 1 for b in later[::97])


def test_the_old_suites_longest_vector_strides_by_one_tail_bin_only():
    """what tests/test_gpu_spectrum.py reaches: 4^10 + 1 bins are one full stride, no second iteration"""
    lay = sc.Layout(4 ** 10 + 1)
    assert lay.iterations == 1 and lay.grid == sc.GRID_MAX and lay.nbins - lay.body == 1


# ---- the cases ----

@pytest.mark.parametrize("name", sorted(sc.CASES))
def test_expected_ranks_agree_with_sorted_mid_ranks_and_sum_to_n_n_plus_1(name):
    v, _ = sc.case(name)
    want = sc.expected_ranks(v)
    assert np.array_equal(want, _sorted_mid_ranks_doubled(v))
    n = v.size
    assert sum(int(x) for x in np.add.reduceat(want, np.arange(0, n, 4096))) == n * (n + 1)
    values, mult = sc.expected_spectrum(v)
    assert int(mult.sum()) == n and np.all(np.diff(values.astype(object)) > 0)


@pytest.mark.parametrize("name", ["a_second_iteration_in_every_tier", "f_table_edges_in_later_iterations"])
def test_large_values_lie_in_later_iterations_only_and_add_up_across_them(name):
    v, claims = sc.case(name)
    first = v[:4 * LAY.grid * 256]
    assert int(first.max()) < sc.NPRIV and np.count_nonzero(first) > 0              # iteration 0: zeros and small values
    large = np.flatnonzero(v >= sc.NPRIV)
    assert set(np.unique(LAY.iteration_of(large)).tolist()) == {-1, 1, 2}
    assert sorted(set(v[large].tolist())) == sorted(claims["values"])
    for x, bins in claims["placed"].items():
        assert all(int(v[b]) == x for b in bins)
        at = np.flatnonzero(v == np.uint64(x))
        its = LAY.iteration_of(at)
        where = [LAY.where(int(b)) for b in at[its >= 0][::17]]
        assert {1, 2, -1} <= set(its.tolist())                                       # both later iterations and the tail
        assert len({w.workgroup for w in where if w.iteration == 1}) > 100           # many workgroups
        assert {LAY.where(int(b)).wave for b in at[its == 2]} == {0, 1, 2, 3} and all(LAY.where(int(b)).workgroup == 0 for b in at[its == 2])
        assert at.size > 1000                                                        # a multiplicity no single workgroup or iteration holds
    if name.startswith("a"):
        for tier, (lo, hi) in {"lds": (sc.NPRIV, sc.LDS_BINS), "global": (sc.LDS_BINS, sc.DENSE), "list": (sc.DENSE, 2 ** 64)}.items():
            assert len(sc.TIER_VALUES[tier]) >= 3 and all(lo <= x < hi for x in sc.TIER_VALUES[tier])
    else:
        assert {sc.RANK_LDS - 1, sc.RANK_LDS, sc.RANK_LDS + 1, sc.DENSE - 1, sc.DENSE} <= set(claims["values"])
    tail = v[LAY.body:]
    assert np.count_nonzero(tail >= sc.NPRIV) >= 2 * len(claims["values"]) - 2 and np.count_nonzero(tail[64:] >= sc.NPRIV) >= 1


def test_partial_merges_are_proper_subsets_in_both_tiers_and_iterations():
    v, claims = sc.case("b_partial_merges")
    seen = set()
    for m in claims["merges"]:
        chunk = LAY.chunk_of(m.iteration, m.workgroup, m.wave)
        w = LAY.where(int(LAY.slot_bins(chunk, m.slot)[0]))
        assert (w.iteration, w.workgroup, w.wave, w.slot, w.lane) == (m.iteration, m.workgroup, m.wave, m.slot, 0)
        n_mid, first, shared, x0, n_small, n_list = sc.merge_facts(v, chunk, m.slot)
        assert (n_mid, first, n_small, n_list) == (64, 0, 0, 0)                      # the whole wave takes the middle branch
        assert shared == m.shared and 2 <= shared <= 63                              # lane 0's value: a proper subset of the lanes
        lo, hi = (sc.NPRIV, sc.LDS_BINS) if m.tier == "lds" else (sc.LDS_BINS, sc.DENSE)
        vals = v[LAY.slot_bins(chunk, m.slot)]
        assert np.all((vals >= lo) & (vals < hi)) and int(vals.max()) - int(vals.min()) <= 24
        others = [s for s in range(4) if s != m.slot]
        assert all(int(v[LAY.slot_bins(chunk, s)].max()) < sc.NPRIV for s in others)
        seen.add((m.tier, m.iteration, m.shared))
    assert seen == {(t, i, s) for t in ("lds", "global") for i in (0, 1) for s in sc.SHARED_COUNTS}
    firsts = set()
    for m in claims["mixed"]:
        chunk = LAY.chunk_of(m.iteration, m.workgroup, m.wave)
        n_mid, first, shared, x0, n_small, n_list = sc.merge_facts(v, chunk, m.slot)
        assert n_mid >= 4 and n_small >= 1 and n_list >= 1 and n_mid + n_small + n_list == 64     # all three branches of tally()
        assert first == m.shared != 0                                                # the first lane of the middle branch is not lane 0
        assert 2 <= shared < n_mid                                                   # and a proper subset of that branch holds its value
        assert (x0 < sc.LDS_BINS) == (m.tier == "lds")
        vals = v[LAY.slot_bins(chunk, m.slot)]
        mid = vals[(vals >= sc.NPRIV) & (vals < sc.DENSE)]
        assert np.any(mid < sc.LDS_BINS) and np.any(mid >= sc.LDS_BINS)              # both tallied tiers among the others
        firsts.add((m.iteration, m.tier, first))
    assert len(firsts) == 12 and {i for i, _, _ in firsts} == {0, 1}
    chunks = [LAY.chunk_of(m.iteration, m.workgroup, m.wave) for m in claims["merges"] + claims["mixed"]]
    assert len(set(chunks)) == len(chunks)
    rest = np.ones(v.size, dtype=bool)
    for c in chunks:
        rest[c * 256:(c + 1) * 256] = False
    assert int(v[rest].max()) < sc.NPRIV


@pytest.mark.parametrize("moved", [0, 1])
def test_one_large_value_per_wave_in_each_slot(moved):
    name = "c_one_large_value_per_wave" + ("_moved_a_slot" if moved else "")
    v, claims = sc.case(name)
    seen_large, seen_15 = set(), set()
    touched = np.zeros(v.size, dtype=bool)
    for s in claims["singles"]:
        chunk = LAY.chunk_of(s.iteration, s.workgroup, s.wave)
        vals = v[chunk * 256:(chunk + 1) * 256]
        b = LAY.bin(s.iteration, s.workgroup, s.wave, s.lane, s.slot)
        w = LAY.where(b)
        assert (w.chunk, w.iteration, w.wave, w.lane, w.slot) == (chunk, s.iteration, s.wave, s.lane, s.slot) and int(v[b]) == s.value
        if s.value >= sc.NPRIV:
            assert np.count_nonzero(vals >= sc.NPRIV) == 1                           # the only one of its wave
            seen_large.add((s.iteration, s.wave, s.slot))
        else:
            assert s.value == sc.NPRIV - 1 and np.count_nonzero(vals) == 1           # alone among zeros
            seen_15.add((s.iteration, s.wave, s.slot))
        touched[b] = True
    every = {(i, w, s) for i in (0, 1) for w in range(4) for s in range(4)}
    assert seen_large == every and seen_15 == every
    assert int(v[~touched].max()) < sc.NPRIV
    assert {s.value for s in claims["singles"]} == set(sc.SINGLE_VALUES) | {sc.NPRIV - 1}
    # the other vector: the same values, each one slot further in the same lane of the same wave
    other, other_claims = sc.case("c_one_large_value_per_wave" + ("" if moved else "_moved_a_slot"))
    assert np.array_equal(np.sort(v), np.sort(other)) and not np.array_equal(v, other)
    for s, o in zip(claims["singles"], other_claims["singles"]):
        assert (s.iteration, s.workgroup, s.wave, s.lane, s.value) == (o.iteration, o.workgroup, o.wave, o.lane, o.value) and (s.slot - o.slot) % 4 in (1, 3)


@pytest.mark.parametrize("name,n_large", zip(["d_list_length_guess", "d_list_length_guess_plus_1", "d_list_length_guess_plus_a_workgroup"], sc.LIST_LENGTHS))
def test_list_lengths_at_and_past_the_guess(name, n_large):
    v, claims = sc.case(name)
    large = v >= sc.DENSE
    assert int(np.count_nonzero(large)) == n_large == claims["n_large"]
    assert sc.LIST_LENGTHS == (sc.GUESS, sc.GUESS + 1, sc.GUESS + sc.WG_BINS + 5)
    # nearly every wave holds large and small values side by side in every slot: wherever the list ends, it ends inside a reservation
    per_slot = large[:LAY.body].reshape(LAY.nchunks, 2, 64, 2).sum(axis=2)              # [chunk][a or b][x or y]: lanes that reserve
    assert np.count_nonzero((per_slot > 0) & (per_slot < 64)) > 0.999 * per_slot.size
    assert np.count_nonzero(large[LAY.body:]) > 0 and int(v[~large].max()) < sc.NPRIV


def test_many_distinct_large_values():
    v, claims = sc.case("e_many_distinct_large_values")
    large = v[v >= sc.DENSE]
    distinct, mult = np.unique(large, return_counts=True)
    assert distinct.size == claims["distinct"] > sc.GUESS and distinct.size < 2 ** 32
    assert int(mult.max()) >= 3 and np.count_nonzero(mult > 1) > 1000 and large.size > distinct.size
    assert int(distinct[0]) == sc.DENSE and int(distinct[-1]) == sc.TOP
    present = set(distinct.tolist())
    low, pairs = claims["low"], claims["high_pairs"]
    assert low.size > sc.GUESS // 2 and all(int(x) in present for x in low[::501]) and all(int(x) in present for x in pairs[::501])
    assert np.array_equal(low & np.uint64(0xFFFFFFFF), pairs & np.uint64(0xFFFFFFFF)) and np.all(pairs >> np.uint64(32) != low >> np.uint64(32))
    same_high = claims["same_high"]
    assert same_high.size > 5000 and np.all(same_high >> np.uint64(32) == 7) and np.unique(same_high & np.uint64(0xFFFFFFFF)).size == same_high.size
    # the low 32 bits alone do not order them: the sorted distinct values, truncated, are not sorted
    assert np.count_nonzero(np.diff((distinct & np.uint64(0xFFFFFFFF)).astype(np.int64)) < 0) > 1000
    assert int(np.ceil(np.log2(distinct.size))) >= 21                                    # depth of the binary search


# ---- the wide cases ----

@pytest.mark.parametrize("nfull", sc.WIDE_SEGMENTS)
def test_wide_tables(nfull):
    t, lengths = sc.wide_table(nfull)
    n = sum(lengths)
    assert n == nfull * 2 ** 20 + sc.WG_BINS + sc.TAIL < 2 ** 32 and t.size == nfull + 1
    assert sc.WIDE_SEGMENTS[0] == 2048 and 2048 * 2 ** 20 + sc.WG_BINS + sc.TAIL == 2 ** 31 + sc.WG_BINS + sc.TAIL
    ranks, (values, mult) = sc.segment_ranks(t, lengths)
    assert sum(r * l for r, l in zip(ranks, lengths)) == n * (n + 1) and sum(mult) == n
    assert np.any(np.diff(t.astype(object)) < 0) and len(values) < t.size and min(mult[:-1]) >= 2 ** 20      # not monotone, with repeats
    for lo, hi in ((0, sc.NPRIV), (sc.NPRIV, sc.LDS_BINS), (sc.LDS_BINS, sc.DENSE), (sc.DENSE, 2 ** 32), (2 ** 32, 2 ** 64)):
        assert any(lo <= x < hi for x in values)
    assert {sc.RANK_LDS - 1, sc.RANK_LDS, sc.RANK_LDS + 1, sc.DENSE - 1, sc.DENSE, sc.DENSE + 1} <= set(values)
    assert sum(l for x, l in zip(t.tolist(), lengths) if x >= sc.DENSE) <= 2 ** 23 + sc.WIDE_LAST        # what the host has to sort
    wide = [r >= 2 ** 32 for r in ranks]
    assert wide[-1] and max(ranks) <= 2 * n
    if nfull == 2048:
        # 2 below + eq + 1 >= 2^32 with below + eq <= n = 2^31 + 1101 needs eq <= 2203: of segments of 2^20 bins only the short last can
        assert wide.count(True) == 1
    else:
        assert wide.count(True) >= (nfull + 1) / 2
        tiers = [(0, sc.RANK_LDS), (sc.RANK_LDS, sc.DENSE), (sc.DENSE, 2 ** 64)]        # LDS table, global table, binary search
        assert all(any(w and lo <= x < hi for w, x in zip(wide, t.tolist())) for lo, hi in tiers)
        assert all(any(not w and lo <= x < hi for w, x in zip(wide, t.tolist())) for lo, hi in tiers[:1])
