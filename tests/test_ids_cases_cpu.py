"""CPU: the helpers of tests/ids_cases.py do what the GPU tests of the window-id path rely on -- the expected-ids builder
equals the pure-Python restatement of kmer.shred, and the generated layouts reach every edge they are meant to reach."""
import numpy as np
import pytest

import ids_cases as ic
from ids_cases import T

ALL_K = list(range(1, 18))


def test_expected_window_ids_equal_py_shred(oracle):
    """Builder A against oracle.py_shred (replace_with_none=True: N-windows dropped), records of k, k + 1 and 40 residues and
    a few random lengths, with and without N, both strand modes."""
    rng = np.random.Generator(np.random.PCG64(5))
    letters = np.array(list("ACGTN"))
    checked = with_n = 0
    for k in (1, 2, 3, 5, 8, 13, 16, 17):
        lens = [k, k, k + 1, k + 1, 40, 40] + [int(x) for x in rng.integers(k, 60, size=4)]
        recs = ["".join(letters[rng.choice(5, size=n, p=[0.235] * 4 + [0.06])]) for n in lens]
        recs[0] = recs[0].replace("N", "A")                     # one record of k residues that has its window
        recs[4] = recs[4][:20] + "N" + recs[4][21:]
        bases, offsets = oracle.pack_records(recs)
        for canon in (True, False):
            got = ic.expected_window_ids(bases, offsets, k, canon)
            want = np.full(bases.size, ic.NO_WINDOW, dtype=np.uint64)
            for r, seq in enumerate(recs):
                ids, pos = oracle.py_shred(seq, k, replace_with_none=True, canonicalize=canon)
                for i, p in zip(ids, pos):
                    want[int(offsets[r]) + p] = i
            assert got.dtype == np.uint64 and np.array_equal(got, want), (k, canon, ic.describe_mismatch(got, want, offsets))
            # the last k - 1 positions of every record start no window
            for r in range(len(recs)):
                assert np.all(got[int(offsets[r + 1]) - (k - 1):int(offsets[r + 1])] == ic.NO_WINDOW)
        checked += len(recs)
        with_n += sum("N" in r for r in recs)
    assert checked >= 36 and with_n >= 12


@pytest.mark.parametrize("k", [1, 4, 17])
def test_expected_window_ids_equal_c_shred_per_record(oracle, k):
    """... and oracle.c_shred(record, k, canon, N_DROP) record by record, as it is defined, on a generated layout."""
    lay = ic.ragged_layout(k, 3)
    raw = lay.bases.tobytes()
    for canon in (True, False):
        want = np.full(lay.total, ic.NO_WINDOW, dtype=np.uint64)
        for s, e in zip(lay.offsets[:-1], lay.offsets[1:]):
            ids, pos = oracle.c_shred(raw[int(s):int(e)], k, canon, oracle.N_DROP)
            want[int(s) + pos.astype(np.int64)] = ids
        got = ic.expected_window_ids(lay.bases, lay.offsets, k, canon)
        assert np.array_equal(got, want), ic.describe_mismatch(got, want, lay.offsets)
        assert 0 < int(np.sum(got == ic.NO_WINDOW)) < lay.total // 4


def test_expected_window_ids_raise_what_the_oracle_raises(oracle):
    bases, offsets = oracle.pack_records(["ACGTACGT", "ACG"])
    with pytest.raises(oracle.OracleError) as ei:
        ic.expected_window_ids(bases, offsets, 4, True)
    assert ei.value.status == oracle.SHORT_READ
    bases, offsets = oracle.pack_records(["ACGTACGT", "ACGRACGT"])
    with pytest.raises(oracle.OracleError) as ei:
        ic.expected_window_ids(bases, offsets, 4, True)
    assert ei.value.status == oracle.BAD_RESIDUE
    bases, offsets = oracle.pack_records(["ACGTACGT", "ACNRNCGT"])      # every window with the R holds an N
    got = ic.expected_window_ids(bases, offsets, 4, False)
    assert [int(x) for x in np.flatnonzero(got != ic.NO_WINDOW)] == [0, 1, 2, 3, 4]


def test_describe_mismatch_names_position_record_and_edges():
    offsets = np.array([0, T - 5, T + 40, 2 * T], dtype=np.uint64)
    want = np.zeros(2 * T, dtype=np.uint64)
    assert ic.describe_mismatch(want.copy(), want, offsets) == ""
    got = want.copy()
    got[T + 3] = 7
    got[T + 9] = 7
    msg = ic.describe_mismatch(got, want, offsets)
    assert "2 of 32768 positions" in msg and "first at 16387" in msg and "record 1 = [16379, 16424) (position 8 of it)" in msg
    assert "+3 from the nearest tile edge" in msg and "+3 from the nearest chunk edge" in msg
    got = want.copy()
    got[T - 2] = 1
    assert "-2 from the nearest tile edge, -2 from the nearest chunk edge" in ic.describe_mismatch(got, want, offsets)


@pytest.mark.parametrize("k", ALL_K)
def test_ragged_family_reaches_every_edge(k):
    fam = ic.ragged_family(k)
    every_d = set(range(-ic.EDGE_REACH, ic.EDGE_REACH + 1))
    for lay in fam:
        lens = lay.lengths
        assert int(lay.offsets[0]) == 0 and int(lay.offsets[-1]) == lay.total == lay.bases.size
        assert lens.min() >= k and lens.max() <= k + ic.MAX_EXTRA, lay
        assert set(np.unique(lay.bases)) <= set(b"ACGTN")
        assert len(lens) > 1 and lens.min() != lens.max(), lay                    # ragged: the engine marks the record starts
    cov = ic.coverage(fam, k)
    assert cov["start_d"] == every_d
    assert cov["n_d"] >= every_d
    # the forced N's alone reach every distance (the sprinkled ones are not needed for it)
    forced = set()
    for lay in fam:
        assert all(lay.bases[p] == 78 for p in lay.forced_n)
        forced |= ic.edge_distances(lay.forced_n, lay.total)
    assert forced == every_d
    assert cov["start_chunk_offset"] == set(range(16))
    assert cov["k_records_on_an_edge"] >= ic.EDGE_REACH + 1                        # one across 3 T in every full layout
    assert {T - 1, T, T + 1, ic.RAGGED_TOTAL} == cov["totals"]
    assert ic.RAGGED_TOTAL % ic.CHUNK == 7 and abs(ic.RAGGED_TOTAL - (3 * T + 7)) <= 2 * ic.CHUNK
    # the forced record starts and the straddling records are where the generator says
    for d, lay in enumerate(fam[:ic.EDGE_REACH + 1]):
        starts = set(int(x) for x in lay.offsets)
        a = ic.straddle_lead(k, d)
        assert {T + d, 2 * T - d, 3 * T - a, 3 * T - a + k} <= starts
        assert (0 < a < k) if k > 1 else a == 0
        if 0 < d < k:
            assert T + d - k in starts


@pytest.mark.parametrize("k", ALL_K)
def test_uniform_layouts_and_their_rebatched_forms(k):
    lengths = ic.uniform_lengths(k)
    assert k in lengths and {150, T - 1, T, T + 1} <= set(lengths) and all(L >= k for L in lengths)
    assert set(lengths) == {L for L in (k, 5, 15, 16, 17, 31, 150, T - 1, T, T + 1) if L >= k}
    for L in lengths:
        lay = ic.uniform_layout(k, L)
        assert lay.total > 2 * T and lay.total == int(lay.offsets[-1]) and np.all(lay.lengths == L)
        assert set(np.unique(lay.bases)) <= set(b"ACGTN")
        n_frac = float(np.mean(lay.bases == 78))
        assert 0.002 < n_frac < 0.009, (L, n_frac)
        re = ic.rebatch_ragged(lay, k)
        assert re.bases is lay.bases and re.total == lay.total and int(re.offsets[0]) == 0 and int(re.offsets[-1]) == lay.total
        assert re.lengths.min() >= k and re.lengths.min() != re.lengths.max()
        nrec = len(lay.lengths)
        # one record a residue longer; the next one a residue shorter, or (L = k) joined with the one behind it
        changed = [L + 1, L - 1] if L > k else [L + 1, 2 * L - 1]
        assert sorted(int(x) for x in re.lengths) == sorted([L] * (nrec - len(changed) - (L == k)) + changed)


@pytest.mark.parametrize("k", ALL_K)
def test_single_records(k):
    lengths = ic.single_lengths(k)
    assert set(lengths) == {L for L in (k, 15, 16, 17, T - 1, T, T + 1, 2 * T + 9) if L >= k}
    for L in lengths:
        rec = ic.single_record(k, L)
        assert len(rec) == L and set(rec) <= set(b"ACGTN")
    assert b"N" in ic.single_record(k, 2 * T + 9) and b"N" in ic.single_record(k, T)


def test_graph_records_and_files(oracle, tmp_path):
    for kind, writer, suffix in (("uniform", ic.write_fastq, ".fq"), ("ragged", ic.write_fastq, ".fq"), ("long", ic.write_fasta, ".fa")):
        recs = ic.graph_records(kind)
        lens = [len(s) for _, s in recs]
        assert all(set(s) <= set("ACGT") for _, s in recs)
        if kind == "long":
            assert len(recs) == 3 and min(lens) > T
        else:
            assert 45000 < sum(lens) < 75000 and (min(lens) == max(lens)) == (kind == "uniform")
        path = str(tmp_path / (kind + suffix))
        writer(path, recs)
        assert list(oracle.read_records(path)) == recs
