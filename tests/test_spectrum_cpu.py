"""CPU: what stands above the spectrum kernels and needs no device -- util.get_histo's argument check, its `> 2` quirk and its size guard on a
stubbed spectrum(); the command line's new choices; the metric tables of kmerdb_amd.distance."""
import numpy as np
import pytest


@pytest.fixture
def stub_spectrum(monkeypatch):
    """spectrum.spectrum replaced by np.unique: get_histo's own logic without a device"""
    from kmerdb_amd import spectrum
    seen = []

    def fake(vector, device=0):
        assert isinstance(vector, np.ndarray) and vector.dtype == np.uint64
        seen.append(vector)
        values, mult = np.unique(vector, return_counts=True)
        return values.astype(np.uint64), mult.astype(np.uint64)
    monkeypatch.setattr(spectrum, "spectrum", fake)
    return seen


def test_get_histo_takes_a_list_only(stub_spectrum):
    from kmerdb_amd import util
    for bad in (np.array([1, 2, 3], dtype=np.uint64), (1, 2, 3), None, 3, "123"):
        with pytest.raises(TypeError):
            util.get_histo(bad)
    assert stub_spectrum == []


def test_get_histo_tallies_only_counts_above_two(stub_spectrum):
    """the reference's loop (kmerdb/util.py:100-116): a list of max + 1 entries, hist[c] += 1 only `if counts[i] > 2`"""
    from kmerdb_amd import util
    counts = [0, 0, 0, 1, 1, 2, 2, 2, 3, 3, 5, 9, 9, 9]
    want = [0] * 10
    for c in counts:
        if c > 2:
            want[c] += 1
    got = util.get_histo(counts)
    assert got == want == [0, 0, 0, 2, 0, 1, 0, 0, 0, 3] and type(got) is list and all(type(x) is int for x in got)
    assert util.get_histo([0, 1, 2, 2]) == [0, 0, 0]
    assert util.get_histo([0]) == [0]
    assert util.get_histo([4]) == [0, 0, 0, 0, 1]
    assert len(stub_spectrum) == 4


def test_get_histo_refuses_a_list_of_more_than_two_to_the_27_entries(stub_spectrum):
    from kmerdb_amd import util
    assert util.HISTO_MAX_ENTRIES == 2 ** 27
    with pytest.raises(ValueError, match=r"spectrum\(\)"):
        util.get_histo([1, 2, 3, 2 ** 27])                      # max + 1 = 2^27 + 1 entries
    with pytest.raises(ValueError, match=r"spectrum\(\)"):
        util.get_histo([0, 2 ** 64 - 1])


def test_the_command_line_accepts_spearman_and_spectrum(monkeypatch):
    from kmerdb_amd import distance, profile
    calls = []
    monkeypatch.setattr(distance, "distances", lambda inputs, metric, **kw: calls.append(("distance", list(inputs), metric, kw)))
    assert profile.main(["distance", "spearman", "a.kdb", "b.kdb"]) == 0
    assert calls == [("distance", ["a.kdb", "b.kdb"], "spearman", {"column_names": None, "output_delimiter": "\t", "device": 0})]
    with pytest.raises(SystemExit):
        profile.main(["distance", "kendall", "a.kdb", "b.kdb"])
    with pytest.raises(SystemExit):
        profile.main(["spectrum"])                               # at least one file


def test_the_spectrum_command_prints_count_and_bins_rows(monkeypatch, capsys):
    from kmerdb_amd import profile, spectrum

    class Kdb:
        counts = np.array([0, 0, 3, 2 ** 64 - 1], dtype=np.uint64)
    monkeypatch.setattr(profile.fileutil, "read_kdb", lambda p: Kdb)
    monkeypatch.setattr(spectrum, "spectrum", lambda v, device=0: (np.array([0, 3, 2 ** 64 - 1], dtype=np.uint64), np.array([2, 1, 1], dtype=np.uint64)))
    capsys.readouterr()
    assert profile.main(["spectrum", "x.4.kdb"]) == 0
    assert capsys.readouterr().out == "0\t2\n3\t1\n18446744073709551615\t1\n"
    assert profile.main(["spectrum", "--device", "0", "x.4.kdb", "y.4.kdb"]) == 0
    assert capsys.readouterr().out == "# x.4.kdb\n0\t2\n3\t1\n18446744073709551615\t1\n# y.4.kdb\n0\t2\n3\t1\n18446744073709551615\t1\n"


def test_metric_tables():
    from kmerdb_amd import distance
    assert distance.METRICS == ("pearson", "correlation", "cosine", "sqeuclidean", "euclidean")
    assert distance.RANK_METRICS == ("spearman",)
    assert set(distance.IDENTITY) == set(distance.METRICS)
    # rho is not a function of the COUNT moments: from_moments keeps refusing it
    with pytest.raises(ValueError):
        distance.from_moments([1, 2], [[1, 0], [0, 4]], 4, "spearman")
    with pytest.raises(ValueError, match="spearman"):
        distance.distance_matrix([np.zeros(4, dtype=np.uint64)] * 2, "kendall")


def test_spearman_of_too_many_bins_is_refused_before_any_device_is_asked_for(monkeypatch):
    from kmerdb_amd import distance

    def no(*a, **kw):
        raise AssertionError("device work")
    monkeypatch.setattr(distance, "_require_device", no)
    monkeypatch.setattr(distance, "moments", no)
    huge = np.broadcast_to(np.uint64(0), (2 ** 32,))            # (no memory behind it)
    with pytest.raises(ValueError, match="k <= 15"):
        distance.distance_matrix([huge, huge], "spearman")
    with pytest.raises(ValueError, match="k <= 15"):
        distance.profile_distances(["reads.fq"], 16, metric="spearman")
    with pytest.raises(ValueError):
        distance.rank_vectors([np.zeros(4, dtype=np.uint64), np.zeros(5, dtype=np.uint64)])
