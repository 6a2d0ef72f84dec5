"""GPU: kdb_gram -- exact sums and Gram matrix of count vectors in HBM -- against Python integers, and the layers above it
(distance.moments / profile_distances / the `distance` command)."""
import ctypes
import io
import os
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INPUTS = os.path.join(ROOT, "tests", "golden", "inputs")


def _header_constant(name):
    text = open(os.path.join(ROOT, "include", "kdbhip.h")).read()
    return int(re.search(r"#define\s+%s\s+(\d+)" % name, text).group(1))


GRAM_MAX = _header_constant("KDB_GRAM_MAX")
B = _header_constant("KDB_GRAM_BLOCK")
WG_BINS = _header_constant("KDB_GRAM_WG_BINS")


@pytest.fixture(scope="module")
def dev(gpu_engine_cls):
    import torch
    from kmerdb_amd import _abi, distance

    class Dev:
        lib = _abi.lib()

        @staticmethod
        def upload(a):
            return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64)).to("cuda:0")

        @staticmethod
        def gram(tensors, nbins=None):
            torch.cuda.synchronize(0)
            return distance.gram([t.data_ptr() for t in tensors], tensors[0].numel() if nbins is None else nbins)[:2]

        @classmethod
        def raw(cls, ptrs, n, nbins):
            """the C call with arguments as given -> status"""
            arr = (ctypes.c_void_p * max(len(ptrs), 1))(*[ctypes.c_void_p(p) for p in ptrs])
            sums = (ctypes.c_uint64 * (2 * max(n, 1)))()
            g = (ctypes.c_uint64 * (2 * max(n, 1) ** 2))()
            torch.cuda.synchronize(0)
            return cls.lib.kdb_gram(0, arr, n, nbins, sums, g, None)
    return Dev


def _expected(vs):
    o = [v.astype(object) for v in vs]
    return [int(a.sum()) for a in o], [[int(np.dot(a, b)) for b in o] for a in o]


def _counts(rng, nbins):
    return (rng.poisson(3.0, nbins) * rng.integers(0, 2, nbins)).astype(np.uint64)


@pytest.mark.parametrize("nbins", [1, 2, 3, 63, 64, 65, 4 ** 5, WG_BINS - 1, WG_BINS, WG_BINS + 1, 4 ** 10 + 1])
def test_lengths_at_lane_wave_workgroup_and_grid_edges(dev, nbins):
    rng = np.random.default_rng(nbins)
    vs = [_counts(rng, nbins) for _ in range(3)]
    vs[2][-1] = np.uint64(7)                              # (the last bin counts)
    assert dev.gram([dev.upload(v) for v in vs]) == _expected(vs)


@pytest.mark.parametrize("n", [1, 2, B, B + 1, 2 * B + 1, GRAM_MAX])
def test_vector_counts_at_block_edges_fill_both_triangles(dev, n):
    nbins = 4 ** 6
    rng = np.random.default_rng(100 + n)
    vs = [_counts(rng, nbins) for _ in range(n)]
    s, G = dev.gram([dev.upload(v) for v in vs])
    want_s, want_G = _expected(vs)
    assert s == want_s and G == want_G
    assert all(G[i][j] == G[j][i] for i in range(n) for j in range(n))


def test_the_same_pointer_twice(dev):
    rng = np.random.default_rng(5)
    a, b = dev.upload(_counts(rng, 4 ** 6)), dev.upload(_counts(rng, 4 ** 6))
    for order in ([a, a], [a, b, a], [b, a, b, b, a, a]):
        s, G = dev.gram(order)
        for i, x in enumerate(order):
            for j, y in enumerate(order):
                if x is y:
                    assert G[i][j] == G[i][i] == G[j][j] and s[i] == s[j]


def test_values_zeros_carries_and_both_multiply_paths(dev):
    nbins = 4 ** 6 + 77
    rng = np.random.default_rng(9)
    zeros = np.zeros(nbins, dtype=np.uint64)
    # below 2^32 with many 2^32 - 1: the products' low words wrap and carry
    big32 = np.where(rng.integers(0, 2, nbins) == 1, np.uint64(2 ** 32 - 1), rng.integers(0, 2 ** 32, nbins, dtype=np.uint64)).astype(np.uint64)
    big32b = np.where(rng.integers(0, 3, nbins) > 0, np.uint64(2 ** 32 - 1), np.uint64(12345)).astype(np.uint64)
    # one value >= 2^32 in a single lane of an otherwise small wave: that wave takes the full product, its neighbours the short one
    one_big = _counts(rng, nbins)
    one_big[WG_BINS + 130 + 17] = np.uint64(2 ** 32 + 5)
    small = _counts(rng, nbins)
    vs = [zeros, big32, big32b, one_big, small]
    assert dev.gram([dev.upload(v) for v in vs]) == _expected(vs)
    # 2^63 in one bin of each of two vectors: a product of 2^126
    p, q = _counts(rng, nbins), _counts(rng, nbins)
    p[300] = q[300] = np.uint64(2 ** 63)
    s, G = dev.gram([dev.upload(p), dev.upload(q)])
    assert (s, G) == _expected([p, q]) and G[0][1] >= 2 ** 126
    # ... and in the vectors' last bins, which the tail kernel takes
    p[-1], q[-1] = np.uint64(2 ** 62), np.uint64(2 ** 63 - 1)
    p[300] = q[300] = np.uint64(0)                       # (else q's sum would pass 2^64)
    assert dev.gram([dev.upload(p), dev.upload(q)]) == _expected([p, q])


def test_a_sum_of_two_to_the_64_is_refused(dev):
    from kmerdb_amd import _abi
    v = np.zeros(4 ** 6, dtype=np.uint64)
    v[10] = v[4000] = np.uint64(2 ** 63)
    t, ok = dev.upload(v), dev.upload(np.ones(4 ** 6, dtype=np.uint64))
    assert dev.raw([ok.data_ptr(), t.data_ptr()], 2, 4 ** 6) == _abi.KDB_ERR_ARG
    v[4000] = np.uint64(2 ** 63 - 1)                      # 2^64 - 1 is fine
    t = dev.upload(v)
    assert dev.gram([ok, t]) == _expected([np.ones(4 ** 6, dtype=np.uint64), v])


def test_argument_errors(dev):
    from kmerdb_amd import _abi
    t = dev.upload(np.arange(4 ** 4, dtype=np.uint64))
    p = t.data_ptr()
    assert dev.raw([p], 1, 4 ** 4) == _abi.KDB_OK
    assert dev.raw([p], 0, 4 ** 4) == _abi.KDB_ERR_ARG
    assert dev.raw([p] * (GRAM_MAX + 1), GRAM_MAX + 1, 4 ** 4) == _abi.KDB_ERR_ARG
    assert dev.raw([p, p + 8], 2, 4 ** 4 - 1) == _abi.KDB_ERR_ARG          # a pointer off by 8 bytes
    assert dev.raw([p], 1, 0) == _abi.KDB_ERR_ARG
    assert dev.raw([p, 0], 2, 4 ** 4) == _abi.KDB_ERR_ARG                  # NULL


def test_inputs_stay_as_they_were_and_two_calls_agree(dev):
    import torch
    rng = np.random.default_rng(11)
    vs = [_counts(rng, 4 ** 8 + 3) for _ in range(B + 2)]
    ts = [dev.upload(v) for v in vs]
    first = dev.gram(ts)
    second = dev.gram(ts)
    torch.cuda.synchronize(0)
    assert first == second == _expected(vs)
    for v, t in zip(vs, ts):
        assert np.array_equal(t.cpu().numpy().view(np.uint64), v)


def test_moments_takes_engines_tensors_and_host_arrays_without_copying_a_table_back(dev, gpu_engine_cls):
    from kmerdb_amd import distance, reader
    k = 7
    engines = [gpu_engine_cls(k), gpu_engine_cls(k)]
    try:
        for eng, f in zip(engines, ("reads150.fq", "ragged_n.fq")):
            for bases, offsets, _ in reader.iter_blocks(os.path.join(INPUTS, f)):
                eng.submit(bases, offsets)
        rng = np.random.default_rng(3)
        host = _counts(rng, 4 ** k)
        tens_src = _counts(rng, 4 ** k)
        before = [e.get_option("d2h_bytes") for e in engines]
        s, G = distance.moments([engines[0], host, engines[1], dev.upload(tens_src)])
        assert [e.get_option("d2h_bytes") for e in engines] == before
        vs = [engines[0].finish()[0], host, engines[1].finish()[0], tens_src]
        assert int(vs[0].sum()) > 0 and int(vs[2].sum()) > 0
        assert (s, G) == _expected(vs)
        with pytest.raises(ValueError):
            distance.moments([engines[0], host[:-4]])
    finally:
        for e in engines:
            e.close()


@pytest.mark.parametrize("k", [5, 9])
def test_profile_distances_equals_the_moments_of_parsefile_vectors(dev, k):
    """tiny.fq, reads150.fq and contigs.fa at k = 5 and k = 9: the matrix equals from_moments of the moments of the three parse.parsefile
    vectors, bit for bit.  tiny.fq holds a record of 5 residues: at k = 9 parse.parsefile refuses the file (ValueError, as the reference raises at
    kmer.py:461-463 -- never a silent skip), so there are no three vectors to compare with; profile_distances must then refuse the samplesheet
    in the same way, and must still equal parsefile on the files parsefile takes."""
    from kmerdb_amd import distance, parse
    files = [os.path.join(INPUTS, f) for f in ("tiny.fq", "reads150.fq", "contigs.fa")]

    def both(fs):
        vs = [parse.parsefile(f, k, replace_with_none=True, canonicalize=True)[0] for f in fs]
        m, cols, md = distance.profile_distances(fs, k, metric="correlation", no_ambiguous=True)
        s, G = _expected(vs)
        assert m.tobytes() == distance.from_moments(s, G, 4 ** k, "correlation").tobytes()
        assert cols == [os.path.basename(f).split(".")[0] for f in fs]
        assert [d["total_kmers"] for d in md] == s and [d["filename"] for d in md] == fs

    refused = None
    try:
        parse.parsefile(files[0], k, replace_with_none=True, canonicalize=True)
    except ValueError as e:
        refused = str(e)
    assert (refused is None) == (k == 5)                  # (the 5-residue record)
    if refused is None:
        both(files)
    else:
        with pytest.raises(ValueError) as e:
            distance.profile_distances(files, k, metric="correlation", no_ambiguous=True)
        assert str(e.value) == refused and "shorter than k" in refused
        both(files[1:])


def test_distance_command_prints_the_formatted_matrix(dev, tmp_path, capsys):
    from kmerdb_amd import distance, fileutil, profile
    k = 4
    rng = np.random.default_rng(21)
    vs, paths = [], []
    for name in ("a", "b", "c"):
        v = _counts(rng, 4 ** k) + np.uint64(1)
        md = {"version": fileutil.VERSION, "metadata_blocks": 1, "k": k, "total_kmers": int(v.sum()), "unique_kmers": int(np.count_nonzero(v)),
              "unique_nullomers": 0, "sorted": False, "tags": [], "files": []}
        p = str(tmp_path / (name + ".%d.kdb" % k))
        fileutil.write_kdb(p, md, v)
        vs.append(v)
        paths.append(p)
    want = distance.format_matrix(distance.distance_matrix(vs, "correlation"), ["a", "b", "c"])
    capsys.readouterr()
    assert profile.main(["distance", "correlation"] + paths) == 0
    assert capsys.readouterr().out == want
    out = io.StringIO()
    distance.distances(paths[:2], "pearson", out=out)
    assert out.getvalue() == distance.format_matrix(distance.distance_matrix(vs[:2], "pearson"), ["a", "b"]) and out.getvalue().count("\n") == 1
    with pytest.raises(IOError):
        distance.distances([paths[0], str(tmp_path / "x.txt")], "correlation")
