"""GPU: kdb_size_factors -- median-of-ratios size factors by a radix select on the device -- against medians known from the construction
and against 50-digit decimals within a derived bound; kdb_scale_counts against numpy's IEEE arithmetic, bit for bit; and the layers above
them (matrix.size_factors / normalize / the .kdb driver, distance's normalize="DESeq2", the command line).

The accuracy bound.  With u = 2^-53 and Lmax the largest ln x in the call, eps = (n + 10) u Lmax: a device log within 1 ulp gives
<= 2 u Lmax, taken twice (the term of the sum and the term of the ratio); the n - 1 additions of the sum, its one division, the one
subtraction and the one averaging of the two middle values are each <= u 2 Lmax or less; an order statistic moves by no more than the
largest per-element error, so the median inherits the per-element bound.  Measured worst share of eps: see DESIGN section 13."""
import ctypes
import decimal
import io
import math
import os
import re
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INPUTS = os.path.join(ROOT, "tests", "golden", "inputs")
TOP = 2 ** 64 - 1
U = 2.0 ** -53


def _header_constant(name):
    text = open(os.path.join(ROOT, "include", "kdbhip.h")).read()
    return int(re.search(r"#define\s+%s\s+(\d+)" % name, text).group(1))


GRAM_MAX = _header_constant("KDB_GRAM_MAX")
WG_BINS = _header_constant("KDB_SIZEFACTORS_WG_BINS")
LENGTHS = [1, 2, 127, 128, 129, 513, 4 ** 6, WG_BINS - 1, WG_BINS, WG_BINS + 1]


@pytest.fixture(scope="module")
def dev(gpu_engine_cls):
    import torch
    from kmerdb_amd import _abi, matrix

    class Dev:
        lib = _abi.lib()
        KDB_OK, KDB_ERR_ARG = _abi.KDB_OK, _abi.KDB_ERR_ARG

        @staticmethod
        def upload(a):
            return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64)).to("cuda:0")

        @staticmethod
        def download(t):
            return t.cpu().numpy().view(np.uint64)

        @staticmethod
        def log_sf(tensors):
            """-> (ln s: float64[n], eligible)"""
            torch.cuda.synchronize(0)
            return matrix.size_factors_raw([t.data_ptr() for t in tensors], tensors[0].numel())[:2]

        @classmethod
        def raw(cls, ptrs, n, nbins):
            """kdb_size_factors with arguments as given -> (status, ln s, eligible)"""
            arr = (ctypes.c_void_p * max(len(ptrs), 1))(*[ctypes.c_void_p(p) for p in ptrs])
            out, m = (ctypes.c_double * max(n, 1))(), ctypes.c_uint64(12345)
            torch.cuda.synchronize(0)
            rc = cls.lib.kdb_size_factors(0, arr, n, nbins, out, ctypes.byref(m), None)
            return rc, list(out), m.value

        @classmethod
        def scale(cls, src, s, dst, as_float64=0):
            """kdb_scale_counts -> status"""
            torch.cuda.synchronize(0)
            return cls.lib.kdb_scale_counts(0, ctypes.c_void_p(src.data_ptr()), src.numel(), ctypes.c_double(s), ctypes.c_void_p(dst.data_ptr()), as_float64, None)
    return Dev


# ---- the select is exact: medians known from the construction ----

T_VALUES = (-3, -1, 2, 4)                  # y = 8 * 2^t: 1, 4, 32, 128 against x = 8; r_y = t ln 2 / 2, r_x = -r_y: gaps of 0.35 and more


def _grouped_case(nbins, mode, seed):
    """x is 8 and y is 8 * 2^t on the eligible bins, a zero in x or in y on the others (scattered through the body, and the last bin).  The
    sorted t of the m eligible bins change value at up to three places; `mode` puts one of them so that the lower middle rank is the first
    element of its group, the upper middle rank the last of its group, or the two middle ranks of an even m lie in different groups.
    -> (x, y, the sorted t list)"""
    rng = np.random.default_rng(seed)
    inel = rng.random(nbins) < 0.25
    inel[0] = False
    if nbins > 4:
        inel[1] = inel[-1] = True
    if mode == "between" and (nbins - int(inel.sum())) % 2 == 1:
        inel[nbins // 2] = not inel[nbins // 2]
    m = nbins - int(inel.sum())
    lo, hi = (m - 1) // 2, m // 2
    cuts = {"first": lo, "last": hi + 1, "between": hi}[mode]
    cuts = {cuts, m // 5, (4 * m) // 5 + 1}
    if mode != "between" and lo != hi:
        cuts.discard(hi)                                                   # (the two middle elements share a group)
    cuts = sorted(c for c in cuts if 1 <= c <= m - 1)
    ts = [T_VALUES[sum(1 for c in cuts if c <= i)] for i in range(m)]
    if m >= 8:                                                             # the construction does what it says
        if mode == "first":
            assert ts[lo - 1] < ts[lo] == ts[hi]
        elif mode == "last":
            assert ts[lo] == ts[hi] < ts[hi + 1]
        else:
            assert hi == lo + 1 and ts[lo] < ts[hi]
    x, y = np.full(nbins, 8, dtype=np.uint64), np.zeros(nbins, dtype=np.uint64)
    y[~inel] = [8 * 2 ** t if t >= 0 else 8 >> -t for t in rng.permutation(ts)]
    zero_in_x = inel & (rng.random(nbins) < 0.5)
    x[zero_in_x] = 0
    y[inel & ~zero_in_x] = 0
    y[zero_in_x] = rng.integers(0, 3, int(zero_in_x.sum())).astype(np.uint64) * np.uint64(16)
    return x, y, ts


# (one bin has no two middle ranks: six bins instead)
@pytest.mark.parametrize("nbins,mode", [(nb, mode) for nb in LENGTHS for mode in ("first", "last", "between") if (nb, mode) != (1, "between")] + [(6, "between")])
def test_the_median_rank_at_the_edges_of_its_group(dev, nbins, mode):
    x, y, ts = _grouped_case(nbins, mode, 1000 + nbins)
    m = len(ts)
    assert m == int(np.count_nonzero((x > 0) & (y > 0))) and m >= 1
    want = (ts[(m - 1) // 2] + ts[m // 2]) / 2 * (math.log(2.0) / 2)       # the median of t, times ln 2 / 2: a neighbouring rank is 0.35 away
    eps = (2 + 10) * U * math.log(128.0)
    got, eligible = dev.log_sf([dev.upload(x), dev.upload(y)])
    print("nbins", nbins, mode, "m", m, "want", want, "got", got.tolist(), "eps", eps)
    assert eligible == m
    assert abs(got[1] - want) <= eps and abs(got[0] + want) <= eps         # (x's ratios are y's with the other sign: the same ranks from the other end)


# ---- accuracy against 50-digit decimals ----

_CTX = decimal.Context(prec=50)
_LN = {}


def _ln(v):
    v = int(v)
    if v not in _LN:
        _LN[v] = _CTX.ln(decimal.Decimal(v))
    return _LN[v]


def _true_log_sf(vs):
    """ln s of every vector in 50-digit decimals, the exact median; -> (list of Decimal, eligible, Lmax)"""
    n = len(vs)
    eligible = np.ones(len(vs[0]), dtype=bool)
    for v in vs:
        eligible &= v > 0
    idx = np.flatnonzero(eligible)
    with decimal.localcontext(_CTX):
        logs = [[_ln(v[b]) for b in idx] for v in vs]
        mean = [sum(col, decimal.Decimal(0)) / n for col in zip(*logs)]
        out = []
        for j in range(n):
            r = sorted(a - l for a, l in zip(logs[j], mean))
            m = len(r)
            out.append((r[(m - 1) // 2] + r[m // 2]) / 2)
    return out, len(idx), float(max(max(row) for row in logs))


def _seeded_vectors(nbins, n, seed, twin=True):
    """a third of the bins zero in some sample, small counts elsewhere (every sample at a depth of its own), one count of 2^40 and one of
    2^64 - 1 among the eligible bins; twin: the last sample is the first with a few bins changed"""
    rng = np.random.default_rng(seed)
    vs = [(rng.poisson(3.0 + 2.0 * j, nbins) + 1).astype(np.uint64) for j in range(n)]
    if n >= 2 and twin:
        vs[-1] = vs[0].copy()
        vs[-1][:: 37] += np.uint64(1)
    zero = rng.random(nbins) < 1.0 / 3.0
    zero[[0, nbins // 2]] = False
    who = rng.integers(0, n, nbins)
    for j in range(n):
        vs[j][zero & (who == j)] = 0
    vs[0][0] = np.uint64(2 ** 40)
    vs[n - 1][nbins // 2] = np.uint64(TOP)
    return vs


_WORST = {"share": 0.0}


# (with two samples the near-identical pair is the whole call and the median ratio is 0: the cases without a twin have one that is not)
@pytest.mark.parametrize("nbins,n,twin", [(4 ** 6, 2, True), (4 ** 6, 3, True), (4 ** 6, 5, True), (513, 2, True), (513, 3, True), (513, 5, True),
                                          (4 ** 6, 2, False), (513, 3, False), (129, 17, False), (WG_BINS + 1, 17, True)])
def test_size_factors_within_the_bound_of_their_roundings(dev, nbins, n, twin):
    vs = _seeded_vectors(nbins, n, 7 * nbins + n, twin)
    want, m, lmax = _true_log_sf(vs)
    assert m > nbins // 2 and lmax == pytest.approx(64 * math.log(2.0))
    eps = (n + 10) * U * lmax
    ts = [dev.upload(v) for v in vs]
    got, eligible = dev.log_sf(ts)
    assert eligible == m
    with decimal.localcontext(_CTX):
        errs = [abs(decimal.Decimal(float(g)) - w) for g, w in zip(got, want)]
    share = float(max(errs)) / eps
    _WORST["share"] = max(_WORST["share"], share)
    print("nbins", nbins, "n", n, "m", m, "eps", eps, "worst error", float(max(errs)), "share of eps", share, "worst so far", _WORST["share"])
    assert all(float(e) <= eps for e in errs)
    again, _ = dev.log_sf(ts)                                              # run to run: the same bits
    assert again.tobytes() == got.tobytes()


@pytest.mark.parametrize("n", [1, 2, 3, 5, 17])
def test_the_same_vector_n_times_has_size_factor_one(dev, n):
    """every ratio is ln x - (n ln x) / n; for n = 1 that is exactly 0.0"""
    v = _seeded_vectors(513, 1, 3)[0]
    t = dev.upload(v)
    got, eligible = dev.log_sf([t] * n)
    assert eligible == int(np.count_nonzero(v))
    eps = (n + 10) * U * 64 * math.log(2.0)
    assert all(abs(g) <= eps for g in got)
    if n == 1:
        assert got.tobytes() == np.zeros(1).tobytes()                      # +0.0 exactly
        from kmerdb_amd import matrix
        sf, _ = matrix.size_factors([t])
        assert sf.tolist() == [1.0]


def test_no_eligible_bin_and_the_argument_ladder(dev):
    from kmerdb_amd import matrix
    x = np.array([1, 0, 3, 0] * 40, dtype=np.uint64)
    y = np.array([0, 2, 0, 0] * 40, dtype=np.uint64)
    tx, ty = dev.upload(x), dev.upload(y)
    rc, log_sf, m = dev.raw([tx.data_ptr(), ty.data_ptr()], 2, x.size)
    assert rc == dev.KDB_OK and m == 0 and all(math.isnan(v) for v in log_sf)
    with pytest.raises(ValueError, match="every k-mer contains at least one zero"):
        matrix.size_factors([tx, ty])
    with pytest.raises(ValueError, match="every k-mer contains at least one zero"):
        matrix.normalize([x, y])
    p = tx.data_ptr()
    assert dev.raw([p], 1, x.size)[0] == dev.KDB_OK
    for ptrs, n, nbins in (([p], 0, x.size), ([p] * (GRAM_MAX + 1), GRAM_MAX + 1, x.size), ([p], 1, 0), ([p], 1, 2 ** 36 + 1), ([0], 1, x.size),
                           ([p + 8], 1, x.size - 1), ([p, 0], 2, x.size)):
        assert dev.raw(ptrs, n, nbins)[0] == dev.KDB_ERR_ARG, (n, nbins)
    assert dev.raw([p] * GRAM_MAX, GRAM_MAX, x.size)[0] == dev.KDB_OK
    with pytest.raises(ValueError):
        matrix.size_factors([x, y[:-4]])


# ---- kdb_scale_counts ----

def _scale_counts(nbins, seed):
    rng = np.random.default_rng(seed)
    v = rng.integers(0, 1000, nbins).astype(np.uint64)
    v[:: 3] |= np.uint64(1)                                                # odd counts: halves, for the ties
    edge = [2 ** 53 - 1, 2 ** 53, 2 ** 53 + 1, 2 ** 53 + 3, 1, 3, 5, 7, 0, 2 ** 62 + 1, 2 ** 40 + 1]
    v[-min(nbins, len(edge)):] = np.array(edge[:min(nbins, len(edge))], dtype=np.uint64)
    return v


@pytest.mark.parametrize("s", [2.0, 0.75, 3.0, 1.0, 1.2345678901234567])
@pytest.mark.parametrize("nbins", LENGTHS)
def test_scaled_counts_are_numpys_bit_for_bit(dev, nbins, s):
    import torch
    v = _scale_counts(nbins, nbins)
    q = v.astype(np.float64) / np.float64(s)
    want = np.rint(q).astype(np.uint64)
    src = dev.upload(v)
    buf = torch.full((nbins + 2,), -1, dtype=torch.int64, device="cuda:0")             # (two words behind the output: they must stay)
    dst = buf[:nbins]
    assert dev.scale(src, s, dst) == dev.KDB_OK
    assert buf[nbins:].tolist() == [-1, -1]
    assert dev.download(dst).tobytes() == want.tobytes()
    assert dev.download(src).tobytes() == v.tobytes()
    fl = torch.zeros(nbins, dtype=torch.int64, device="cuda:0")
    assert dev.scale(src, s, fl, as_float64=1) == dev.KDB_OK                           # the float64 output: the quotient, not rounded
    assert dev.download(fl).tobytes() == q.tobytes()
    assert dev.scale(src, s, src) == dev.KDB_OK                                        # in place
    assert dev.download(src).tobytes() == want.tobytes()
    if s == 2.0:
        ties = (v % 2 == 1) & (v < 2 ** 53)
        assert ties.any() and np.all(want[ties] % 2 == 0)                              # halves went to the even neighbour


def test_a_quotient_of_two_to_the_63_and_a_bad_size_factor_are_refused(dev):
    v = _scale_counts(WG_BINS + 1, 5)
    v[7] = np.uint64(TOP)
    src = dev.upload(v)
    assert dev.scale(src, 1.0, src) == dev.KDB_ERR_ARG
    assert dev.download(src).tobytes() == v.tobytes()                                  # refused before anything was written
    assert dev.scale(src, 2.0, src.clone()) == dev.KDB_ERR_ARG                         # 2^64 / 2
    dst = src.clone()
    s = np.nextafter(np.float64(2.0), np.float64(3.0))                                 # 2^64 / s is the float64 below 2^63
    assert dev.scale(src, float(s), dst) == dev.KDB_OK and int(dev.download(dst)[7]) == int(np.float64(2.0 ** 64) / s) == 2 ** 63 - 2048
    for s in (0.0, -1.0, float("inf"), float("nan")):
        assert dev.scale(src, s, dst) == dev.KDB_ERR_ARG, s
    assert dev.lib.kdb_scale_counts(0, ctypes.c_void_p(src.data_ptr() + 8), 4, ctypes.c_double(1.0), ctypes.c_void_p(dst.data_ptr()), 0, None) == dev.KDB_ERR_ARG
    assert dev.lib.kdb_scale_counts(0, ctypes.c_void_p(src.data_ptr()), 0, ctypes.c_double(1.0), ctypes.c_void_p(dst.data_ptr()), 0, None) == dev.KDB_ERR_ARG
    assert dev.lib.kdb_scale_counts(0, None, 4, ctypes.c_double(1.0), ctypes.c_void_p(dst.data_ptr()), 0, None) == dev.KDB_ERR_ARG


# ---- the layers ----

def _host_stats(vs):
    n = len(vs)
    w = [v.astype(np.int64) for v in vs]
    out = {"S": [int(v.sum()) for v in w], "nnz": [int(np.count_nonzero(v)) for v in w]}
    for key in ("L1", "Linf", "ne", "both"):
        out[key] = [[0] * n for _ in range(n)]
    for i in range(n):
        for j in range(n):
            d = np.abs(w[i] - w[j])
            out["L1"][i][j], out["Linf"][i][j], out["ne"][i][j] = int(d.sum()), int(d.max()), int(np.count_nonzero(d))
            out["both"][i][j] = int(np.count_nonzero((w[i] > 0) & (w[j] > 0)))
    return out


def _rint(v, s):
    return np.rint(v.astype(np.float64) / np.float64(s)).astype(np.uint64)


def test_normalize_leaves_an_engines_table_and_a_callers_tensor_as_they_are(dev, gpu_engine_cls):
    import torch
    from kmerdb_amd import distance, matrix, reader
    k = 5
    engines = [gpu_engine_cls(k), gpu_engine_cls(k)]
    try:
        for eng, f in zip(engines, ("reads150.fq", "ragged_n.fq")):
            for bases, offsets, _ in reader.iter_blocks(os.path.join(INPUTS, f)):
                eng.submit(bases, offsets)
        outs, sf = matrix.normalize(engines)
        dist = distance.distance_matrix(engines, "braycurtis", normalize="DESeq2")
        sf2, eligible = matrix.size_factors(engines)
        vs = [e.finish()[0] for e in engines]
        assert sf.tobytes() == sf2.tobytes() and eligible == int(np.count_nonzero((vs[0] > 0) & (vs[1] > 0))) > 0
        assert sf[0] != 1.0 and sf[0] * sf[1] == pytest.approx(1.0, rel=1e-12)         # two samples: the ratios mirror each other
        norm = [_rint(v, s) for v, s in zip(vs, sf)]
        assert all(o.dtype == torch.int64 and dev.download(o).tobytes() == w.tobytes() for o, w in zip(outs, norm))
        assert any(w.tobytes() != v.tobytes() for w, v in zip(norm, vs))               # (so `finish` above saw tables that were not scaled)
        assert dist.tobytes() == distance.from_pairstats(_host_stats(norm), 4 ** k, "braycurtis").tobytes() and 0.0 < dist[0][1] < 1.0
    finally:
        for e in engines:
            e.close()
    ts = [dev.upload(v) for v in vs]
    outs, _ = matrix.normalize(ts, ints=False)
    assert all(dev.download(t).tobytes() == v.tobytes() for t, v in zip(ts, vs))
    assert all(o.dtype == torch.float64 and o.cpu().numpy().tobytes() == (v.astype(np.float64) / s).tobytes() for o, v, s in zip(outs, vs, sf))
    outs, _ = matrix.normalize(ts, inplace=True)
    assert all(o.data_ptr() == t.data_ptr() and dev.download(t).tobytes() == w.tobytes() for o, t, w in zip(outs, ts, norm))
    with pytest.raises(ValueError):
        matrix.normalize(vs, inplace=True)


def test_profile_distances_normalised_equals_the_separately_counted_vectors(dev):
    from kmerdb_amd import distance, matrix, parse
    files = [os.path.join(INPUTS, f) for f in ("reads150.fq", "contigs.fa", "ragged_n.fq")]
    vs = [parse.parsefile(f, 6, replace_with_none=True, canonicalize=True)[0] for f in files]
    for metric in ("braycurtis", "euclidean", "spearman"):
        m, cols, _ = distance.profile_distances(files, 6, metric=metric, no_ambiguous=True, normalize="DESeq2")
        want = distance.distance_matrix(vs, metric, normalize="DESeq2")
        assert m.tobytes() == want.tobytes() and cols == ["reads150", "contigs", "ragged_n"]
    sf, _ = matrix.size_factors(vs)
    print("size factors", sf.tolist())
    norm = [_rint(v, s) for v, s in zip(vs, sf)]
    assert any(w.tobytes() != v.tobytes() for w, v in zip(norm, vs))                   # (the normalisation is not the identity on these)
    assert distance.distance_matrix(vs, "braycurtis", normalize="DESeq2").tobytes() == distance.from_pairstats(_host_stats(norm), 4 ** 6, "braycurtis").tobytes()


def test_the_kdb_driver_and_the_command_line(dev, tmp_path, capsys):
    from kmerdb_amd import distance, fileutil, matrix, profile
    k = 3
    rng = np.random.default_rng(33)
    vs, paths = [], []
    for name, depth in (("a", 3.0), ("b", 11.0)):
        v = rng.poisson(depth, 4 ** k).astype(np.uint64)
        v[5 if name == "a" else 9] = 0
        md = {"version": fileutil.VERSION, "metadata_blocks": 1, "k": k, "total_kmers": int(v.sum()), "unique_kmers": int(np.count_nonzero(v)),
              "unique_nullomers": 0, "sorted": False, "tags": [], "files": []}
        p = str(tmp_path / (name + ".%d.kdb" % k))
        fileutil.write_kdb(p, md, v)
        vs.append(v)
        paths.append(p)
    sf, _ = matrix.size_factors(vs)
    assert sf[0] < 1.0 < sf[1]
    norm = [_rint(v, s) for v, s in zip(vs, sf)]
    out = io.StringIO()
    cols = matrix.matrix(paths, "DESeq2", out=out)
    assert out.getvalue() == "a\tb\n" + "".join("%d\t%d\n" % (int(x), int(y)) for x, y in zip(*norm))
    assert all(c.tobytes() == w.view(np.int64).tobytes() for c, w in zip(cols, norm))
    out = io.StringIO()
    matrix.matrix(paths, "DESeq2", out=out, no_normalized_ints=True, with_index=True, output_delimiter=",")
    q = [v.astype(np.float64) / s for v, s in zip(vs, sf)]
    assert out.getvalue() == ",a,b\n" + "".join("%d,%s,%s\n" % (i, repr(float(x)), repr(float(y))) for i, (x, y) in enumerate(zip(*q)))
    for method in ("from", "Frequency"):
        out = io.StringIO()
        matrix.matrix(paths, method, out=out)
        assert out.getvalue() == "a\tb\n" + "".join("%d\t%d\n" % (int(x), int(y)) for x, y in zip(*vs))
    out = io.StringIO()
    dist = distance.distances(paths, "euclidean", out=out, normalize="DESeq2")
    want = float(np.sqrt(((norm[0].astype(np.float64) - norm[1].astype(np.float64)) ** 2).sum()))
    assert dist[0][1] == pytest.approx(want, rel=1e-12) and out.getvalue() == repr(float(dist[0][1])) + "\n"
    # `python -m kmerdb_amd ...` is sys.exit(profile.main()): the same parser and dispatch, without a second process and its start-up
    assert profile.main(["distance", "euclidean", "--normalize", "DESeq2"] + paths) == 0
    assert capsys.readouterr().out == out.getvalue()
    assert profile.main(["matrix", "DESeq2"] + paths) == 0                             # (the same parser, in this process)
    assert capsys.readouterr().out == "a\tb\n" + "".join("%d\t%d\n" % (int(x), int(y)) for x, y in zip(*norm))
