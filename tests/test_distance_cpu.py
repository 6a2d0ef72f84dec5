"""CPU: kmerdb_amd.distance.from_moments and the output formatter -- the host half of `kmerdb distance` (the device half, kdb_gram, is
tests/test_gpu_gram.py).  The moments are exact integers, so every value must be the float64 nearest the true one or its neighbour: the same
formulas in fractions.Fraction with an 80-digit Decimal square root are the yardstick."""
import decimal
import math
from fractions import Fraction

import numpy as np
import pytest

from kmerdb_amd import distance


def _vectors(nbins, n, seed):
    """seeded count-like vectors; with n >= 2: vector 1 is a copy of vector 0; with n >= 5: vector 2 falls where vector 0 rises (r < 0)
    and vector 3 holds one count of 2^40"""
    rng = np.random.default_rng(seed)
    v = [rng.poisson(6.0, nbins).astype(np.uint64) * rng.integers(0, 2, nbins).astype(np.uint64) for _ in range(n)]
    if n >= 2:
        v[1] = v[0].copy()
    if n >= 5:
        v[2] = (np.uint64(40) - np.minimum(v[0], np.uint64(40))).astype(np.uint64)
        v[3][nbins // 3] = np.uint64(1 << 40)
    return v


def _moments(vs):
    o = [[int(x) for x in v] for v in vs]
    return [sum(a) for a in o], [[sum(x * y for x, y in zip(a, b)) for b in o] for a in o]


CASES = [(64, 1, 1), (64, 2, 2), (257, 5, 3), (4096, 5, 4), (1000, 2, 5)]


@pytest.fixture(scope="module")
def cases():
    out = []
    for nbins, n, seed in CASES:
        vs = _vectors(nbins, n, seed)
        s, G = _moments(vs)
        out.append((nbins, vs, s, G))
    return out


_CTX80 = decimal.Context(prec=80)


def _sqrt80(fr):
    """sqrt of a non-negative Fraction to 80 digits, as a Fraction"""
    d = _CTX80.sqrt(_CTX80.divide(decimal.Decimal(fr.numerator), decimal.Decimal(fr.denominator)))
    return Fraction(d)


def _exact(s, G, N, metric, i, j):
    """the metric's value as a Fraction (80-digit square root), or None where the denominator is zero"""
    gxx, gyy, gxy, sx, sy = Fraction(G[i][i]), Fraction(G[j][j]), Fraction(G[i][j]), Fraction(s[i]), Fraction(s[j])
    if metric in ("pearson", "correlation"):
        den = (N * gxx - sx * sx) * (N * gyy - sy * sy)
        if den == 0:
            return None
        r = (N * gxy - sx * sy) / _sqrt80(den)
        return r if metric == "pearson" else 1 - r
    if metric == "cosine":
        if gxx * gyy == 0:
            return None
        return 1 - gxy / _sqrt80(gxx * gyy)
    d2 = gxx + gyy - 2 * gxy
    return d2 if metric == "sqeuclidean" else _sqrt80(d2)


def _within_one_ulp(got, want):
    """|got - want| <= one ulp of got's neighbourhood, compared exactly"""
    if want == 0:
        return got == 0.0
    return abs(Fraction(got) - want) <= Fraction(math.ulp(float(want)))


@pytest.mark.parametrize("metric", distance.METRICS)
def test_from_moments_is_within_one_ulp_of_the_exact_value(cases, metric):
    saw_negative = saw_identical = False
    for nbins, vs, s, G in cases:
        m = distance.from_moments(s, G, nbins, metric)
        n = len(s)
        assert m.shape == (n, n) and m.dtype == np.float64
        for i in range(n):
            assert m[i][i] == (1.0 if metric == "pearson" else 0.0)
            for j in range(n):
                if i == j:
                    continue
                want = _exact(s, G, nbins, metric, min(i, j), max(i, j))
                assert want is not None
                assert _within_one_ulp(float(m[i][j]), want), (nbins, metric, i, j, float(m[i][j]), float(want))
                assert m[i][j] == m[j][i]
        if n >= 2:                                        # vectors 0 and 1 are identical
            saw_identical = True
            assert m[0][1] == (1.0 if metric == "pearson" else 0.0)
        if n >= 5 and metric == "pearson":
            saw_negative = saw_negative or m[0][2] < 0
    assert saw_identical and (saw_negative or metric != "pearson")


def test_a_count_of_two_to_the_forty_is_in_the_cases(cases):
    assert any(int(v.max()) == 1 << 40 for _, vs, _, _ in cases for v in vs)


def test_zero_denominators_give_nan_and_unknown_metrics_raise():
    const = np.full(64, 3, dtype=np.uint64)
    zero = np.zeros(64, dtype=np.uint64)
    other = np.arange(64, dtype=np.uint64)
    s, G = _moments([const, other, zero])
    for metric in ("pearson", "correlation"):
        m = distance.from_moments(s, G, 64, metric)
        assert math.isnan(m[0][1]) and math.isnan(m[1][0]) and math.isnan(m[1][2])
        assert m[0][0] == m[1][1] == (1.0 if metric == "pearson" else 0.0)
    m = distance.from_moments(s, G, 64, "cosine")
    assert math.isnan(m[1][2]) and math.isnan(m[0][2]) and not math.isnan(m[0][1])
    assert distance.from_moments(s, G, 64, "sqeuclidean")[0][2] == float(9 * 64)
    for bad in ("spearman", "EMD", "", "Pearson"):
        with pytest.raises(ValueError) as e:
            distance.from_moments(s, G, 64, bad)
        assert all(name in str(e.value) for name in distance.METRICS)


def test_metric_names_mean_what_scipy_means(cases):
    """What the names mean, not precision.  scipy's pdist in float64 against the exact value on these inputs, measured where this test was
    written (scipy 1.15.3): largest relative deviation 5.65e-16 (correlation 5.65e-16, cosine 3.15e-16, euclidean and sqeuclidean 0: the
    inputs are small counts whose sums float64 holds exactly, and the one count of 2^40 dominates its sums).  Ten times that is allowed, for
    builds that sum in another order -- far below the 1e-9 at which the inputs would have to be called ill-conditioned."""
    sd = pytest.importorskip("scipy.spatial.distance")
    tol = 10 * 5.65e-16
    assert tol <= 1e-9
    worst = 0.0
    for nbins, vs, s, G in cases:
        if len(vs) < 2:
            continue
        X = np.array(vs, dtype=np.float64)
        for metric in ("correlation", "cosine", "euclidean", "sqeuclidean"):
            want = sd.squareform(sd.pdist(X, metric=metric))
            got = distance.from_moments(s, G, nbins, metric)
            for i in range(len(vs)):
                for j in range(len(vs)):
                    if i == j or (i, j) in ((0, 1), (1, 0)):
                        # identical vectors: the exact value is 0; scipy's float sums may leave a few 1e-16 -- an absolute matter, not a relative one
                        assert abs(want[i][j] - got[i][j]) <= 1e-12
                        continue
                    dev = abs(want[i][j] - got[i][j]) / abs(got[i][j])
                    worst = max(worst, dev)
                    print("scipy deviation", nbins, metric, i, j, dev)
                    assert dev <= tol, (nbins, metric, i, j, want[i][j], got[i][j])
    print("largest relative deviation of scipy from the exact value:", worst)


def test_formatter_writes_what_pandas_to_csv_writes():
    pd = pytest.importorskip("pandas")
    dist = np.array([[0.0, 0.1 + 0.2, float("nan")], [0.1 + 0.2, 0.0, 1e-05], [float("nan"), 1e-05, 0.0]])
    cols = ["a", "b_1", "c"]
    assert distance.format_matrix(dist, cols) == pd.DataFrame(dist, columns=cols).to_csv(sep="\t", index=False)
    assert distance.format_matrix(dist, cols, ",") == pd.DataFrame(dist, columns=cols).to_csv(sep=",", index=False)
    two = np.array([[0.0, 0.1 + 0.2], [0.1 + 0.2, 0.0]])
    assert distance.format_matrix(two, ["a", "b"]) == "0.30000000000000004\n"          # print(dist[0][1]) of the reference
    with pytest.raises(ValueError):
        distance.format_matrix(dist, ["a", "b"])


def test_distance_matrix_raises_without_a_device():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is visible")
    from kmerdb_amd import _abi
    v = np.arange(64, dtype=np.uint64)
    with pytest.raises(_abi.KdbHipError):
        distance.distance_matrix([v, v[::-1].copy()])
    with pytest.raises(_abi.KdbHipError):
        distance.moments([v])
