"""CPU: the host half of the distances that are not moments -- kmerdb_amd.distance.from_pairstats on integers computed here, what the
metric names mean (scipy), the degenerate cases, the metric tables, the `distance` command's parser -- and the register budget of the two
sweeps of csrc/kdb_pairstats.hip.h, read from the compiler's own assembly (hipcc cross-compiles gfx950 without a GPU).  The device half
is tests/test_gpu_pairstats.py."""
import math
import os
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

INTEGER_METRICS = ("cityblock", "chebyshev", "braycurtis", "hamming", "matching", "jaccard", "dice", "rogerstanimoto", "sokalmichener",
                   "russellrao", "sokalsneath", "yule", "kulsinski")


def host_stats(vs):
    """kdb_pairstats' integers of small vectors, in Python ints"""
    vs = [[int(x) for x in v] for v in vs]
    n = len(vs)
    pair = lambda f: [[f(vs[i], vs[j]) for j in range(n)] for i in range(n)]
    return {"S": [sum(v) for v in vs], "nnz": [sum(1 for x in v if x > 0) for v in vs],
            "L1": pair(lambda a, b: sum(abs(x - y) for x, y in zip(a, b))),
            "Linf": pair(lambda a, b: max(abs(x - y) for x, y in zip(a, b))),
            "ne": pair(lambda a, b: sum(1 for x, y in zip(a, b) if x != y)),
            "both": pair(lambda a, b: sum(1 for x, y in zip(a, b) if x > 0 and y > 0))}


def table(metric, a, b):
    """the issue's table, evaluated in fractions on two small vectors -> Fraction, or None where the denominator is zero"""
    a, b = [int(x) for x in a], [int(x) for x in b]
    N = len(a)
    l1, linf = sum(abs(x - y) for x, y in zip(a, b)), max(abs(x - y) for x, y in zip(a, b))
    ne = sum(1 for x, y in zip(a, b) if x != y)
    ctt = sum(1 for x, y in zip(a, b) if x > 0 and y > 0)
    ctf = sum(1 for x, y in zip(a, b) if x > 0 and not y > 0)
    cft = sum(1 for x, y in zip(a, b) if not x > 0 and y > 0)
    cff = N - ctt - ctf - cft
    num, den = {
        "cityblock": (l1, 1), "chebyshev": (linf, 1), "braycurtis": (l1, sum(a) + sum(b)), "hamming": (ne, N), "matching": (ne, N),
        "jaccard": (ctf + cft, ctt + ctf + cft), "dice": (ctf + cft, 2 * ctt + ctf + cft),
        "rogerstanimoto": (2 * (ctf + cft), ctt + cff + 2 * (ctf + cft)), "sokalmichener": (2 * (ctf + cft), ctt + cff + 2 * (ctf + cft)),
        "russellrao": (N - ctt, N), "sokalsneath": (2 * (ctf + cft), ctt + 2 * (ctf + cft)),
        "yule": (2 * ctf * cft, ctt * cff + ctf * cft), "kulsinski": (ctf + cft - ctt + N, ctf + cft + N)}[metric]
    return None if den == 0 else Fraction(num, den)


A = [3, 0, 2, 0, 0, 1, 2 ** 40, 0]
VECTORS = [A,
           [0, 0, 0, 0, 0, 0, 0, 2 ** 64 - 1],           # 2^64 - 1 beside a 0 of every other vector but the next
           [1, 0, 9, 0, 0, 0, 2 ** 40, 5],
           [0, 5, 0, 0, 7, 0, 0, 0],                     # disjoint from A
           [2, 1, 1, 4, 1, 3, 2 ** 40 - 1, 0]]


def close_to_nearest(v, exact):
    want = float(exact)
    return abs(v - want) <= np.spacing(want)


@pytest.mark.parametrize("metric", INTEGER_METRICS)
def test_from_pairstats_gives_the_nearest_float64_of_the_table(metric):
    from kmerdb_amd import distance
    m = distance.from_pairstats(host_stats(VECTORS), len(A), metric)
    assert m.shape == (5, 5) and m.dtype == np.float64
    for i in range(5):
        assert m[i][i] == 0.0
        for j in range(5):
            if i != j:
                exact = table(metric, VECTORS[i], VECTORS[j])
                assert exact is not None and close_to_nearest(m[i][j], exact), (metric, i, j, m[i][j], exact)
                assert m[i][j] == m[j][i]
    if metric == "cityblock":
        assert m[0][1] == float(2 ** 64 - 1 + 2 ** 40 + 6) and m[0][1] > 2.0 ** 64
    if metric == "chebyshev":
        assert m[0][1] == float(2 ** 64 - 1) and m[0][2] == 7.0


SMALL = np.array([[3, 0, 2, 0, 0, 1, 0, 4, 1, 0, 0, 6],
                  [0, 5, 0, 0, 7, 0, 0, 4, 2, 0, 1, 6],
                  [1, 0, 9, 0, 0, 0, 2, 0, 1, 0, 0, 6],
                  [3, 0, 2, 0, 0, 1, 0, 4, 1, 0, 0, 7]], dtype=np.uint64)


def test_what_the_names_mean_scipy():
    ssd = pytest.importorskip("scipy.spatial.distance")
    from kmerdb_amd import distance
    stats = host_stats(SMALL)
    have = 0
    for metric in INTEGER_METRICS:
        ours = distance.from_pairstats(stats, SMALL.shape[1], metric)
        if metric == "kulsinski":                        # scipy <= 1.11's documented formula; later versions dropped the name
            want = np.zeros((4, 4))
            for i in range(4):
                for j in range(4):
                    if i != j:
                        x, y = SMALL[i] > 0, SMALL[j] > 0
                        ctt, r = int((x & y).sum()), int((x ^ y).sum())
                        want[i][j] = (r - ctt + SMALL.shape[1]) / (r + SMALL.shape[1])
        else:
            data = (SMALL > 0) if metric == "dice" else SMALL.astype(np.float64)          # (dice: of the presence vectors, on purpose)
            try:
                want = ssd.squareform(ssd.pdist(data, metric))
            except ValueError:                           # (a name this scipy no longer has)
                continue
        have += 1
        assert np.allclose(ours, want, rtol=1e-9, atol=0.0), (metric, ours, want)
    assert have >= 12
    # minkowski is scipy's default p = 2: euclidean, on the moment path
    assert distance.ALIAS_METRICS == {"minkowski": "euclidean"}
    o = [v.astype(object) for v in SMALL]
    eu = distance.from_moments([int(a.sum()) for a in o], [[int(np.dot(a, b)) for b in o] for a in o], SMALL.shape[1], "euclidean")
    assert np.allclose(eu, ssd.squareform(ssd.pdist(SMALL.astype(np.float64), "minkowski")), rtol=1e-9, atol=0.0)


def test_degenerate_cases():
    from kmerdb_amd import distance
    N = 6
    zero, a, b = [0] * N, [3, 0, 2, 0, 0, 1], [0, 5, 0, 0, 7, 0]            # b's support is disjoint from a's
    full = [1] * N
    vs = [zero, zero, a, a, b, full, full]
    stats = host_stats(vs)
    nan = float("nan")
    # (zero, zero), (a, a): identical; (a, b): disjoint; (zero, a): one empty; (full, full): identical with no absent bin
    want = {                 # zero-zero, a-a, a-b, zero-a, full-full
        "cityblock": (0.0, 0.0, 18.0, 6.0, 0.0),
        "chebyshev": (0.0, 0.0, 7.0, 3.0, 0.0),
        "braycurtis": (nan, 0.0, 1.0, 1.0, 0.0),                            # 0 / 0: nan, as scipy
        "hamming": (0.0, 0.0, 5 / 6, 0.5, 0.0),
        "matching": (0.0, 0.0, 5 / 6, 0.5, 0.0),
        "jaccard": (0.0, 0.0, 1.0, 1.0, 0.0),                               # two empty sets: 0.0, pinned to scipy 1.15.3
        "dice": (nan, 0.0, 1.0, 1.0, 0.0),
        "rogerstanimoto": (0.0, 0.0, 10 / 11, 2 / 3, 0.0),
        "sokalmichener": (0.0, 0.0, 10 / 11, 2 / 3, 0.0),
        "russellrao": (1.0, 0.5, 1.0, 1.0, 0.0),                            # not 0 for identical vectors: (N - ctt) / N, as scipy
        "sokalsneath": (nan, 0.0, 1.0, 1.0, 0.0),
        "yule": (0.0, 0.0, 2.0, 0.0, 0.0),                                  # ctf cft == 0: 0.0 whatever the denominator, pinned to scipy 1.15.3
        "kulsinski": (1.0, 0.5, 11 / 11, 9 / 9, 0.0),
    }
    assert set(want) == set(INTEGER_METRICS)
    for metric, (zz, aa, ab, za, ff) in want.items():
        m = distance.from_pairstats(stats, N, metric)
        for got, w in ((m[0][1], zz), (m[2][3], aa), (m[2][4], ab), (m[0][2], za), (m[5][6], ff)):
            assert (math.isnan(got) and math.isnan(w)) or got == pytest.approx(w, rel=1e-15, abs=0.0), (metric, m)
        assert all(m[i][i] == 0.0 for i in range(len(vs)))
    # the float metrics' last step: canberra is C, jensenshannon sqrt(D / 2); nan (an all-zero vector) stays nan
    c = np.array([[0.0, 3.0], [3.0, 0.0]])
    d = np.array([[0.0, nan], [nan, 0.0]])
    assert distance.from_pairfloat(c, d, "canberra").tolist() == [[0.0, 3.0], [3.0, 0.0]]
    js = distance.from_pairfloat(c, d, "jensenshannon")
    assert js[0][0] == js[1][1] == 0.0 and math.isnan(js[0][1]) and math.isnan(js[1][0])
    assert distance.from_pairfloat(c, np.array([[0.0, 0.5], [0.5, 0.0]]), "jensenshannon")[0][1] == 0.5
    with pytest.raises(ValueError):
        distance.from_pairfloat(c, d, "cityblock")


def test_degenerate_cases_follow_scipy_where_it_returns_a_number():
    ssd = pytest.importorskip("scipy.spatial.distance")
    from kmerdb_amd import distance
    N = 6
    vs = [[0] * N, [0] * N, [3, 0, 2, 0, 0, 1], [3, 0, 2, 0, 0, 1], [0, 5, 0, 0, 7, 0], [1] * N, [1] * N]
    stats = host_stats(vs)
    data = np.array(vs, dtype=np.float64)
    for metric in ("cityblock", "chebyshev", "braycurtis", "hamming", "jaccard", "rogerstanimoto", "sokalmichener", "russellrao", "sokalsneath", "yule"):
        with np.errstate(all="ignore"):
            want = ssd.squareform(ssd.pdist(data, metric))
        ours = distance.from_pairstats(stats, N, metric)
        for i in range(len(vs)):
            for j in range(len(vs)):
                if i != j:
                    assert (math.isnan(ours[i][j]) and math.isnan(want[i][j])) or ours[i][j] == pytest.approx(want[i][j], rel=1e-12), (metric, i, j)


def test_metric_tables_and_the_parser():
    from kmerdb_amd import distance, profile
    new = distance.SWEEP_METRICS + distance.FLOAT_METRICS + tuple(distance.ALIAS_METRICS)
    assert set(distance.SWEEP_METRICS) == set(INTEGER_METRICS) and distance.FLOAT_METRICS == ("canberra", "jensenshannon")
    assert not set(new) & set(distance.METRICS + distance.RANK_METRICS) and len(set(new)) == len(new)
    assert set(distance.SWEEP_IDENTITY) == set(distance.SWEEP_METRICS + distance.FLOAT_METRICS)
    assert set(distance.ALL_METRICS) == set(new) | set(distance.METRICS) | set(distance.RANK_METRICS)
    for metric in distance.ALL_METRICS:
        distance._check_metric(metric)
    for bad in ("EMD", "kendall", "seuclidean", "mahalanobis"):
        with pytest.raises(ValueError) as e:
            distance._check_metric(bad)
        for name in distance.ALL_METRICS:
            assert name in str(e.value)
    # from_moments keeps to the moment metrics, from_pairstats to its own
    with pytest.raises(ValueError):
        distance.from_moments([1, 2], [[1, 0], [0, 4]], 4, "braycurtis")
    with pytest.raises(ValueError):
        distance.from_pairstats(host_stats([[1, 2], [3, 4]]), 2, "canberra")
    with pytest.raises(ValueError):
        distance.from_pairstats(host_stats([[1, 2], [3, 4]]), 2, "euclidean")


def test_the_distance_command_takes_every_name(monkeypatch):
    from kmerdb_amd import distance, profile
    seen = []
    monkeypatch.setattr(distance, "distances", lambda inputs, metric, **kw: seen.append((list(inputs), metric, kw)))
    assert profile.main(["distance", "braycurtis", "a.kdb", "b.kdb"]) == 0
    assert seen[0][:2] == (["a.kdb", "b.kdb"], "braycurtis") and seen[0][2]["device"] == 0
    for metric in distance.ALL_METRICS:
        assert profile.main(["distance", metric, "a.kdb", "b.kdb", "c.kdb"]) == 0
        assert seen[-1][:2] == (["a.kdb", "b.kdb", "c.kdb"], metric)
    for bad in ("EMD", "seuclidean"):
        with pytest.raises(SystemExit):
            profile.main(["distance", bad, "a.kdb", "b.kdb"])


@pytest.fixture(scope="module")
def isa(tmp_path_factory):
    import isa_stats
    d = tmp_path_factory.mktemp("isa_pairstats")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared", "-I", os.path.join(ROOT, "include"), "-save-temps",
           "-o", str(d / "lib.so"), os.path.join(ROOT, "kmerdb_amd", "csrc", "kdb_engine.hip"), "-lz", "-lpthread"]
    subprocess.check_call(cmd, cwd=str(d), stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    s = [f for f in os.listdir(d) if f.endswith("gfx950.s")]
    assert len(s) == 1
    return isa_stats.kernel_stats(str(d / s[0]))


def test_every_sweep_keeps_four_waves_per_simd_and_does_not_spill(isa):
    hits = {n: v for n, v in isa.items() if "kdbpair::pair_kernel<" in n}
    # the diagonal blocks of 1..4 vectors, and a full block against 1 or 2 vectors of a later block
    want = ["pair_kernel<%d, %d, true>" % (a, a) for a in (1, 2, 3, 4)] + ["pair_kernel<4, %d, false>" % b for b in (1, 2)]
    for w in want:
        assert sum(1 for n in hits if w in n) == 1, (w, sorted(hits))
    assert len(hits) == len(want), sorted(hits)
    flt = {n: v for n, v in isa.items() if "kdbpair::pairfloat_kernel" in n}
    assert len(flt) == 1, sorted(flt)
    for n, v in list(hits.items()) + list(flt.items()):
        assert v["scratch"] == 0 and v["vgprs"] <= 128, (n, v)
    for name in ("kdbpair::pair_tail_kernel", "kdbpair::pair_combine_kernel", "kdbpair::pairfloat_tail_kernel", "kdbpair::pairfloat_combine_kernel"):
        v = [s for n, s in isa.items() if name in n]
        assert len(v) == 1 and v[0]["scratch"] == 0, (name, v)
