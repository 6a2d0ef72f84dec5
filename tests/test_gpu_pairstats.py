"""GPU: kdb_pairstats -- the exact integers of the distances that are not moments -- against Python integers; kdb_pairfloat -- canberra and
Jensen-Shannon in float64 -- against exact rationals and 60-digit decimals within derived bounds; and the layers above them
(distance.pairstats / distance_matrix / profile_distances / the .kdb driver)."""
import collections
import ctypes
import decimal
import io
import os
import re
from fractions import Fraction

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INPUTS = os.path.join(ROOT, "tests", "golden", "inputs")
KEYS = ("S", "nnz", "L1", "Linf", "ne", "both")
TOP = 2 ** 64 - 1


def _header_constant(name):
    text = open(os.path.join(ROOT, "include", "kdbhip.h")).read()
    return int(re.search(r"#define\s+%s\s+(\d+)" % name, text).group(1))


GRAM_MAX = _header_constant("KDB_GRAM_MAX")
B = _header_constant("KDB_PAIRSTATS_BLOCK")
WG_BINS = _header_constant("KDB_PAIRSTATS_WG_BINS")


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
        def stats(tensors):
            torch.cuda.synchronize(0)
            return distance.pairstats_raw([t.data_ptr() for t in tensors], tensors[0].numel())[0]

        @staticmethod
        def floats(tensors):
            torch.cuda.synchronize(0)
            return distance.pairfloat_raw([t.data_ptr() for t in tensors], tensors[0].numel())[:2]

        @classmethod
        def raw(cls, ptrs, n, nbins, call="kdb_pairstats"):
            """the C call with arguments as given -> status"""
            m = max(n, 1)
            arr = (ctypes.c_void_p * max(len(ptrs), 1))(*[ctypes.c_void_p(p) for p in ptrs])
            torch.cuda.synchronize(0)
            if call == "kdb_pairfloat":
                c, d = (ctypes.c_double * (m * m))(), (ctypes.c_double * (m * m))()
                return cls.lib.kdb_pairfloat(0, arr, n, nbins, c, d, None)
            u = lambda k: (ctypes.c_uint64 * k)()
            return cls.lib.kdb_pairstats(0, arr, n, nbins, u(2 * m), u(m), u(2 * m * m), u(m * m), u(m * m), u(m * m), None)
    return Dev


def _expected(vs):
    """kdb_pairstats' integers on the host: Python ints (int64 differences where every value is small, object arrays otherwise)"""
    n = len(vs)
    small = all(int(v.max()) < 2 ** 62 for v in vs)
    w = [v.astype(np.int64) if small else v.astype(object) for v in vs]
    out = {"S": [int(v.astype(object).sum()) for v in vs], "nnz": [int(np.count_nonzero(v)) for v in vs]}
    for key in KEYS[2:]:
        out[key] = [[0] * n for _ in range(n)]
    for i in range(n):
        out["both"][i][i] = out["nnz"][i]
        for j in range(i + 1, n):
            d = np.abs(w[i] - w[j])
            vals = {"L1": int(d.astype(object).sum()), "Linf": int(d.max()), "ne": int(np.count_nonzero(vs[i] != vs[j])),
                    "both": int(np.count_nonzero((vs[i] > 0) & (vs[j] > 0)))}
            for key, v in vals.items():
                out[key][i][j] = out[key][j][i] = v
    return out


def _counts(rng, nbins):
    return (rng.poisson(3.0, nbins) * rng.integers(0, 2, nbins)).astype(np.uint64)


@pytest.mark.parametrize("nbins", [1, 2, 3, 63, 64, 65, 4 ** 5, WG_BINS - 1, WG_BINS, WG_BINS + 1, 4 ** 10 + 1])
def test_lengths_at_lane_wave_workgroup_and_grid_edges(dev, nbins):
    rng = np.random.default_rng(nbins)
    vs = [_counts(rng, nbins) for _ in range(3)]
    vs[0][-1] = vs[1][-1] = np.uint64(0)
    vs[2][-1] = np.uint64(7)                              # (the last bin counts, in one vector only)
    assert dev.stats([dev.upload(v) for v in vs]) == _expected(vs)


@pytest.mark.parametrize("n", [1, 2, B, B + 1, 2 * B + 1, GRAM_MAX])
def test_vector_counts_at_block_edges_fill_both_triangles(dev, n):
    nbins = 4 ** 6
    rng = np.random.default_rng(100 + n)
    vs = [_counts(rng, nbins) for _ in range(n)]
    got = dev.stats([dev.upload(v) for v in vs])
    assert got == _expected(vs)
    for key in KEYS[2:]:
        assert all(got[key][i][j] == got[key][j][i] for i in range(n) for j in range(n))
    if n > 1:
        assert all(got["L1"][i][j] > 0 for i in range(n) for j in range(n) if i != j)


def test_the_same_pointer_twice(dev):
    rng = np.random.default_rng(5)
    a, b = dev.upload(_counts(rng, 4 ** 6)), dev.upload(_counts(rng, 4 ** 6))
    for order in ([a, a], [a, b, a], [b, a, b, b, a, a]):
        st = dev.stats(order)
        for i, x in enumerate(order):
            for j, y in enumerate(order):
                if x is y:
                    assert st["L1"][i][j] == st["Linf"][i][j] == st["ne"][i][j] == 0
                    assert st["both"][i][j] == st["nnz"][i] == st["nnz"][j] > 0
                else:
                    assert st["L1"][i][j] > 0 and st["ne"][i][j] > 0


@pytest.mark.parametrize("where", ["x in the body, y in the tail", "x in the tail, y in the body"])
def test_difference_signs_and_the_high_word_of_l1(dev, where):
    nbins = 2 * WG_BINS + 77                              # two workgroups' whole chunks and a tail of 77 bins
    body, tail = WG_BINS + 130 + 17, nbins - 3
    bx, by = (body, tail) if where.startswith("x in the body") else (tail, body)
    b = np.arange(nbins)
    # a lane holds two consecutive bins: even lanes x > y, odd lanes x < y, in every wave
    up = np.where((b // 2) % 2 == 0, 2 ** 40 + b, b % 5).astype(np.uint64)
    down = np.where((b // 2) % 2 == 0, b % 7, 2 ** 33 + 3 * b).astype(np.uint64)
    # disjoint supports, each sum 2^64 - 1: L1 = 2^65 - 2 needs its high word; Linf = 2^64 - 1
    x, y = np.zeros(nbins, dtype=np.uint64), np.zeros(nbins, dtype=np.uint64)
    x[bx], y[by] = np.uint64(TOP), np.uint64(TOP)
    vs = [up, x, down, y]                                 # x before `down` and y after it: the extreme value on either side of the difference
    got = dev.stats([dev.upload(v) for v in vs])
    assert got == _expected(vs)
    assert got["L1"][1][3] == 2 ** 65 - 2 and got["Linf"][1][3] == TOP and got["ne"][1][3] == 2 and got["both"][1][3] == 0
    assert got["Linf"][1][2] == TOP - int(down[bx]) and got["Linf"][2][3] == TOP - int(down[by]) and got["Linf"][0][1] == TOP - int(up[bx])
    assert got["L1"][0][2] == sum(abs(int(p) - int(q)) for p, q in zip(up, down))
    # one bin with x = 2^64 - 1 against 0, and the mirrored bin elsewhere, among lanes of either sign
    p, q = np.zeros(nbins, dtype=np.uint64), ((b + 1) % 3).astype(np.uint64)     # p <= q everywhere but at bx, where p - q = 2^64 - 1
    p[bx], q[bx] = np.uint64(TOP), np.uint64(0)
    got = dev.stats([dev.upload(p), dev.upload(q), dev.upload(p)])
    assert got == _expected([p, q, p])
    assert got["Linf"][0][1] == got["Linf"][1][2] == TOP and got["L1"][0][1] == TOP + int(q.astype(object).sum())


def test_a_sum_of_two_to_the_64_is_refused_and_the_argument_ladder(dev):
    from kmerdb_amd import _abi
    v = np.zeros(4 ** 6, dtype=np.uint64)
    v[10] = v[4000] = np.uint64(2 ** 63)
    ones = np.ones(4 ** 6, dtype=np.uint64)
    t, ok = dev.upload(v), dev.upload(ones)
    for call in ("kdb_pairstats", "kdb_pairfloat"):
        assert dev.raw([ok.data_ptr(), t.data_ptr()], 2, 4 ** 6, call) == _abi.KDB_ERR_ARG
    assert "2^64" in _abi.last_error()
    v[4000] = np.uint64(2 ** 63 - 1)                      # 2^64 - 1 is fine
    t = dev.upload(v)
    assert dev.stats([ok, t]) == _expected([ones, v])
    small = dev.upload(np.arange(4 ** 4, dtype=np.uint64))
    p = small.data_ptr()
    for call in ("kdb_pairstats", "kdb_pairfloat"):
        assert dev.raw([p], 1, 4 ** 4, call) == _abi.KDB_OK
        assert dev.raw([p], 0, 4 ** 4, call) == _abi.KDB_ERR_ARG
        assert dev.raw([p] * (GRAM_MAX + 1), GRAM_MAX + 1, 4 ** 4, call) == _abi.KDB_ERR_ARG
        assert dev.raw([p, p + 8], 2, 4 ** 4 - 1, call) == _abi.KDB_ERR_ARG          # a pointer off by 8 bytes
        assert dev.raw([p], 1, 0, call) == _abi.KDB_ERR_ARG
        assert dev.raw([p], 1, 2 ** 36 + 1, call) == _abi.KDB_ERR_ARG
        assert dev.raw([p, 0], 2, 4 ** 4, call) == _abi.KDB_ERR_ARG                  # NULL


def test_an_engines_table_in_place_and_profile_distances(dev, gpu_engine_cls):
    from kmerdb_amd import distance, parse, reader
    k = 7
    engines = [gpu_engine_cls(k), gpu_engine_cls(k)]
    try:
        for eng, f in zip(engines, ("reads150.fq", "ragged_n.fq")):
            for bases, offsets, _ in reader.iter_blocks(os.path.join(INPUTS, f)):
                eng.submit(bases, offsets)
        before = [e.get_option("d2h_bytes") for e in engines]
        got = {m: distance.distance_matrix(engines, m) for m in ("braycurtis", "jaccard")}
        st = distance.pairstats(engines)
        assert [e.get_option("d2h_bytes") for e in engines] == before
        vs = [e.finish()[0] for e in engines]
        assert int(vs[0].sum()) > 0 and int(vs[1].sum()) > 0
        want = _expected(vs)
        assert st == want
        for m in got:
            assert got[m].tobytes() == distance.from_pairstats(want, 4 ** k, m).tobytes()
            assert 0.0 < got[m][0][1] < 1.0
        with pytest.raises(ValueError):
            distance.pairstats([engines[0], vs[1][:-4]])
    finally:
        for e in engines:
            e.close()
    files = [os.path.join(INPUTS, f) for f in ("reads150.fq", "contigs.fa")]
    vs = [parse.parsefile(f, 8, replace_with_none=True, canonicalize=True)[0] for f in files]
    m, cols, md = distance.profile_distances(files, 8, metric="cityblock", no_ambiguous=True)
    assert m.tobytes() == distance.from_pairstats(_expected(vs), 4 ** 8, "cityblock").tobytes() and m[0][1] > 0
    assert cols == ["reads150", "contigs"] and [d["total_kmers"] for d in md] == [int(v.sum()) for v in vs]


# ---- the float sweep ----

def _float_vectors(nbins, seed):
    """seeded counts, half the bins zero, one count of 2^40 in the first; the third vector is the second with a few bins changed (a small D)"""
    rng = np.random.default_rng(seed)
    a = ((rng.poisson(3.0, nbins) + 1) * rng.integers(0, 2, nbins)).astype(np.uint64)
    b = ((rng.poisson(5.0, nbins) + 1) * rng.integers(0, 2, nbins)).astype(np.uint64)
    a[nbins // 3] = np.uint64(2 ** 40)
    c = b.copy()
    c[::17] += np.uint64(1)
    return [a, b, c]


def _exact_canberra(x, y):
    groups = collections.Counter(zip(x.tolist(), y.tolist()))
    return sum((m * Fraction(abs(p - q), p + q) for (p, q), m in groups.items() if p + q > 0), Fraction(0))


_CTX = decimal.Context(prec=60)


def _decimal_js(x, y):
    """D = Sum p ln(p/m) + q ln(q/m) to 60 digits"""
    sx, sy = decimal.Decimal(int(x.astype(object).sum())), decimal.Decimal(int(y.astype(object).sum()))
    total = decimal.Decimal(0)
    for (a, b), mult in collections.Counter(zip(x.tolist(), y.tolist())).items():
        p, q = _CTX.divide(decimal.Decimal(a), sx), _CTX.divide(decimal.Decimal(b), sy)
        m = _CTX.divide(_CTX.add(p, q), decimal.Decimal(2))
        t = decimal.Decimal(0)
        if a:
            t = _CTX.add(t, _CTX.multiply(p, _CTX.ln(_CTX.divide(p, m))))
        if b:
            t = _CTX.add(t, _CTX.multiply(q, _CTX.ln(_CTX.divide(q, m))))
        total = _CTX.add(total, _CTX.multiply(t, decimal.Decimal(mult)))
    return total


@pytest.fixture(scope="module", params=[4 ** 6, WG_BINS + 1])
def float_case(request, dev):
    nbins = request.param
    vs = _float_vectors(nbins, nbins)
    c, d = dev.floats([dev.upload(v) for v in vs])
    return nbins, vs, c, d


def test_canberra_within_the_bound_of_its_roundings(float_case):
    """|C - exact| <= (nbins + 4) 2^-53 exact: one rounding per conversion and quotient, nbins adds of non-negative terms in any order."""
    nbins, vs, c, _ = float_case
    for i in range(3):
        assert c[i][i] == 0.0
        for j in range(i + 1, 3):
            exact = _exact_canberra(vs[i], vs[j])
            err = abs(Fraction(float(c[i][j])) - exact)
            print("canberra nbins=%d pair=(%d, %d): C=%r, error %.3g of the bound" % (nbins, i, j, c[i][j], float(err / ((nbins + 4) * Fraction(1, 2 ** 53) * exact))))
            assert exact > 0 and err <= (nbins + 4) * Fraction(1, 2 ** 53) * exact
            assert c[i][j] == c[j][i]


def test_jensen_shannon_sum_within_the_bound_of_its_roundings(float_case):
    """|D - ref| <= (16 + nbins D) 2^-53, ref a 60-digit decimal evaluation: nbins D is the summation bound for non-negative terms, 16 the
    roundings of quotient, log and product inside terms whose halves sum to at most 2 ln 2.  D itself is tested, not its root."""
    nbins, vs, _, d = float_case
    for i in range(3):
        assert d[i][i] == 0.0
        for j in range(i + 1, 3):
            ref = _decimal_js(vs[i], vs[j])
            err = abs(decimal.Decimal(float(d[i][j])) - ref)
            bound = (16 + nbins * ref) * decimal.Decimal(2) ** -53
            print("jensenshannon nbins=%d pair=(%d, %d): D=%r, error %.3g of the bound" % (nbins, i, j, d[i][j], float(err / bound)))
            assert ref > 0 and err <= bound
            assert d[i][j] == d[j][i]
    assert d[1][2] < 0.1 * d[0][1]                        # (the near-identical pair)


def test_float_sweep_is_repeatable_and_empty_waves_add_nothing(dev):
    nbins = 4 ** 6 + 5
    vs = _float_vectors(nbins, 77)
    for v in vs:
        v[WG_BINS:2 * WG_BINS] = 0                        # four waves of bins empty in every vector ...
    vs[1][128:256] = 0                                    # ... and one empty in one vector only
    ts = [dev.upload(v) for v in vs]
    c1, d1 = dev.floats(ts)
    c2, d2 = dev.floats(ts)
    assert c1.tobytes() == c2.tobytes() and d1.tobytes() == d2.tobytes()
    for i in range(3):
        for j in range(i + 1, 3):
            exact = _exact_canberra(vs[i], vs[j])
            assert abs(Fraction(float(c1[i][j])) - exact) <= (nbins + 4) * Fraction(1, 2 ** 53) * exact
            ref = _decimal_js(vs[i], vs[j])
            assert abs(decimal.Decimal(float(d1[i][j])) - ref) <= (16 + nbins * ref) * decimal.Decimal(2) ** -53
    # an all-zero vector: every bin of the other is a canberra term of 1; D is nan
    zero = np.zeros(nbins, dtype=np.uint64)
    c, d = dev.floats([ts[0], dev.upload(zero)])
    assert c[0][1] == c[1][0] == float(np.count_nonzero(vs[0])) and np.isnan(d[0][1]) and np.isnan(d[1][0]) and d[0][0] == d[1][1] == 0.0


def test_the_kdb_driver_prints_the_float_and_integer_metrics(dev, tmp_path):
    from kmerdb_amd import distance, fileutil
    k = 4
    rng = np.random.default_rng(21)
    vs, paths = [], []
    for name in ("a", "b", "c"):
        v = _counts(rng, 4 ** k) + np.uint64(name == "c")
        md = {"version": fileutil.VERSION, "metadata_blocks": 1, "k": k, "total_kmers": int(v.sum()), "unique_kmers": int(np.count_nonzero(v)),
              "unique_nullomers": 0, "sorted": False, "tags": [], "files": []}
        p = str(tmp_path / (name + ".%d.kdb" % k))
        fileutil.write_kdb(p, md, v)
        vs.append(v)
        paths.append(p)

    def host_js(x, y):
        p, q = x / x.sum(), y / y.sum()
        m = (p + q) / 2
        with np.errstate(divide="ignore", invalid="ignore"):
            t = np.where(p > 0, p * np.log(p / m), 0.0) + np.where(q > 0, q * np.log(q / m), 0.0)
        return float(np.sqrt(t.sum() / 2))

    out = io.StringIO()
    m = distance.distances(paths, "jensenshannon", out=out)
    lines = out.getvalue().splitlines()
    assert lines[0].split("\t") == ["a", "b", "c"] and len(lines) == 4
    printed = np.array([[float(x) for x in line.split("\t")] for line in lines[1:]])
    f = [v.astype(np.float64) for v in vs]
    for i in range(3):
        for j in range(3):
            want = 0.0 if i == j else host_js(f[i], f[j])
            assert printed[i][j] == pytest.approx(want, rel=1e-9) and printed[i][j] == m[i][j]
    out = io.StringIO()
    distance.distances(paths[:2], "jensenshannon", out=out)
    assert out.getvalue().count("\n") == 1 and float(out.getvalue()) == pytest.approx(host_js(f[0], f[1]), rel=1e-9)
    out = io.StringIO()
    distance.distances(paths[:2], "braycurtis", out=out)
    want = np.abs(f[0] - f[1]).sum() / (f[0].sum() + f[1].sum())
    assert float(out.getvalue()) == pytest.approx(want, rel=1e-12)
    out = io.StringIO()
    distance.distances(paths[:2], "minkowski", out=out)
    assert float(out.getvalue()) == pytest.approx(float(np.sqrt(((f[0] - f[1]) ** 2).sum())), rel=1e-12)
