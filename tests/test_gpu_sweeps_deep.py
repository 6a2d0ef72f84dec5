"""GPU: the analysis sweeps -- kdb_gram, kdb_pairstats, kdb_pairfloat, kdb_size_factors, kdb_scale_counts -- past one grid stride, per
block role and per carry: the cases of tests/sweep_cases.py (tests/test_sweep_cases_cpu.py proves each is where it claims to be) against
exact Python integers, exact rationals, 60-digit decimals and numpy's IEEE arithmetic.  The float bounds are the ones the tests written
beside the kernels derive, with these cases' nbins."""
import ctypes
import decimal
import math
import os
import sys
from fractions import Fraction

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sweep_cases as sc  # noqa: E402

pytestmark = pytest.mark.gpu

TOP = sc.TOP
U = 2.0 ** -53


@pytest.fixture(scope="module")
def dev(gpu_engine_cls):
    import torch
    from kmerdb_amd import _abi, distance, matrix

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
        def gram(tensors):
            torch.cuda.synchronize(0)
            return distance.gram([t.data_ptr() for t in tensors], tensors[0].numel())[:2]

        @staticmethod
        def stats(tensors):
            torch.cuda.synchronize(0)
            return distance.pairstats_raw([t.data_ptr() for t in tensors], tensors[0].numel())[0]

        @staticmethod
        def floats(tensors):
            torch.cuda.synchronize(0)
            return distance.pairfloat_raw([t.data_ptr() for t in tensors], tensors[0].numel())[:2]

        @staticmethod
        def log_sf(tensors):
            torch.cuda.synchronize(0)
            return matrix.size_factors_raw([t.data_ptr() for t in tensors], tensors[0].numel())[:2]

        @classmethod
        def raw(cls, call, tensors):
            """the C call -> status"""
            n, nbins = len(tensors), tensors[0].numel()
            arr = (ctypes.c_void_p * n)(*[ctypes.c_void_p(t.data_ptr()) for t in tensors])
            u = lambda k: (ctypes.c_uint64 * k)()
            torch.cuda.synchronize(0)
            if call == "kdb_gram":
                return cls.lib.kdb_gram(0, arr, n, nbins, u(2 * n), u(2 * n * n), None)
            if call == "kdb_pairfloat":
                return cls.lib.kdb_pairfloat(0, arr, n, nbins, (ctypes.c_double * (n * n))(), (ctypes.c_double * (n * n))(), None)
            return cls.lib.kdb_pairstats(0, arr, n, nbins, u(2 * n), u(n), u(2 * n * n), u(n * n), u(n * n), u(n * n), None)

        @classmethod
        def scale(cls, src, s, dst, as_float64=0):
            torch.cuda.synchronize(0)
            return cls.lib.kdb_scale_counts(0, ctypes.c_void_p(src.data_ptr()), src.numel(), ctypes.c_double(s), ctypes.c_void_p(dst.data_ptr()), as_float64, None)
    return Dev


def _both_triangles(m):
    n = len(m)
    return all(m[i][j] == m[j][i] for i in range(n) for j in range(n))


def _differing(got, want):
    """the (i, j) at which two square matrices differ: what a failure prints"""
    return [(i, j) for i in range(len(want)) for j in range(len(want)) if got[i][j] != want[i][j]]


# ---- a. kdb_gram: the guard between the two multiplies ----

@pytest.mark.parametrize("n", sc.GUARD_NS)
def test_gram_one_wide_value_per_wave_in_every_vector_and_half(dev, n):
    vs, placed = sc.gram_guard_case(n)
    s, G = dev.gram([dev.upload(v) for v in vs])
    want_s, want_G = sc.gram_expected(vs)
    assert s == want_s
    assert G == want_G, _differing(G, want_G)
    assert _both_triangles(G)
    assert all(G[v][v] >= sc.GUARD_VALUE ** 2 for v, _, _ in placed)


# ---- b. kdb_gram and kdb_pairstats across the stride ----

@pytest.fixture(scope="module", params=sc.STRIDE_NS)
def stride(request, dev):
    vs, classes, planted = sc.stride_case(request.param)
    return vs, classes, planted, [dev.upload(v) for v in vs]


def test_gram_across_the_stride_in_every_off_diagonal_instantiation(dev, stride):
    vs, classes, planted, ts = stride
    s, G = dev.gram(ts)
    want_s, want_G = sc.gram_expected(vs)
    assert s == want_s
    assert G == want_G, _differing(G, want_G)
    assert _both_triangles(G)
    late = classes.index("late")
    assert G[late][late] >= 2 ** 122 and s[late] < 2 ** 62                 # (its only bins are second-iteration bins)


def test_pairstats_across_the_stride_in_every_off_diagonal_instantiation(dev, stride):
    vs, classes, planted, ts = stride
    got = dev.stats(ts)
    want = sc.pair_expected(vs)
    for key in ("S", "nnz"):
        assert got[key] == want[key], key
    for key in ("L1", "Linf", "ne", "both"):
        assert got[key] == want[key], (key, _differing(got[key], want[key]))
        assert _both_triangles(got[key])


# ---- c. kdb_pairstats: the carry of L1 at every level ----

@pytest.mark.parametrize("placement", sc.PLACEMENTS)
@pytest.mark.parametrize("n", sc.LADDER_NS)
def test_pairstats_l1_carries_at_every_level_in_every_instantiation(dev, n, placement):
    vs, a, b = sc.ladder_case(n, placement)
    got = dev.stats([dev.upload(v) for v in vs])
    want = sc.pair_expected(vs)
    assert got == want, [(key, _differing(got[key], want[key])) for key in ("L1", "Linf", "ne", "both") if got[key] != want[key]]
    for i in sc.LADDER_A:
        for j in (j for j in sc.LADDER_B if j < n):
            assert got["L1"][i][j] == got["L1"][j][i] == 2 ** 65 - 2 and got["Linf"][i][j] == got["Linf"][j][i] == TOP
            assert got["ne"][i][j] == 2 and got["both"][i][j] == 0
    assert got["S"][0] == got["S"][1] == TOP


@pytest.mark.parametrize("placement", sc.REFUSALS)
def test_a_sum_of_two_to_the_64_inside_one_lane_is_refused(dev, placement):
    from kmerdb_amd import _abi
    vs, (a, b) = sc.refusal_case(placement)
    ts = [dev.upload(v) for v in vs]
    for call in ("kdb_pairstats", "kdb_pairfloat", "kdb_gram"):
        assert dev.raw(call, ts) == dev.KDB_ERR_ARG, call
        assert "2^64" in _abi.last_error()
    vs[1][b] = np.uint64(2 ** 63 - 1)                                      # 2^64 - 1 is fine
    ts[1] = dev.upload(vs[1])
    assert dev.stats(ts) == sc.pair_expected(vs)
    assert dev.gram(ts) == sc.gram_expected(vs)
    assert dev.raw("kdb_pairfloat", ts) == dev.KDB_OK


# ---- d. kdb_pairfloat ----

@pytest.fixture(scope="module", params=[sc.FLOAT_DEEP_NBINS, sc.FLOAT_MID_NBINS])
def float_case(request, dev):
    nbins = request.param
    vs, lone = sc.float_case(nbins)
    ts = [dev.upload(v) for v in vs]
    c, d = dev.floats(ts)
    c2, d2 = dev.floats(ts)
    return nbins, vs, c, d, c2, d2


def test_pairfloat_two_calls_are_bit_identical(float_case):
    _, _, c, d, c2, d2 = float_case
    assert c.tobytes() == c2.tobytes() and d.tobytes() == d2.tobytes()


def test_pairfloat_canberra_within_the_bound_of_its_roundings(float_case):
    """|C - exact| <= (nbins + 4) 2^-53 exact, as test_gpu_pairstats derives it: one rounding per conversion and quotient, nbins adds of
    non-negative terms in any order.  A lone word that the empty-wave skip dropped would cost a whole term of 1."""
    nbins, vs, c, _, _, _ = float_case
    for i in range(3):
        assert c[i][i] == 0.0
        for j in range(i + 1, 3):
            exact = sc._tp._exact_canberra(vs[i], vs[j])
            err = abs(Fraction(float(c[i][j])) - exact)
            bound = (nbins + 4) * Fraction(1, 2 ** 53) * exact
            print("canberra nbins=%d pair=(%d, %d): C=%r, error %.3g of the bound" % (nbins, i, j, c[i][j], float(err / bound)))
            assert exact > 0 and err <= bound
            assert c[i][j] == c[j][i]


def test_pairfloat_jensen_shannon_within_the_bound_of_its_roundings(float_case):
    """|D - ref| <= (16 + nbins D) 2^-53 against the 60-digit decimal, as test_gpu_pairstats derives it"""
    nbins, vs, _, d, _, _ = float_case
    for i in range(3):
        assert d[i][i] == 0.0
        for j in range(i + 1, 3):
            ref = sc._tp._decimal_js(vs[i], vs[j])
            err = abs(decimal.Decimal(float(d[i][j])) - ref)
            bound = (16 + nbins * ref) * decimal.Decimal(2) ** -53
            print("jensenshannon nbins=%d pair=(%d, %d): D=%r, error %.3g of the bound" % (nbins, i, j, d[i][j], float(err / bound)))
            assert ref > 0 and err <= bound
            assert d[i][j] == d[j][i]


# ---- e. kdb_size_factors and kdb_scale_counts ----

@pytest.mark.parametrize("mode", sc.SF_MODES)
def test_size_factors_with_the_medians_group_beyond_the_first_stride(dev, mode):
    x, y, ts, deep = sc.grouped_case_deep(mode, 2000 + sc.SF_MODES.index(mode))
    m = len(ts)
    want = (ts[(m - 1) // 2] + ts[m // 2]) / 2 * (math.log(2.0) / 2)       # the median of t, times ln 2 / 2: a neighbouring group is 0.35 away
    eps = (2 + 10) * U * math.log(128.0)
    got, eligible = dev.log_sf([dev.upload(x), dev.upload(y)])
    print("mode", mode, "m", m, "deep", deep.size, "want", want, "got", got.tolist(), "eps", eps)
    assert eligible == m
    assert abs(got[1] - want) <= eps and abs(got[0] + want) <= eps


@pytest.mark.parametrize("s", [2.0, 0.75, 1.2345678901234567])
def test_scaled_counts_beyond_the_first_stride_are_numpys_bit_for_bit(dev, s):
    import torch
    v, second = sc.scale_case_deep(9)
    nbins = v.size
    q = v.astype(np.float64) / np.float64(s)
    want = np.rint(q).astype(np.uint64)
    src = dev.upload(v)
    buf = torch.full((nbins + 2,), -1, dtype=torch.int64, device="cuda:0")             # (two words behind the output: they must stay)
    dst = buf[:nbins]
    assert dev.scale(src, s, dst) == dev.KDB_OK
    assert buf[nbins:].tolist() == [-1, -1]
    assert dev.download(dst).tobytes() == want.tobytes()
    assert dev.download(src).tobytes() == v.tobytes()
    fl = torch.full((nbins + 2,), -1, dtype=torch.int64, device="cuda:0")
    assert dev.scale(src, s, fl[:nbins], as_float64=1) == dev.KDB_OK                   # the float64 output: the quotient, not rounded
    assert fl[nbins:].tolist() == [-1, -1]
    assert dev.download(fl[:nbins]).tobytes() == q.tobytes()
    assert dev.scale(src, s, src) == dev.KDB_OK                                        # in place
    assert dev.download(src).tobytes() == want.tobytes()
    if s == 2.0:
        assert all(int(want[b]) % 2 == 0 for b, e in zip(second, sc.SCALE_EDGE) if e % 2 == 1 and e < 2 ** 53)     # halves went to the even neighbour


@pytest.mark.parametrize("where", sorted(sc.overflow_bins()))
def test_a_quotient_of_two_to_the_63_is_found_wherever_it_lies(dev, where):
    v, _ = sc.scale_case_deep(5)
    v[sc.overflow_bins()[where]] = np.uint64(TOP)
    src = dev.upload(v)
    assert dev.scale(src, 1.0, src) == dev.KDB_ERR_ARG
    assert dev.download(src).tobytes() == v.tobytes()                                  # refused before anything was written
    dst = src.clone()
    dst.fill_(-1)
    assert dev.scale(src, 2.0, dst) == dev.KDB_ERR_ARG                                 # 2^64 / 2
    assert bool((dst == -1).all())
    s = np.nextafter(np.float64(2.0), np.float64(3.0))                                 # 2^64 / s is the float64 below 2^63
    assert dev.scale(src, float(s), dst) == dev.KDB_OK
    assert dev.download(dst).tobytes() == np.rint(v.astype(np.float64) / s).astype(np.uint64).tobytes()
