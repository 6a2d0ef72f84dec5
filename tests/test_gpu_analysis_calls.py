"""GPU: what an analysis call does around its kernels (csrc/kdb_analysis_host.hip.h: the device check, the selected device, the call's own
stream, events and scratch), entry point by entry point through the C ABI: a call that succeeds, a call the library refuses after its
scratch exists, and the first call again with the same bits; a device id one past the visible ones; torch's current device as it was
after every call.  Small on purpose: 129 bins are one whole chunk and one tail bin, five vectors a full block and a short one, the
reads three short records at k = 3.  Every failing call is an argument the library refuses by design.

Expected values and bounds are those of the tests written beside the kernels (tests/sweep_cases.py imports their recipes): Python
integers for kdb_gram and kdb_pairstats, exact rationals and 60-digit decimals for kdb_pairfloat, 50-digit decimals for
kdb_size_factors, numpy's IEEE quotient for kdb_scale_counts, a count over all bins for the spectrum and the ranks, the definition
for kdb_strand_merge, tests/score_cases.py for kdb_score_reads."""
import ctypes
import decimal
import os
import sys
from fractions import Fraction

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import score_cases  # noqa: E402
import sweep_cases as swc  # noqa: E402
from test_gpu_strand_merge import rc_ids  # noqa: E402

NBINS, N, K = 129, 5, 3
DENSE = swc.header_constant("KDB_SPECTRUM_DENSE")
PIECE, LANES = swc.header_constant("KDB_SCORE_PIECE"), swc.header_constant("KDB_SCORE_LANES")
TOP = 2 ** 64 - 1
BAD_DEVICE = "device_id=%d but %d device(s) visible"
_dp, _u64p = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_uint64)


@pytest.fixture(scope="module")
def dev(gpu_engine_cls):
    import torch
    from kmerdb_amd import _abi

    class Dev:
        lib = _abi.lib()
        OK, ARG, BAD = _abi.KDB_OK, _abi.KDB_ERR_ARG, _abi.KDB_ERR_BAD_RESIDUE
        ndev = torch.cuda.device_count()

        @staticmethod
        def upload(a):
            return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64)).to("cuda:0")

        @staticmethod
        def download(t):
            return t.cpu().numpy().view(np.uint64).copy()

        @classmethod
        def call(cls, name, *args):
            """one call of the C ABI -> (status, message); the device torch works on is the same before and after"""
            before = torch.cuda.current_device()
            torch.cuda.synchronize()
            rc = getattr(cls.lib, name)(*args)
            assert torch.cuda.current_device() == before, name
            return rc, (_abi.last_error() if rc != cls.OK else "")

        @staticmethod
        def pointers(tensors):
            return (ctypes.c_void_p * len(tensors))(*[ctypes.c_void_p(t.data_ptr()) for t in tensors])
    n = ctypes.c_int(0)
    assert Dev.lib.kdb_device_count(ctypes.byref(n)) == Dev.OK and n.value == Dev.ndev >= 1
    return Dev


@pytest.fixture(scope="module")
def vectors():
    """five vectors of 129 bins: small counts, a third of the bins zero somewhere, the tail bin non-zero in all; and the same with vector 2
    replaced by one whose sum is 2^64"""
    rng = np.random.default_rng(129)
    vs = [((rng.poisson(3.0 + j, NBINS) + 1) * (rng.random(NBINS) > 0.1)).astype(np.uint64) for j in range(N)]
    for v in vs:
        v[NBINS - 1] += np.uint64(2)
    wide = np.zeros(NBINS, dtype=np.uint64)
    wide[[5, NBINS - 1]] = np.uint64(2 ** 63)            # one body bin, the tail bin
    return vs, vs[:2] + [wide] + vs[3:]


def _thrice(good, bad):
    """the call that succeeds, the call that is refused, the first again: -> the first result, after checking that the third has its bits"""
    first = good()
    bad()
    assert good() == first
    return first


# ---- kdb_gram, kdb_pairstats, kdb_pairfloat ----

def _gram(dev, tensors, device=0):
    sums, g = (ctypes.c_uint64 * (2 * N))(), (ctypes.c_uint64 * (2 * N * N))()
    ms = ctypes.c_double(-1.0)
    rc, msg = dev.call("kdb_gram", device, dev.pointers(tensors), N, NBINS, sums, g, ctypes.byref(ms))
    return rc, msg, list(sums), list(g), ms.value


def test_gram(dev, vectors):
    vs, vs_wide = vectors
    ts, ts_wide = [dev.upload(v) for v in vs], [dev.upload(v) for v in vs_wide]

    def good():
        rc, msg, sums, g, ms = _gram(dev, ts)
        assert (rc, msg) == (dev.OK, "") and ms > 0.0
        return sums, g

    def bad():
        rc, msg, sums, _, _ = _gram(dev, ts_wide)
        assert (rc, msg) == (dev.ARG, "kdb_gram: the sum of vector 2 is 2^64 or more: its products may have wrapped 128 bits")
        assert (sums[4], sums[5]) == (0, 1)
    sums, g = _thrice(good, bad)
    S, G = swc.gram_expected(vs)
    assert [sums[2 * i] | (sums[2 * i + 1] << 64) for i in range(N)] == S
    assert [[g[2 * (i * N + j)] | (g[2 * (i * N + j) + 1] << 64) for j in range(N)] for i in range(N)] == G
    assert all(np.array_equal(dev.download(t), v) for t, v in zip(ts, vs))


def _pairstats(dev, tensors, device=0):
    outs = [(ctypes.c_uint64 * m)() for m in (2 * N, N, 2 * N * N, N * N, N * N, N * N)]
    ms = ctypes.c_double(-1.0)
    rc, msg = dev.call("kdb_pairstats", device, dev.pointers(tensors), N, NBINS, *outs, ctypes.byref(ms))
    return rc, msg, [list(o) for o in outs], ms.value


def test_pairstats(dev, vectors):
    vs, vs_wide = vectors
    ts, ts_wide = [dev.upload(v) for v in vs], [dev.upload(v) for v in vs_wide]

    def good():
        rc, msg, outs, ms = _pairstats(dev, ts)
        assert (rc, msg) == (dev.OK, "") and ms > 0.0
        return outs

    def bad():
        rc, msg, outs, _ = _pairstats(dev, ts_wide)
        assert (rc, msg) == (dev.ARG, "kdb_pairstats: the sum of vector 2 is 2^64 or more: L1 of a pair with it may not fit its two words")
        assert (outs[0][4], outs[0][5]) == (0, 1)
    sums, nnz, l1, linf, ne, both = _thrice(good, bad)
    want = swc.pair_expected(vs)
    square = lambda a: [[a[i * N + j] for j in range(N)] for i in range(N)]
    assert [sums[2 * i] | (sums[2 * i + 1] << 64) for i in range(N)] == want["S"] and nnz == want["nnz"]
    assert [[l1[2 * (i * N + j)] | (l1[2 * (i * N + j) + 1] << 64) for j in range(N)] for i in range(N)] == want["L1"]
    assert (square(linf), square(ne), square(both)) == (want["Linf"], want["ne"], want["both"])


def _pairfloat(dev, tensors, device=0):
    c, d = np.full((N, N), -7.0), np.full((N, N), -7.0)
    ms = ctypes.c_double(-1.0)
    rc, msg = dev.call("kdb_pairfloat", device, dev.pointers(tensors), N, NBINS, c.ctypes.data_as(_dp), d.ctypes.data_as(_dp), ctypes.byref(ms))
    return rc, msg, c, d, ms.value


def test_pairfloat(dev, vectors):
    vs, vs_wide = vectors
    ts, ts_wide = [dev.upload(v) for v in vs], [dev.upload(v) for v in vs_wide]

    def good():
        rc, msg, c, d, ms = _pairfloat(dev, ts)
        assert (rc, msg) == (dev.OK, "") and ms > 0.0
        return c.tobytes(), d.tobytes()

    def bad():                                         # (its sums are kdb_pairstats': the refusal is that call's, and the outputs are as they were)
        rc, msg, c, d, ms = _pairfloat(dev, ts_wide)
        assert (rc, msg) == (dev.ARG, "kdb_pairstats: the sum of vector 2 is 2^64 or more: L1 of a pair with it may not fit its two words")
        assert np.all(c == -7.0) and np.all(d == -7.0) and ms == -1.0
    cb, db = _thrice(good, bad)
    c, d = np.frombuffer(cb).reshape(N, N), np.frombuffer(db).reshape(N, N)
    u = Fraction(1, 2 ** 53)
    for i in range(N):
        assert c[i][i] == 0.0 and d[i][i] == 0.0
        for j in range(i + 1, N):
            exact = swc._tp._exact_canberra(vs[i], vs[j])
            assert exact > 0 and abs(Fraction(float(c[i][j])) - exact) <= (NBINS + 4) * u * exact                 # test_gpu_pairstats' bounds
            ref = swc._tp._decimal_js(vs[i], vs[j])
            assert ref > 0 and abs(decimal.Decimal(float(d[i][j])) - ref) <= (16 + NBINS * ref) * decimal.Decimal(2) ** -53
            assert c[i][j] == c[j][i] and d[i][j] == d[j][i]


# ---- kdb_size_factors, kdb_scale_counts ----

def _size_factors(dev, tensors, device=0):
    out, m = np.full(N, -7.0), ctypes.c_uint64(12345)
    ms = ctypes.c_double(-1.0)
    rc, msg = dev.call("kdb_size_factors", device, dev.pointers(tensors), N, NBINS, out.ctypes.data_as(_dp), ctypes.byref(m), ctypes.byref(ms))
    return rc, msg, out, m.value, ms.value


def test_size_factors(dev, vectors):
    vs, _ = vectors
    ts = [dev.upload(v) for v in vs]
    rc, msg, got, m, ms = _size_factors(dev, ts)
    assert (rc, msg) == (dev.OK, "") and ms > 0.0
    want, eligible, lmax = swc._ts._true_log_sf(vs)
    assert m == eligible > NBINS // 3
    eps = (N + 10) * 2.0 ** -53 * lmax                                     # test_gpu_sizefactors' bound
    with decimal.localcontext(swc._ts._CTX):
        assert all(float(abs(decimal.Decimal(float(g)) - w)) <= eps for g, w in zip(got, want))
    rc, msg, again, m2, _ = _size_factors(dev, ts)
    assert (rc, msg, m2) == (dev.OK, "", m) and again.tobytes() == got.tobytes()


def _scale(dev, src, s, dst, device=0):
    ms = ctypes.c_double(-1.0)
    rc, msg = dev.call("kdb_scale_counts", device, ctypes.c_void_p(src.data_ptr()), NBINS, ctypes.c_double(s), ctypes.c_void_p(dst.data_ptr()), 0, ctypes.byref(ms))
    return rc, msg, ms.value


def test_scale_counts(dev, vectors):
    v = vectors[0][0]
    over = v.copy()
    over[[0, NBINS - 1]] = np.uint64(TOP)              # at s = 1 the quotient is 2^64 rounded: it reaches 2^63
    src, src_over = dev.upload(v), dev.upload(over)
    sentinel = np.full(NBINS, 0x5A5A5A5A5A5A5A5A, dtype=np.uint64)

    def good():
        dst = dev.upload(sentinel)
        rc, msg, ms = _scale(dev, src, 1.5, dst)
        assert (rc, msg) == (dev.OK, "") and ms > 0.0
        return dev.download(dst).tobytes()

    def bad():
        dst = dev.upload(sentinel)
        rc, msg, _ = _scale(dev, src_over, 1.0, dst)
        assert (rc, msg) == (dev.ARG, "kdb_scale_counts: a count divided by the size factor 1 reaches 2^63: it has no place in an int64 matrix")
        assert np.array_equal(dev.download(dst), sentinel)                 # d_out is untouched
    got = np.frombuffer(_thrice(good, bad), dtype=np.int64)
    assert np.array_equal(got, np.rint(v.astype(np.float64) / 1.5).astype(np.int64))


# ---- kdb_spectrum, kdb_rank_transform ----

@pytest.fixture(scope="module")
def spectrum_vector(vectors):
    v = vectors[0][1].copy()
    v[[3, 64, NBINS - 1]] = [DENSE, 2 ** 40, DENSE]                        # three large values, two of them equal, one in the tail
    return v


def _spectrum(dev, t, cap, device=0):
    dense, over = np.full(DENSE, 7, dtype=np.uint64), np.full(max(cap, 1), 7, dtype=np.uint64)
    n_over, ms = ctypes.c_uint64(12345), ctypes.c_double(-1.0)
    rc, msg = dev.call("kdb_spectrum", device, ctypes.c_void_p(t.data_ptr()), NBINS, dense.ctypes.data_as(_u64p), over.ctypes.data_as(_u64p), cap,
                       ctypes.byref(n_over), ctypes.byref(ms))
    return rc, msg, dense, over, n_over.value, ms.value


def test_spectrum(dev, spectrum_vector):
    v = spectrum_vector
    t = dev.upload(v)

    def good():
        rc, msg, dense, over, n_over, ms = _spectrum(dev, t, 8)
        assert (rc, msg, n_over) == (dev.OK, "", 3) and ms > 0.0
        return dense.tobytes(), sorted(over[:3].tolist()), over[3:].tolist()

    def bad():
        rc, msg, dense, over, n_over, ms = _spectrum(dev, t, 2)
        assert (rc, msg) == (dev.ARG, "kdb_spectrum: 3 values of 65536 and above do not fit the 2 entries given")
        assert n_over == 3 and np.all(over == 7) and ms > 0.0              # the length is told, the list is not written
    dense, over, rest = _thrice(good, bad)
    small = v[v < DENSE].astype(np.int64)
    assert np.array_equal(np.frombuffer(dense, dtype=np.uint64), np.bincount(small, minlength=DENSE).astype(np.uint64))
    assert over == [DENSE, DENSE, 2 ** 40] and rest == [7] * 5


def test_rank_transform(dev, spectrum_vector):
    v = spectrum_vector
    t = dev.upload(v)
    want = np.array([2 * int(np.count_nonzero(v < x)) + int(np.count_nonzero(v == x)) + 1 for x in v], dtype=np.uint64)
    outs = []
    for _ in range(2):
        out = dev.upload(np.zeros(NBINS, dtype=np.uint64))
        ms = ctypes.c_double(-1.0)
        rc, msg = dev.call("kdb_rank_transform", 0, ctypes.c_void_p(t.data_ptr()), NBINS, ctypes.c_void_p(out.data_ptr()), ctypes.byref(ms))
        assert (rc, msg) == (dev.OK, "") and ms.value > 0.0
        outs.append(dev.download(out))
    assert np.array_equal(outs[0], want) and np.array_equal(outs[1], want)
    assert int(want.astype(object).sum()) == NBINS * (NBINS + 1) and np.array_equal(dev.download(t), v)


# ---- kdb_strand_merge ----

def test_strand_merge(dev):
    n = 4 ** K
    rng = np.random.default_rng(64)
    F, table = rng.integers(0, 1 << 40, size=n, dtype=np.uint64), rng.integers(1, 1 << 40, size=n, dtype=np.uint64)
    ids = np.arange(n, dtype=np.uint64)
    rc_of = rc_ids(ids, K)
    want = table + np.where(ids < rc_of, F + F[rc_of], np.where(ids == rc_of, F, np.uint64(0)))
    for _ in range(2):
        d_F, d_t = dev.upload(F), dev.upload(table)
        assert dev.call("kdb_strand_merge", 0, ctypes.c_void_p(d_F.data_ptr()), ctypes.c_void_p(d_t.data_ptr()), K) == (dev.OK, "")
        assert np.array_equal(dev.download(d_t), want) and not dev.download(d_F).any()


# ---- kdb_score_reads ----

RECORDS = (b"ACGTACG", b"TTN", b"GATTACAGATT")


def _score(dev, t, total, records, device=0):
    bases, offsets = score_cases.pack(list(records))
    n = len(records)
    log10_p, ints = np.full(n, -7.0), [np.full(n, 7, dtype=np.uint64) for _ in range(3)]
    ms = ctypes.c_double(-1.0)
    rc, msg = dev.call("kdb_score_reads", device, ctypes.c_void_p(t.data_ptr()), K, 0, total, 1, ctypes.c_void_p(bases.ctypes.data), bases.size,
                       ctypes.c_void_p(offsets.ctypes.data), n, 0, ctypes.c_void_p(log10_p.ctypes.data), *[ctypes.c_void_p(a.ctypes.data) for a in ints],
                       ctypes.byref(ms))
    return rc, msg, log10_p, ints, ms.value


def test_score_reads(dev):
    v, total = score_cases.forward_profile([b"ACGTTGCAACGTAGATTACA"], K)
    t = dev.upload(v)

    def good():
        rc, msg, log10_p, ints, ms = _score(dev, t, total, RECORDS)
        assert (rc, msg) == (dev.OK, "") and ms > 0.0
        return log10_p.tobytes(), [a.tolist() for a in ints]

    def bad():
        rc, msg, log10_p, ints, ms = _score(dev, t, total, (RECORDS[0], b"TTX", RECORDS[2]))
        assert (rc, msg) == (dev.BAD, "1 residue(s) outside ACGTN (reference: kmer.py:309 / :170 raises)")
        assert np.all(log10_p == -7.0) and all(np.all(a == 7) for a in ints) and ms > 0.0
    log10_p, (windows, zeros, mins) = _thrice(good, bad)
    log10_p = np.frombuffer(log10_p)
    for r, rec in enumerate(RECORDS):
        s = score_cases.score_record(rec, v, K, False, total, 1)
        assert (windows[r], zeros[r], mins[r]) == (s.windows, s.zero_windows, s.min_count), r
        if s.log10_p is None:
            assert np.isnan(log10_p[r]) and mins[r] == TOP and windows[r] == 0
        else:
            assert score_cases.error(log10_p[r], s) <= score_cases.bound(s, PIECE, LANES), r
    assert windows == [5, 0, 9]


# ---- a device that is not there ----

def test_a_device_id_past_the_visible_ones_is_refused_by_every_entry_point(dev, vectors, spectrum_vector):
    vs, _ = vectors
    ts = [dev.upload(v) for v in vs]
    past = dev.ndev
    want = (dev.ARG, BAD_DEVICE % (past, past))
    assert _gram(dev, ts, past)[:2] == want
    assert _pairstats(dev, ts, past)[:2] == want
    rc, msg, c, d, _ = _pairfloat(dev, ts, past)
    assert (rc, msg) == want and np.all(c == -7.0) and np.all(d == -7.0)
    rc, msg, out, m, _ = _size_factors(dev, ts, past)
    assert (rc, msg) == want and np.all(out == -7.0) and m == 12345
    sentinel = np.full(NBINS, 3, dtype=np.uint64)
    dst = dev.upload(sentinel)
    assert _scale(dev, ts[0], 1.5, dst, past)[:2] == want and np.array_equal(dev.download(dst), sentinel)
    t = dev.upload(spectrum_vector)
    rc, msg, dense, over, n_over, _ = _spectrum(dev, t, 8, past)
    assert (rc, msg) == want and n_over == 0 and np.all(dense == 7) and np.all(over == 7)       # (n_over_out is zeroed before any check)
    assert dev.call("kdb_rank_transform", past, ctypes.c_void_p(t.data_ptr()), NBINS, ctypes.c_void_p(dst.data_ptr()), None) == want
    assert np.array_equal(dev.download(dst), sentinel)
    fwd, table = dev.upload(np.ones(4 ** K, dtype=np.uint64)), dev.upload(np.ones(4 ** K, dtype=np.uint64))
    assert dev.call("kdb_strand_merge", past, ctypes.c_void_p(fwd.data_ptr()), ctypes.c_void_p(table.data_ptr()), K) == want
    assert dev.download(fwd).all() and np.array_equal(dev.download(table), np.ones(4 ** K, dtype=np.uint64))
    rc, msg, log10_p, ints, ms = _score(dev, dev.upload(np.ones(4 ** K, dtype=np.uint64)), 64, RECORDS, past)
    assert (rc, msg) == want and np.all(log10_p == -7.0) and ms == 0.0                         # (kernel_ms_out is zeroed first)
