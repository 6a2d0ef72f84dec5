"""GPU: what the analysis sweeps may touch.  Every device input is a payload of exactly nbins words inside 1 MiB of 0xA5 on either side
(tests/zones.py), so a read past the end meets 0xA5A5A5A5A5A5A5A5 -- about 2^63.4, which moves any sum, and twice it passes 2^64 into a
refusal -- where an exactly sized tensor would have shown the allocator's zeros; after every call every input's payload is compared with
its snapshot and both its zones with the poison.  The device outputs of kdb_scale_counts and kdb_rank_transform and the host outputs
that take a capacity lie inside zones of their own.  The expected values are the restatements the suite already has: sweep_cases,
spectrum_cases, score_cases, ids_cases, tables_cases, minimizer_cases and the oracle; the float bounds are those of
tests/test_gpu_pairstats.py and tests/test_gpu_sizefactors.py with these cases' nbins.

The bite cases at the end ask for nbins + 1 on a payload of nbins: the extra entry is the first word of the back zone, inside the
tensor.  A writer must then trip assert_zones and a reader must return something else than the restatement on nbins, or refuse.

Lengths: 1, 2 and 3 are below one lane's 16-byte load; 511 / 512 / 513 and 1023 / 1025 surround a workgroup's stride (512 bins, 1024 in
kdb_spectrum); 4097 is several workgroups and a tail.  An odd length ends the payload 8 bytes into a 16-byte line."""
import ctypes
import decimal
import math
import os
import sys
from fractions import Fraction

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ids_cases  # noqa: E402
import minimizer_cases as mc  # noqa: E402
import score_cases  # noqa: E402
import spectrum_cases as spc  # noqa: E402
import sweep_cases as sc  # noqa: E402
import tables_cases as tc  # noqa: E402
import zones  # noqa: E402

pytestmark = pytest.mark.gpu

NBINS = (1, 2, 3, 511, 512, 513, 1023, 1025, 4097)
NVECTORS = (1, 2, 5)                                   # 5 = KDB_GRAM_BLOCK + 1
TOP = 2 ** 64 - 1
U = 2.0 ** -53
DENSE = spc.DENSE
POISON_WORD = 0xA5A5A5A5A5A5A5A5
assert sc.B + 1 == 5


def mix(nbins, seed):
    """a seeded mix: a quarter of the bins zero, small counts elsewhere, one count each of 65 535, 65 536 and 2^32 - 1 where there is
    room; bin 0 and the last bin are never zero (a sweep that stops one bin early loses the last one).  Sums stay far below 2^64."""
    rng = np.random.default_rng(seed)
    v = ((rng.poisson(3.0, nbins) + 1) * (rng.random(nbins) >= 0.25)).astype(np.uint64)
    for value, at in zip((65535, 65536, 2 ** 32 - 1), rng.permutation(nbins)[:3]):
        v[at] = np.uint64(value)
    v[0] = max(int(v[0]), 1 + seed % 3)
    v[-1] = max(int(v[-1]), 2 + seed % 5)
    return v


class Inputs:
    """n zoned vectors of nbins words; slot 4 of five is slot 1's pointer again"""

    def __init__(self, nbins, n, seed=0):
        distinct = n if n < 5 else 4
        self.host = [mix(nbins, 100 * nbins + 10 * n + j + seed) for j in range(distinct)]
        self.zoned = [zones.zoned_words(v) for v in self.host]
        self.order = list(range(distinct)) + ([1] if n == 5 else [])
        self.vs = [self.host[j] for j in self.order]
        self.ptrs = [self.zoned[j].ptr for j in self.order]
        self.nbins, self.n = nbins, n
        assert all(p % 16 == 0 for p in self.ptrs)

    def assert_clean(self, where):
        import torch
        torch.cuda.synchronize(0)
        for j, z in enumerate(self.zoned):
            z.assert_clean("%s, nbins=%d, n=%d, vector %d" % (where, self.nbins, self.n, j))


@pytest.fixture(scope="module")
def lib(gpu_engine_cls):
    import torch
    from kmerdb_amd import _abi
    torch.cuda.synchronize(0)
    return _abi.lib()


@pytest.fixture(scope="module", params=[(nbins, n) for nbins in NBINS for n in NVECTORS], ids=lambda p: "nbins%d-n%d" % p)
def inputs(request, lib):
    import torch
    ins = Inputs(*request.param)
    torch.cuda.synchronize(0)
    return ins


# ---- the read-only sweeps of n vectors ----

def test_gram_reads_the_payload_alone(inputs):
    from kmerdb_amd import distance
    s, G, _ = distance.gram(inputs.ptrs, inputs.nbins)
    inputs.assert_clean("kdb_gram")
    want_s, want_G = sc.gram_expected(inputs.vs)
    assert s == want_s and G == want_G


def test_pairstats_reads_the_payload_alone(inputs):
    from kmerdb_amd import distance
    got, _ = distance.pairstats_raw(inputs.ptrs, inputs.nbins)
    inputs.assert_clean("kdb_pairstats")
    assert got == sc.pair_expected(inputs.vs)


def test_pairfloat_reads_the_payload_alone(inputs):
    """the bounds of tests/test_gpu_pairstats.py: |C - exact| <= (nbins + 4) 2^-53 exact and |D - ref| <= (16 + nbins D) 2^-53; one
    poison word read for a count would add a term of nearly 1 to C and move D by about ln 2"""
    from kmerdb_amd import distance
    c, d, _ = distance.pairfloat_raw(inputs.ptrs, inputs.nbins)
    inputs.assert_clean("kdb_pairfloat")
    nbins, vs = inputs.nbins, inputs.vs
    for i in range(inputs.n):
        assert c[i][i] == 0.0 and d[i][i] == 0.0
        for j in range(i + 1, inputs.n):
            exact = sc._tp._exact_canberra(vs[i], vs[j])
            assert abs(Fraction(float(c[i][j])) - exact) <= (nbins + 4) * Fraction(1, 2 ** 53) * exact, (i, j)
            ref = sc._tp._decimal_js(vs[i], vs[j])
            assert abs(decimal.Decimal(float(d[i][j])) - ref) <= (16 + nbins * ref) * decimal.Decimal(2) ** -53, (i, j)
            assert c[i][j] == c[j][i] and d[i][j] == d[j][i]


def test_size_factors_read_the_payload_alone(inputs):
    """the bound of tests/test_gpu_sizefactors.py: (n + 10) 2^-53 Lmax, Lmax the largest ln of an eligible count; the number of eligible
    bins is exact, and one poison word past the end would be one more"""
    from kmerdb_amd import matrix
    got, eligible, _ = matrix.size_factors_raw(inputs.ptrs, inputs.nbins)
    inputs.assert_clean("kdb_size_factors")
    ok = np.ones(inputs.nbins, dtype=bool)
    for v in inputs.vs:
        ok &= v > 0
    assert eligible == int(ok.sum())
    if eligible == 0:
        assert all(math.isnan(g) for g in got)
        return
    want, m, lmax = sc._ts._true_log_sf(inputs.vs)
    assert m == eligible
    eps = (inputs.n + 10) * U * lmax
    assert all(abs(float(decimal.Decimal(float(g)) - w)) <= eps for g, w in zip(got, want))


# ---- one vector: spectrum, ranks, scaled counts ----

@pytest.fixture(scope="module", params=NBINS, ids=lambda p: "nbins%d" % p)
def one(request, lib):
    import torch
    v = mix(request.param, 7000 + request.param)
    z = zones.zoned_words(v)
    torch.cuda.synchronize(0)
    return v, z


def _u64p(ptr):
    from kmerdb_amd import _abi
    return ctypes.cast(ctypes.c_void_p(ptr), _abi._u64p)


def _spectrum(lib, ptr, nbins, over_cap):
    """kdb_spectrum with both host outputs inside zones, the list's capacity exact -> (status, dense, over, n_over)"""
    dense = zones.HostZoned(DENSE * 8).write(np.zeros(DENSE, dtype=np.uint64))
    over = zones.HostZoned(over_cap * 8)
    n_over = ctypes.c_uint64(12345)
    rc = lib.kdb_spectrum(0, ctypes.c_void_p(ptr), nbins, _u64p(dense.ptr), _u64p(over.ptr), over_cap, ctypes.byref(n_over), None)
    dense.assert_zones("kdb_spectrum's table")
    over.assert_zones("kdb_spectrum's list of %d" % over_cap)
    return rc, dense.read(np.uint64), over.read(np.uint64), n_over.value


def test_spectrum_reads_the_payload_alone_and_fills_an_exact_list(lib, one):
    from kmerdb_amd import _abi
    v, z = one
    big = np.sort(v[v >= DENSE])
    rc, dense, over, n_over = _spectrum(lib, z.ptr, v.size, big.size)
    z.assert_clean("kdb_spectrum")
    assert rc == _abi.KDB_OK and n_over == big.size
    assert np.array_equal(dense, np.bincount(v[v < DENSE].astype(np.int64), minlength=DENSE).astype(np.uint64))     # (the count of zero bins among them)
    assert np.array_equal(np.sort(over), big)
    if big.size:                                                               # one entry short: refused, the number still reported, nothing behind the cap
        rc, dense, over, n_over = _spectrum(lib, z.ptr, v.size, big.size - 1)
        assert rc == _abi.KDB_ERR_ARG and n_over == big.size
        z.assert_clean("kdb_spectrum, list too short")


@pytest.mark.parametrize("in_place", [False, True], ids=["separate", "in_place"])
def test_rank_transform_writes_its_nbins_words_alone(lib, one, in_place):
    from kmerdb_amd import spectrum
    v, z = one
    want = spc.expected_ranks(v)
    if in_place:
        out = zones.zoned_words(v)
        spectrum.rank_transform_raw(out.ptr, v.size, out.ptr)
    else:
        out = zones.Zoned(v.size * 8, fill=0x5A)
        spectrum.rank_transform_raw(z.ptr, v.size, out.ptr)
        z.assert_clean("kdb_rank_transform's input")
    out.sync()
    out.assert_zones("kdb_rank_transform's output, nbins=%d" % v.size)
    assert np.array_equal(out.read(np.uint64), want)


@pytest.mark.parametrize("as_float64", [0, 1], ids=["uint64", "float64"])
@pytest.mark.parametrize("in_place", [False, True], ids=["separate", "in_place"])
def test_scale_counts_writes_its_nbins_words_alone(lib, one, in_place, as_float64):
    from kmerdb_amd import matrix
    v, z = one
    s = 1.2345678901234567
    q = v.astype(np.float64) / np.float64(s)
    want = q if as_float64 else np.rint(q).astype(np.uint64)
    if in_place:
        out = zones.zoned_words(v)
        matrix.scale_counts_raw(out.ptr, v.size, s, out.ptr, as_float64)
    else:
        out = zones.Zoned(v.size * 8, fill=0x5A)
        matrix.scale_counts_raw(z.ptr, v.size, s, out.ptr, as_float64)
        z.assert_clean("kdb_scale_counts' input")
    out.sync()
    out.assert_zones("kdb_scale_counts' output, nbins=%d" % v.size)
    assert out.read().tobytes() == want.tobytes()


@pytest.mark.parametrize("nbins", [3, 513, 4097])
def test_refused_calls_leave_the_output_as_it_was(lib, nbins):
    """the refusals that exist: a factor that is not finite and positive; a rounded quotient of 2^63 or more, found in the last bin of the
    odd tail.  (kdb_rank_transform's third, nbins >= 2^32, needs a 32 GiB vector to stay inside an allocation: see the next test.)"""
    from kmerdb_amd import _abi
    v = mix(nbins, 8000 + nbins)
    z = zones.zoned_words(v)
    out = zones.Zoned(nbins * 8, fill=0x5A).write(np.full(nbins, 0x1234567, dtype=np.uint64))
    scale = lambda src, s, dst, fl=0: lib.kdb_scale_counts(0, ctypes.c_void_p(src), nbins, ctypes.c_double(s), ctypes.c_void_p(dst), fl, None)
    for s in (float("inf"), float("nan"), 0.0, -2.0):
        for fl in (0, 1):
            assert scale(z.ptr, s, out.ptr, fl) == _abi.KDB_ERR_ARG, s
    v[-1] = np.uint64(TOP)
    z.write(v)
    z.sync()
    assert scale(z.ptr, 2.0, out.ptr) == _abi.KDB_ERR_ARG                      # 2^64 / 2
    assert scale(z.ptr, 1.0, z.ptr) == _abi.KDB_ERR_ARG                        # in place: the input is the output
    out.sync()
    out.assert_clean("kdb_scale_counts refused")
    z.assert_clean("kdb_scale_counts refused in place")
    assert scale(z.ptr, 2.0, out.ptr, 1) == _abi.KDB_OK                        # (the float64 output has no such limit)
    out.sync()
    out.assert_zones("kdb_scale_counts, float64")
    assert out.read().tobytes() == (v.astype(np.float64) / 2.0).tobytes()


def test_rank_transform_refuses_two_to_the_32_bins_and_leaves_them_alone():
    """nbins = 2^32 is refused before anything is read.  The vector is real -- 32 GiB inside its zones, every word the poison -- because no
    length handed to the library may leave its allocation; in place, so the input is the output.  Checked in 4 GiB pieces."""
    import torch
    from kmerdb_amd import _abi
    nbins = 2 ** 32
    free, _ = torch.cuda.mem_get_info(0)
    assert free > 48 * 2 ** 30, "less than 48 GiB free on the device"
    z = zones.Zoned(nbins * 8)
    z.sync()
    assert _abi.lib().kdb_rank_transform(0, ctypes.c_void_p(z.ptr), nbins, ctypes.c_void_p(z.ptr), None) == _abi.KDB_ERR_ARG
    z.sync()
    z.assert_zones("kdb_rank_transform refused")
    words = z.view(torch.int64)
    piece = 2 ** 29
    poison = POISON_WORD - 2 ** 64
    assert all(bool((words[at:at + piece] == poison).all()) for at in range(0, nbins, piece))
    del words, z
    torch.cuda.empty_cache()


# ---- kdb_score_reads: the profile vector ----

@pytest.mark.parametrize("canonical", [False, True], ids=["forward", "canonical"])
@pytest.mark.parametrize("k", [2, 6])
def test_score_reads_reads_the_profile_alone(lib, k, canonical):
    """4^2 words are 128 bytes, less than one wave's load; the last bin (TT..T) is scored by a poly-T record, bin 0 by a poly-A one.
    The integer outputs are exact, log10_p within score_cases' bound."""
    from kmerdb_amd import probability
    import torch
    piece, lanes = spc.header_constant("KDB_SCORE_PIECE"), spc.header_constant("KDB_SCORE_LANES")
    records = score_cases.ragged_records(k, 900 + k, n=24) + [b"A" * 40, b"T" * 40, b"T" * (k - 1) + b"G" + b"T" * k]
    v, _ = (score_cases.canonical_profile if canonical else score_cases.forward_profile)(records, k)
    v[5::7] = 0                                                               # some windows meet an empty bin
    total = int(v.sum())
    z = zones.zoned_words(v)
    bases, offsets = score_cases.pack(records)
    torch.cuda.synchronize(0)
    log10_p, windows, zeros, mins = probability.score_reads(bases, offsets, z.ptr, k, canonical, total, 1)
    z.assert_clean("kdb_score_reads, k=%d" % k)
    for r, rec in enumerate(records):
        s = score_cases.score_record(rec, v, k, canonical, total, 1)
        assert (int(windows[r]), int(zeros[r]), int(mins[r])) == (s.windows, s.zero_windows, s.min_count), r
        if s.log10_p is None:
            assert math.isnan(log10_p[r]), r
        else:
            assert score_cases.error(log10_p[r], s) <= score_cases.bound(s, piece, lanes), r


# ---- host outputs with a capacity: nothing behind it ----

def _host_records(k, seed, n=12):
    rng = np.random.default_rng(seed)
    return [tc.random_record(rng, int(L), p_n=0.02) for L in rng.integers(k, k + 90, size=n)] + [b"ACGT" * 9 + b"N"]


@pytest.mark.parametrize("k", [1, 3, 8])
def test_nullomers_with_an_exact_capacity(gpu_engine_cls, oracle, k):
    from kmerdb_amd import _abi
    bases, offsets = tc.pack([b"ACGTTGCA" * 3, b"AAAAAAAAAAAA", b"GATTACAGATTACA"][:3 if k > 1 else 2])
    want = np.flatnonzero(oracle.c_count(bases, offsets, k, True, oracle.N_DROP)[0] == 0).astype(np.uint64)
    with gpu_engine_cls(k) as eng:
        eng.submit(bases, offsets)
        out = zones.HostZoned(want.size * 8)
        n = ctypes.c_uint64(0)
        _abi.check(eng._lib.kdb_nullomers(eng._h, 0, ctypes.c_void_p(out.ptr) if want.size else None, want.size, ctypes.byref(n)))
        out.assert_zones("kdb_nullomers, cap = *n_out = %d" % want.size)
        assert n.value == want.size and np.array_equal(out.read(np.uint64), want)
        if want.size:                                                          # one short: KDB_ERR_ARG with *n_out set, nothing written behind
            short = zones.HostZoned((want.size - 1) * 8)
            rc = eng._lib.kdb_nullomers(eng._h, 0, ctypes.c_void_p(short.ptr), want.size - 1, ctypes.byref(n))
            assert rc == _abi.KDB_ERR_ARG and n.value == want.size
            short.assert_zones("kdb_nullomers, cap one short")


@pytest.mark.parametrize("canon", [False, True])
@pytest.mark.parametrize("k", [1, 5, 13])
def test_shred_and_window_ids_fill_their_arrays_alone(oracle, k, canon):
    from kmerdb_amd import _abi
    from kmerdb_amd.engine import IdsEngine
    records = _host_records(k, 40 + k)
    bases, offsets = tc.pack(records)
    with IdsEngine(k, canonicalize=canon) as eng:
        ids = zones.HostZoned(bases.size * 8)
        _abi.check(eng._lib.kdb_window_ids(eng._h, bases.ctypes.data, bases.size, offsets.ctypes.data, len(records), ctypes.c_void_p(ids.ptr)))
        ids.assert_zones("kdb_window_ids")
        want = ids_cases.expected_window_ids(bases, offsets, k, canon)
        assert np.array_equal(ids.read(np.uint64), want)
        for rec in records[:4] + records[-1:]:
            w_ids, w_pos = oracle.c_shred(rec, k, canon, oracle.N_DROP)
            cap = len(w_ids)                                                   # exactly the windows emitted
            arr = np.frombuffer(rec, dtype=np.uint8)
            out_ids, out_pos = zones.HostZoned(cap * 8), zones.HostZoned(cap * 8, shift=8)
            n = ctypes.c_size_t(0)
            _abi.check(eng._lib.kdb_shred(eng._h, arr.ctypes.data, arr.size, ctypes.c_void_p(out_ids.ptr), ctypes.c_void_p(out_pos.ptr), cap, ctypes.byref(n)))
            out_ids.assert_zones("kdb_shred ids, cap %d" % cap)
            out_pos.assert_zones("kdb_shred positions, cap %d" % cap)
            assert n.value == cap
            assert np.array_equal(out_ids.read(np.uint64), np.asarray(w_ids, dtype=np.uint64)) and np.array_equal(out_pos.read(np.uint64), np.asarray(w_pos, dtype=np.uint64))


@pytest.mark.parametrize("k,stride,canonical", [(1, 1, False), (3, 3, True), (6, 1, False)])
def test_record_tables_rows_end_where_they_should(lib, k, stride, canonical):
    from kmerdb_amd import _abi
    records = _host_records(k, 60 + k, n=7) + [b""]
    bases, offsets = tc.pack(records)
    n = len(records)
    tables = zones.HostZoned(n * 4 ** k * 4)
    windows, skipped = zones.HostZoned(n * 8), zones.HostZoned(n * 8)
    first, last = zones.HostZoned(n * 4), zones.HostZoned(n * 4, shift=4)
    _abi.check(lib.kdb_record_tables(0, k, stride, 1 if canonical else 0, 0, bases.ctypes.data, bases.size, offsets.ctypes.data, n, 0,
                                     ctypes.c_void_p(tables.ptr), ctypes.c_void_p(windows.ptr), ctypes.c_void_p(skipped.ptr),
                                     ctypes.c_void_p(first.ptr), ctypes.c_void_p(last.ptr), None))
    for name, z in (("tables", tables), ("windows", windows), ("skipped", skipped), ("first_id", first), ("last_id", last)):
        z.assert_zones("kdb_record_tables' " + name)
    want = tc.batch_tables(records, k, stride, canonical)
    got = (tables.read(np.uint32).reshape(n, 4 ** k), windows.read(np.uint64), skipped.read(np.uint64), first.read(np.int32), last.read(np.int32))
    assert all(np.array_equal(g, w) for g, w in zip(got, want))


@pytest.mark.parametrize("k,w,canonical", [(3, 4, True), (11, 10, False)])
def test_minimizers_with_an_exact_capacity(lib, k, w, canonical):
    from kmerdb_amd import _abi
    records = _host_records(k, 80 + k)
    bases, offsets = mc.pack(records)
    n = len(records)
    want_counts, want_ids, want_pos, want_strand = mc.batch_minimizers(records, k, w, canonical, mc.LEX)
    t = int(want_counts.sum())
    assert t > n

    def call(cap):
        counts = zones.HostZoned(n * 8)
        ids, pos, strand = zones.HostZoned(cap * 8), zones.HostZoned(cap * 4), zones.HostZoned(cap)
        total = ctypes.c_uint64(0)
        _abi.check(lib.kdb_minimizers(0, k, w, 1 if canonical else 0, mc.LEX, bases.ctypes.data, bases.size, offsets.ctypes.data, n, ctypes.c_void_p(counts.ptr),
                                      ctypes.c_void_p(ids.ptr), ctypes.c_void_p(pos.ptr), ctypes.c_void_p(strand.ptr), cap, ctypes.byref(total), None))
        for name, z in (("counts", counts), ("ids", ids), ("pos", pos), ("strand", strand)):
            z.assert_zones("kdb_minimizers' %s, cap %d of %d" % (name, cap, t))
        assert total.value == t and np.array_equal(counts.read(np.uint64), want_counts)
        return ids, pos, strand

    ids, pos, strand = call(t)
    assert np.array_equal(ids.read(np.uint64), want_ids) and np.array_equal(pos.read(np.uint32), want_pos) and np.array_equal(strand.read(), want_strand)
    ids, pos, strand = call(t - 1)                                             # one short: the lists are left as they were
    assert all(bool((z.payload == z.fill).all()) for z in (ids, pos, strand))


# ---- that these tests bite: nbins + 1 on a payload of nbins, all inside the tensor ----

@pytest.mark.parametrize("nbins", [1, 512, 513])
def test_bite_a_writer_one_entry_too_far_trips_the_back_zone(lib, nbins):
    from kmerdb_amd import matrix, spectrum
    src = zones.zoned_words(mix(nbins + 1, 5))                                 # (the input has the extra entry: nothing is read outside either)
    for name, call in (("kdb_scale_counts", lambda out: matrix.scale_counts_raw(src.ptr, nbins + 1, 2.0, out.ptr)),
                       ("kdb_scale_counts, float64", lambda out: matrix.scale_counts_raw(src.ptr, nbins + 1, 2.0, out.ptr, True)),
                       ("kdb_rank_transform", lambda out: spectrum.rank_transform_raw(src.ptr, nbins + 1, out.ptr))):
        out = zones.Zoned(nbins * 8)
        out.sync()
        out.assert_zones(name + " before the call")
        call(out)
        out.sync()
        with pytest.raises(AssertionError, match=r"back zone: byte 0 of it \(\+%d from the payload's start\)" % (nbins * 8)):
            out.assert_zones(name)
        assert zones._first_changed(out.front, out.fill) is None                # and only there


@pytest.mark.parametrize("nbins", [1, 512, 513])
def test_bite_a_reader_one_entry_too_far_meets_the_poison(lib, nbins):
    from kmerdb_amd import _abi, distance
    v = mix(nbins, 6)
    z = zones.zoned_words(v)
    z.sync()
    want_s, want_G = sc.gram_expected([v])
    s, G, _ = distance.gram([z.ptr], nbins)
    assert (s, G) == (want_s, want_G)
    s, G, _ = distance.gram([z.ptr], nbins + 1)                                # S = the payload's sum + 0xA5A5..A5 < 2^64: no refusal, another sum
    assert s[0] == want_s[0] + POISON_WORD and G[0][0] == want_G[0][0] + POISON_WORD ** 2
    rc, dense, over, n_over = _spectrum(lib, z.ptr, nbins + 1, int(np.count_nonzero(v >= DENSE)) + 1)
    assert rc == _abi.KDB_OK and n_over == np.count_nonzero(v >= DENSE) + 1 and POISON_WORD in over.tolist()
    z.assert_clean("the bite cases only read")
