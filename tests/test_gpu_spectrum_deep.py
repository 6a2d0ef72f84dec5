"""GPU: kdb_spectrum and kdb_rank_transform past one grid stride, through partial merges, at the overflow list's first guess, over a
million distinct large values and up to ranks of 2^32 and more: the cases of tests/spectrum_cases.py (tests/test_spectrum_cases_cpu.py
proves each is where it claims to be) against np.unique(..., return_counts=True) and 2 below + eq + 1.  Everything is exact."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import spectrum_cases as sc  # noqa: E402

pytestmark = pytest.mark.gpu

POISON = 0xDEAD


@pytest.fixture(scope="module")
def dev(gpu_engine_cls):
    import torch
    from kmerdb_amd import _abi, spectrum

    class Dev:
        lib = _abi.lib()
        OK, ARG = _abi.KDB_OK, _abi.KDB_ERR_ARG

        @staticmethod
        def upload(a):
            return torch.from_numpy(np.array(a, dtype=np.uint64).view(np.int64)).to("cuda:0")          # (a copy: the cases are read-only)

        @staticmethod
        def download(t):
            torch.cuda.synchronize(0)
            return t.cpu().numpy().view(np.uint64)

        @staticmethod
        def spectrum(t):
            """-> (values, multiplicities) put together from the C call's two outputs"""
            torch.cuda.synchronize(0)
            dense, over, _ = spectrum.spectrum_raw(t.data_ptr(), t.numel())
            assert dense.shape == (sc.DENSE,) and (over >= sc.DENSE).all()
            small = np.flatnonzero(dense)
            big, big_n = np.unique(over, return_counts=True)
            return np.concatenate([small.astype(np.uint64), big]), np.concatenate([dense[small], big_n.astype(np.uint64)])

        @staticmethod
        def rank(t, out):
            torch.cuda.synchronize(0)
            spectrum.rank_transform_raw(t.data_ptr(), t.numel(), out.data_ptr())

        @classmethod
        def raw_spectrum(cls, t, over_cap):
            """the C call with a list of exactly over_cap entries -> (status, n_over, dense, the list)"""
            dense = np.zeros(sc.DENSE, dtype=np.uint64)
            over = np.full(max(over_cap, 1), POISON, dtype=np.uint64)
            n_over = ctypes.c_uint64(12345)
            torch.cuda.synchronize(0)
            rc = cls.lib.kdb_spectrum(0, ctypes.c_void_p(t.data_ptr()), t.numel(), dense.ctypes.data_as(_abi._u64p), over.ctypes.data_as(_abi._u64p),
                                      over_cap, ctypes.byref(n_over), None)
            return rc, n_over.value, dense, over
    return Dev


def _check(dev, v):
    """the spectrum, the ranks out of place into a poisoned vector and in place, their sum, and all of it a second time -> the spectrum"""
    n = v.size
    t = dev.upload(v)
    want_values, want_mult = sc.expected_spectrum(v)
    want = sc.expected_ranks(v)
    got_spectrum = None
    for call in (1, 2):
        values, mult = dev.spectrum(t)
        assert np.array_equal(values, want_values), call
        assert np.array_equal(mult, want_mult), (call, values[mult != want_mult][:8], mult[mult != want_mult][:8], want_mult[mult != want_mult][:8])
        got_spectrum = (values, mult)
        assert np.array_equal(dev.download(t), v)                           # (the sweep only reads)
        out = dev.upload(np.full(n, POISON, dtype=np.uint64))
        dev.rank(t, out)
        got = dev.download(out)
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, (call, bad.size, bad[:8], v[bad[:8]], got[bad[:8]], want[bad[:8]])
        assert np.array_equal(dev.download(t), v)                           # (the input of an out-of-place call stays)
        assert sum(int(x) for x in np.add.reduceat(got, np.arange(0, n, 4096))) == n * (n + 1)
    dev.rank(t, t)
    assert np.array_equal(dev.download(t), want)
    return got_spectrum


@pytest.mark.parametrize("name", sorted(sc.CASES))
def test_the_cases_of_spectrum_cases(dev, name):
    v, _ = sc.case(name)
    values, mult = _check(dev, v)
    if name.startswith("c_"):                                                # a value moved by one slot: the same spectrum
        other, _ = sc.case("c_one_large_value_per_wave" if name.endswith("moved_a_slot") else "c_one_large_value_per_wave_moved_a_slot")
        assert not np.array_equal(other, v)
        other_values, other_mult = dev.spectrum(dev.upload(other))
        assert np.array_equal(values, other_values) and np.array_equal(mult, other_mult)


@pytest.mark.parametrize("name", ["d_list_length_guess", "d_list_length_guess_plus_1", "d_list_length_guess_plus_a_workgroup", "e_many_distinct_large_values"])
def test_kdb_spectrum_with_a_list_of_exactly_the_length_and_one_short(dev, name):
    v, _ = sc.case(name)
    t = dev.upload(v)
    large = np.sort(v[v >= sc.DENSE])
    dense_want = np.bincount(v[v < sc.DENSE].astype(np.int64), minlength=sc.DENSE).astype(np.uint64)
    rc, n_over, dense, over = dev.raw_spectrum(t, large.size)
    assert (rc, n_over) == (dev.OK, large.size)
    assert np.array_equal(np.sort(over), large) and np.array_equal(dense, dense_want)
    # one entry short: the status says so, the length and the table are right all the same
    rc, n_over, dense, over = dev.raw_spectrum(t, large.size - 1)
    assert (rc, n_over) == (dev.ARG, large.size) and np.array_equal(dense, dense_want)
    # the first guess of kdb_rank_transform as the list's length
    rc, n_over, dense, over = dev.raw_spectrum(t, sc.GUESS)
    assert (rc, n_over) == (dev.OK if large.size <= sc.GUESS else dev.ARG, large.size) and np.array_equal(dense, dense_want)


@pytest.mark.parametrize("nfull", sc.WIDE_SEGMENTS)
def test_ranks_of_two_to_the_32_and_more_in_place(dev, nfull):
    """x[b] = T[b >> 20] over 2^31 + 1101 bins (16 GiB) and over 2^32 - 2^20 + 1101 bins (32 GiB), ranked in place and compared on the
    device.  2 below + eq + 1 >= 2^32 with below + eq <= N needs eq <= 2 N + 1 - 2^32: at N = 2^31 + 1101 only a value that at most 2203
    bins hold can reach it, so of segments of 2^20 bins only the short last one does -- there it takes the way of the binary search.  At
    N = 2^32 - 2^20 + 1101, the longest vector of whole segments the call accepts, more than half of the segments do, in the LDS table,
    the global table and the searched list alike."""
    import torch
    t_host, lengths = sc.wide_table(nfull)
    n = sum(lengths)
    free_b, _ = torch.cuda.mem_get_info(0)
    if free_b < n * 8 + 4 * 10 ** 9:
        pytest.skip("under {0} GB of device memory free".format((n * 8 + 4 * 10 ** 9) // 10 ** 9))
    ranks, (want_values, want_mult) = sc.segment_ranks(t_host, lengths)
    wide = sum(r >= 2 ** 32 for r in ranks)
    assert ranks[-1] >= 2 ** 32 and (wide >= (nfull + 1) / 2 if n >= 2 ** 32 - 2 ** 20 else wide == 1)
    seg = sc.SEGMENT
    table = torch.from_numpy(t_host.view(np.int64)).to("cuda:0")
    want = torch.from_numpy(np.array(ranks, dtype=np.uint64).view(np.int64)).to("cuda:0")
    x = torch.empty(n, dtype=torch.int64, device="cuda:0")
    try:
        x[:nfull * seg].view(nfull, seg).copy_(table[:nfull, None].expand(nfull, seg))
        x[nfull * seg:] = table[nfull]
        values, mult = dev.spectrum(x)
        assert [int(a) for a in values] == want_values and [int(a) for a in mult] == want_mult
        assert max(want_mult) >= 2 ** 20 * (nfull // 4)
        dev.rank(x, x)
        torch.cuda.synchronize(0)
        wrong = []
        for s0 in range(0, nfull, 256):
            s1 = min(nfull, s0 + 256)
            ok = (x[s0 * seg:s1 * seg].view(s1 - s0, seg) == want[s0:s1, None]).all(dim=1)
            wrong += [s0 + int(i) for i in torch.nonzero(~ok).flatten().tolist()]
        if not bool((x[nfull * seg:] == want[nfull]).all()):
            wrong.append(nfull)
        assert wrong == [], [(s, int(t_host[s]), ranks[s], int(x[s * seg]) & (2 ** 64 - 1)) for s in wrong[:8]]
    finally:
        del x
        torch.cuda.empty_cache()
