"""kmerdb_amd.spectrum -- the abundance spectrum of a count profile (how many bins hold each count value: the classic k-mer histogram
with its error k-mers, coverage peak and repeats) and the profile's ranks, both computed where the vector lies in HBM.

The reference tallies the spectrum at the end of every `profile` with a Python loop over the 4^k bins (util.get_histo, lexer.max:
kmerdb/__init__.py:2000, util.py:92-116).  Here one sweep on the device does it (kdb_spectrum, csrc/kdb_spectrum.hip.h), exactly, for
every uint64 value; a second, elementwise sweep turns the vector into its doubled mid-ranks (kdb_rank_transform), from which
kmerdb_amd.distance takes Spearman's rho through the exact moments it already has.  No CPU fallback: without a device these raise.

Vectors are what distance.moments takes: Engine objects (synced, their table read in place and never modified), torch int64/uint64
tensors on the device, host uint64 numpy arrays (uploaded for the call).
"""
import ctypes

import numpy as np

from . import _abi
from .distance import _check_rank_bins, _device_vector, _length, _require_device

DENSE = _abi.KDB_SPECTRUM_DENSE
_FIRST_CAP = 4096                      # values of DENSE and above a first call has room for; a profile has few, and a second call takes the rest


def spectrum_raw(ptr, nbins, device=0):
    """kdb_spectrum on a raw device pointer -> (dense: uint64[DENSE] multiplicities, over: the values >= DENSE in no particular order,
    kernel_ms of the last sweep)."""
    lib = _abi.lib()
    dense = np.zeros(DENSE, dtype=np.uint64)
    n_over = ctypes.c_uint64(0)
    ms = ctypes.c_double(0)
    cap = _FIRST_CAP
    while True:
        over = np.empty(cap, dtype=np.uint64)
        rc = lib.kdb_spectrum(int(device), ctypes.c_void_p(int(ptr)), int(nbins), dense.ctypes.data_as(_abi._u64p), over.ctypes.data_as(_abi._u64p),
                              cap, ctypes.byref(n_over), ctypes.byref(ms))
        if rc == _abi.KDB_ERR_ARG and n_over.value > cap:          # (the list was longer: now its length is known)
            cap = n_over.value
            continue
        _abi.check(rc)
        return dense, over[:n_over.value], ms.value


def rank_transform_raw(ptr, nbins, out_ptr, device=0):
    """kdb_rank_transform on raw device pointers (out_ptr may equal ptr) -> kernel_ms of its sweeps."""
    ms = ctypes.c_double(0)
    _abi.check(_abi.lib().kdb_rank_transform(int(device), ctypes.c_void_p(int(ptr)), int(nbins), ctypes.c_void_p(int(out_ptr)), ctypes.byref(ms)))
    return ms.value


def _resolve(vector, device):
    _require_device(device)
    ptr, nbins, owner = _device_vector(vector, device)
    if owner is not None:
        import torch
        torch.cuda.synchronize(int(device))          # (the upload, or whatever produced the tensor: the kdb_ calls run on a stream of their own)
    return ptr, nbins, owner


def spectrum(vector, device=0):
    """-> (values, multiplicities): two ascending uint64 arrays -- the count values that occur in the vector, 0 included, and how many
    bins hold each.  Exact for every value up to 2^64 - 1 and every multiplicity."""
    ptr, nbins, owner = _resolve(vector, device)
    dense, over, _ = spectrum_raw(ptr, nbins, device)
    del owner
    small = np.flatnonzero(dense).astype(np.uint64)
    big, big_n = np.unique(over, return_counts=True)
    return np.concatenate([small, big.astype(np.uint64)]), np.concatenate([dense[small.astype(np.int64)], big_n.astype(np.uint64)])


def ranks(vector, out=None, device=0):
    """-> the vector's doubled mid-ranks as a torch int64 tensor on the device: 2 #{bins that hold less} + #{bins that hold the same} + 1,
    twice scipy.stats.rankdata's value and an integer; they sum to N (N + 1).  `out`: a contiguous int64/uint64 tensor of the vector's
    length on the device to write them to; it may be the input tensor itself (in place).  Without it a new tensor is made for an engine or
    a tensor, which stay as they are; a host array is ranked where it was uploaded.  ValueError for 2^32 bins or more (k >= 16)."""
    import torch
    _check_rank_bins(_length(vector))                # (before anything is uploaded)
    ptr, nbins, owner = _resolve(vector, device)
    if out is None:
        uploaded = isinstance(vector, np.ndarray)
        out = owner if uploaded else torch.empty(nbins, dtype=torch.int64, device="cuda:{0}".format(int(device)))
    else:
        if not isinstance(out, torch.Tensor) or out.dtype not in (torch.int64, torch.uint64) or out.dim() != 1 or not out.is_contiguous():
            raise ValueError("out must be a contiguous one-dimensional int64/uint64 tensor")
        if out.device.type != "cuda" or out.device.index != int(device) or out.numel() != nbins:
            raise ValueError("out must hold {0} bins on device {1}".format(nbins, device))
    torch.cuda.synchronize(int(device))
    rank_transform_raw(ptr, nbins, out.data_ptr(), device)
    return out


def kmer_coverage(vector, device=0):
    """The reference's lexer.max(util.get_histo(list(counts))) (kmerdb/__init__.py:2000) -> (count, bins): the count value above 2 that the
    most bins hold -- the smallest such value where several tie -- and how many hold it; (0, 0) if no bin holds more than 2."""
    values, mult = spectrum(vector, device=device)
    best, m = 0, 0
    for v, n in zip(values.tolist(), mult.tolist()):
        if v > 2 and n > m:
            best, m = v, n
    return best, m
