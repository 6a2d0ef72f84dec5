"""kmerdb_amd.matrix -- `kmerdb matrix` on count profiles (reference kmerdb/__init__.py:815-1043): the count matrix of several .kdb files,
as it is (`from`, `Frequency`) or normalised for sequencing depth (`DESeq2`, the branch at :930-977).

The reference normalises through rpy2 and R's DESeq2 (estimateSizeFactors, counts(normalized=TRUE)).  Here the same numbers -- the
median-of-ratios size factors of Anders & Huber (2010) -- are computed on the device, on the vectors where they lie in HBM
(kdb_size_factors, kdb_scale_counts; csrc/kdb_sizefactors.hip.h).  For n count vectors x_1 .. x_n:

    a bin b is eligible iff x_j[b] > 0 for every j          L[b] = (1/n) Sum_j ln x_j[b] on eligible bins
    ln s_j = median over the eligible bins of ln x_j[b] - L[b]          normalised count = x_j[b] / s_j

rounded half to even to an integer by default (the reference's np.rint(...).astype(int64); `--no-normalized-ints` keeps the float64
quotients).  No CPU fallback: without a device size_factors() raises.  PCA and tSNE (scikit-learn on the host in the reference) are not
offered; a .tsv or STDIN matrix as input is not read.
"""
import ctypes
import math
import os
import sys

import numpy as np

from . import _abi
from .distance import _device_pointers, _length, _require_device, column_names_for

METHODS = ("from", "Frequency", "DESeq2")
NOT_OFFERED = ("PCA", "tSNE")
NORMALIZE = ("DESeq2",)
NO_ELIGIBLE = "every k-mer contains at least one zero, cannot compute log geometric means"        # DESeq2's message
_CHUNK_ROWS = 1 << 16


def check_normalize(normalize):
    if normalize is not None and normalize not in NORMALIZE:
        raise ValueError("unsupported normalisation '{0}': None or one of {1}".format(normalize, ", ".join(NORMALIZE)))


def size_factors_raw(pointers, nbins, device=0):
    """kdb_size_factors on raw device pointers -> (ln s: float64[n], eligible: int, kernel_ms); ln s is nan where eligible == 0."""
    n = len(pointers)
    arr = (ctypes.c_void_p * max(n, 1))(*[ctypes.c_void_p(int(p)) for p in pointers])
    log_sf = np.zeros(max(n, 1), dtype=np.float64)
    eligible, ms = ctypes.c_uint64(0), ctypes.c_double(0)
    _abi.check(_abi.lib().kdb_size_factors(int(device), arr, n, int(nbins), log_sf.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), ctypes.byref(eligible),
                                           ctypes.byref(ms)))
    return log_sf[:n], int(eligible.value), ms.value


def scale_counts_raw(pointer, nbins, size_factor, out_pointer, as_float64=False, device=0):
    """kdb_scale_counts on raw device pointers -> kernel_ms"""
    ms = ctypes.c_double(0)
    _abi.check(_abi.lib().kdb_scale_counts(int(device), ctypes.c_void_p(int(pointer)), int(nbins), float(size_factor), ctypes.c_void_p(int(out_pointer)),
                                           1 if as_float64 else 0, ctypes.byref(ms)))
    return ms.value


def _size_factors(ptrs, nbins, device):
    log_sf, eligible, _ = size_factors_raw(ptrs, nbins, device)
    if eligible == 0:
        raise ValueError(NO_ELIGIBLE)
    return np.array([math.exp(v) for v in log_sf], dtype=np.float64), eligible


def size_factors(vectors, device=0):
    """-> (sf: float64[n], eligible: int): the median-of-ratios size factor of every vector and the number of bins that are positive in
    all of them, computed on the device.  `vectors` as distance.moments() takes them: engines in place, torch tensors, host arrays.
    ValueError if no bin is eligible (DESeq2's message) or the lengths differ; KdbHipError without a device."""
    ptrs, nbins, keep = _device_pointers(vectors, device, "size_factors")
    sf, eligible = _size_factors(ptrs, nbins, device)
    del keep
    return sf, eligible


def normalize(vectors, device=0, ints=True, inplace=False):
    """-> (list of device tensors, sf): every vector divided by its size factor -- int64 tensors of the quotients rounded half to even
    (ints=True), or float64 tensors of the quotients.  inplace=True: every vector is a torch tensor that the caller owns and is overwritten
    (a float64 result is returned as a view of the same memory).  Otherwise engines and the caller's tensors stay as they are, host arrays
    are scaled where they were uploaded, and new vectors are made for the rest: MemoryError, before any device work, if they do not fit the
    free device memory.  ValueError if no bin is eligible, or if a rounded quotient reaches 2^63."""
    vectors = list(vectors)
    if not vectors:
        raise ValueError("normalize needs at least one vector")
    lengths = sorted(set(_length(v) for v in vectors))
    if len(lengths) != 1:
        raise ValueError("the vectors differ in length: {0}".format(lengths))
    _require_device(device)
    import torch
    if inplace:
        if not all(isinstance(v, torch.Tensor) for v in vectors):
            raise ValueError("inplace=True takes torch tensors that the caller owns")
    else:
        need = 8 * lengths[0] * sum(1 for v in vectors if not isinstance(v, np.ndarray))
        free_b, _ = torch.cuda.mem_get_info(int(device))
        if need > free_b:
            raise MemoryError("the normalised vectors of {0} profiles of {1} bins need {2} bytes of device memory, {3} are free".format(
                len(vectors), lengths[0], need, free_b))
    ptrs, nbins, keep = _device_pointers(vectors, device, "normalize")
    sf, _ = _size_factors(ptrs, nbins, device)
    outs = []
    for v, p, owner, s in zip(vectors, ptrs, keep, sf):
        if inplace or isinstance(v, np.ndarray):                                        # (an uploaded array is this call's own)
            out = owner
        else:
            out = torch.empty(nbins, dtype=torch.int64, device="cuda:{0}".format(int(device)))
        scale_counts_raw(p, nbins, s, out.data_ptr(), as_float64=not ints, device=device)
        if ints and out.dtype != torch.int64:
            out = out.view(torch.int64)
        outs.append(out if ints else out.view(torch.float64))
    return outs, sf


def format_columns(columns_data, columns, output_delimiter="\t", with_index=False, first_row=0, header=True):
    """What pandas' DataFrame(dict(zip(columns, columns_data))).to_csv(sep=..., index=with_index) prints: a header row (an empty first
    field with the index), then a row per bin -- integers as decimals, floats as repr(float).  Vectorised: numpy forms each column's
    strings and joins the columns; `first_row` and `header` let a caller print a long matrix in chunks."""
    if len(columns) != len(columns_data):
        raise ValueError("{0} column names for {1} columns".format(len(columns), len(columns_data)))
    parts = []
    if header:
        parts.append(output_delimiter.join(([""] if with_index else []) + [str(c) for c in columns]) + "\n")
    nrows = len(columns_data[0]) if columns_data else 0
    if nrows == 0:
        return "".join(parts)
    fields = [np.arange(first_row, first_row + nrows).astype(str)] if with_index else []
    for col in columns_data:
        col = np.asarray(col)
        if len(col) != nrows:
            raise ValueError("the columns differ in length")
        fields.append(col.astype(str))
    line = fields[0]
    for f in fields[1:]:
        line = np.char.add(np.char.add(line, output_delimiter), f)
    parts.append("\n".join(line.tolist()))
    parts.append("\n")
    return "".join(parts)


def check_method(method):
    if method in NOT_OFFERED:
        raise ValueError("'kmerdb matrix {0}' is not offered: PCA and tSNE are scikit-learn on the host in the reference, with nothing for the device to do".format(method))
    if method not in METHODS:
        raise ValueError("unsupported method '{0}': one of {1}".format(method, ", ".join(METHODS)))


def matrix(inputs, method, column_names=None, output_delimiter="\t", with_index=False, no_normalized_ints=False, out=None, device=0):
    """The reference driver for two or more .kdb files (kmerdb/__init__.py:844-896, :1041): read the profiles, normalise them on the device
    (`DESeq2`) or pass them through (`from`, `Frequency`), print the 4^k x n matrix.  -> the columns as numpy arrays (uint64 counts; int64
    or float64 normalised counts)."""
    from . import fileutil
    inputs = list(inputs)
    check_method(method)
    if len(inputs) < 2:
        raise ValueError("'kmerdb matrix' requires more than one .kdb file as positional inputs")
    if not all(os.path.splitext(p)[-1] == ".kdb" for p in inputs):
        raise IOError("One or more parseable .kdb filepaths did not end in '.kdb'")
    ks = [int(fileutil._read_header(p)["k"]) for p in inputs]
    if any(k != ks[0] for k in ks):
        raise TypeError("One or more files did not have k set to be equal to {0}: {1}".format(ks[0], ks))
    columns = column_names_for(inputs, column_names)
    if method == "DESeq2":
        _require_device(device)
    profiles = [fileutil.read_kdb(p).counts for p in inputs]
    if method == "DESeq2":
        tensors, _ = normalize(profiles, device=device, ints=not no_normalized_ints)
        profiles = [t.cpu().numpy() for t in tensors]
        del tensors
    stream = sys.stdout if out is None else out
    nrows = len(profiles[0])
    stream.write(format_columns([p[:0] for p in profiles], columns, output_delimiter, with_index))          # (the header row)
    for r0 in range(0, nrows, _CHUNK_ROWS):
        stream.write(format_columns([p[r0:r0 + _CHUNK_ROWS] for p in profiles], columns, output_delimiter, with_index, first_row=r0, header=False))
    return profiles
