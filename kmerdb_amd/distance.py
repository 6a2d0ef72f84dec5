"""kmerdb_amd.distance -- `kmerdb distance` on count profiles (reference kmerdb/__init__.py:577-813, :2314-2338, distance.pyx:108-152).

The moment metrics (METRICS: correlation, pearson, cosine, euclidean, sqeuclidean; `minkowski` is euclidean, scipy's default p = 2) are
functions of the vectors' sums S[i], their Gram matrix G[i][j] = Sum_b x_i[b] x_j[b] and the number of bins N.  The device computes those
as exact 128-bit integers in one sweep of the vectors where they lie in HBM (kdb_gram, csrc/kdb_gram.hip.h); the host does the last step
in exact integer / 150-digit decimal arithmetic, so every value is the float64 nearest the true one, or its neighbour.  No CPU fallback:
without a device moments() raises.

The other metrics people use on count profiles are NOT functions of the moments.  SWEEP_METRICS (cityblock, chebyshev, braycurtis,
hamming / matching and the presence/absence family: jaccard, dice, rogerstanimoto, sokalmichener, russellrao, sokalsneath, yule, kulsinski)
are functions of a second set of exact integers -- per vector S and nnz = #{x > 0}, per pair L1 = Sum |x - y|, Linf = max |x - y|,
ne = #{x != y}, both = #{x > 0 and y > 0} -- which kdb_pairstats makes in one pairwise sweep (csrc/kdb_pairstats.hip.h);
from_pairstats() does the last step in fractions.  FLOAT_METRICS (canberra, jensenshannon) need a quotient or a logarithm per bin: the
float64 sweep kdb_pairfloat, run only when one of the two is asked for.

The presence/absence family is defined on x > 0, which is what scipy computes for jaccard, rogerstanimoto, russellrao, sokalmichener,
sokalsneath and yule on integer input.  Departure from scipy, on purpose: its `dice` on raw counts multiplies the counts and returns a
number without meaning (it can be negative); ours is dice of the presence vectors, i.e. scipy's on `x > 0`.  `kulsinski` follows
scipy <= 1.11's documented formula (later versions dropped the name; the reference still lists it).

Departure from the reference, on purpose: its custom `pearson` (distance.pyx:118-119) rounds both means to float32 before it forms the
residuals; here the means never exist -- num = N Gxy - Sx Sy is an integer.  `correlation` is scipy's 1 - r, the reference CLI's default.

`spearman` (python_distances.py:95-114) is not a function of the count moments, but it is one of the moments of the ranks: rho is
Pearson's r of the mid-ranks.  The device ranks each vector (kdb_rank_transform: doubled mid-ranks, integers; kmerdb_amd/spectrum.py), then
the same exact path runs on the rank vectors.  k <= 15: the doubled ranks of N bins sum to N (N + 1), which kdb_gram needs below 2^64.
"""
import ctypes
import decimal
import fractions
import os
import sys

import numpy as np

from . import _abi

METRICS = ("pearson", "correlation", "cosine", "sqeuclidean", "euclidean")
RANK_METRICS = ("spearman",)                                                         # Pearson's r of the vectors' ranks: the device ranks first
RANK_MAX_BINS = 1 << 32                                                              # kdb_rank_transform refuses this many bins and more
IDENTITY = {"pearson": 1.0, "correlation": 0.0, "cosine": 0.0, "sqeuclidean": 0.0, "euclidean": 0.0}     # python_distances.identity
SWEEP_METRICS = ("cityblock", "chebyshev", "braycurtis", "hamming", "matching", "jaccard", "dice", "rogerstanimoto", "sokalmichener",
                 "russellrao", "sokalsneath", "yule", "kulsinski")                  # functions of kdb_pairstats' integers
FLOAT_METRICS = ("canberra", "jensenshannon")                                        # the float64 sweep, kdb_pairfloat
ALIAS_METRICS = {"minkowski": "euclidean"}                                           # scipy's default p = 2: the moment path
SWEEP_IDENTITY = dict((m, 0.0) for m in SWEEP_METRICS + FLOAT_METRICS)
ALL_METRICS = METRICS + RANK_METRICS + SWEEP_METRICS + FLOAT_METRICS + tuple(ALIAS_METRICS)
_CTX = decimal.Context(prec=150, Emax=decimal.MAX_EMAX, Emin=decimal.MIN_EMIN)       # vx * vy < 2^330 ~ 1e99: held exactly; the quotient to 150 digits


def _require_device(device):
    n = _abi_device_count()
    if n < 1 or not 0 <= int(device) < n:
        raise _abi.KdbHipError("kmerdb_amd.distance needs HIP device {0}; {1} visible (there is no CPU fallback)".format(device, n))


def _abi_device_count():
    n = ctypes.c_int(0)
    rc = _abi.lib().kdb_device_count(ctypes.byref(n))
    if rc != _abi.KDB_OK:
        raise _abi.KdbHipError("no HIP device: {0}".format(_abi.last_error()))
    return n.value


def gram(pointers, nbins, device=0):
    """kdb_gram on raw device pointers -> (sums, gram, kernel_ms): Python ints, both triangles of gram filled."""
    n = len(pointers)
    arr = (ctypes.c_void_p * max(n, 1))(*[ctypes.c_void_p(int(p)) for p in pointers])
    sums = (ctypes.c_uint64 * (2 * max(n, 1)))()
    g = (ctypes.c_uint64 * (2 * max(n, 1) * max(n, 1)))()
    ms = ctypes.c_double(0)
    _abi.check(_abi.lib().kdb_gram(int(device), arr, n, int(nbins), sums, g, ctypes.byref(ms)))
    s = [sums[2 * i] | (sums[2 * i + 1] << 64) for i in range(n)]
    G = [[g[2 * (i * n + j)] | (g[2 * (i * n + j) + 1] << 64) for j in range(n)] for i in range(n)]
    return s, G, ms.value


def _device_vector(v, device):
    """One vector as moments() takes them -> (device pointer, number of bins, the tensor that keeps the memory alive or None for an engine).
    An engine is synced and its table used in place; a host array is uploaded; the caller synchronises the device before a kdb_ call."""
    from .engine import Engine
    if isinstance(v, Engine):
        if v.device != int(device):
            raise ValueError("an engine on device {0} was given, device {1} asked".format(v.device, device))
        v.sync()
        p, nb = v.table_ptr()
        return p, int(nb), None
    if isinstance(v, np.ndarray):
        if v.dtype != np.uint64 or v.ndim != 1:
            raise ValueError("host vectors must be one-dimensional uint64 arrays")
        import torch
        t = torch.from_numpy(np.ascontiguousarray(v).view(np.int64)).to("cuda:{0}".format(int(device)))
        return t.data_ptr(), int(t.numel()), t
    import torch
    if not isinstance(v, torch.Tensor):
        raise TypeError("vectors are Engine objects, torch tensors or numpy arrays, not {0}".format(type(v).__name__))
    if v.dtype not in (torch.int64, torch.uint64) or v.dim() != 1 or not v.is_contiguous():
        raise ValueError("device vectors must be contiguous one-dimensional int64/uint64 tensors")
    if v.device.type != "cuda" or v.device.index != int(device):
        raise ValueError("a tensor on {0} was given, device {1} asked".format(v.device, device))
    return v.data_ptr(), int(v.numel()), v


def _length(v):
    """number of bins of a vector as moments() takes them, without touching the device"""
    if hasattr(v, "nbins"):
        return int(v.nbins)
    if isinstance(v, np.ndarray):
        return int(v.size)
    if hasattr(v, "numel"):
        return int(v.numel())
    raise TypeError("vectors are Engine objects, torch tensors or numpy arrays, not {0}".format(type(v).__name__))


def _check_metric(metric):
    if metric not in ALL_METRICS:
        raise ValueError("unsupported metric '{0}': one of {1}".format(metric, ", ".join(ALL_METRICS)))


def _check_rank_bins(nbins):
    if nbins >= RANK_MAX_BINS:
        raise ValueError("spearman serves k <= 15: {0} bins were given, and the doubled ranks of 2^32 bins or more sum past 2^64".format(nbins))


def moments(vectors, device=0):
    """-> (sums: list[int], gram: n x n list of Python ints), exact, computed on the device.

    `vectors`: any mix of Engine objects (synced; their table is used in place, never copied), torch int64/uint64 tensors on that
    device, and host uint64 numpy arrays (uploaded for the call, freed after it).  ValueError if the lengths differ; KdbHipError
    without a device."""
    ptrs, nbins, keep = _device_pointers(vectors, device, "moments")
    s, G, _ = gram(ptrs, nbins, device)
    del keep
    return s, G


def _device_pointers(vectors, device, who):
    """The vectors as moments() takes them -> (device pointers, number of bins, what keeps the memory alive until the kdb_ call is over)."""
    _require_device(device)
    vectors = list(vectors)
    if not vectors:
        raise ValueError("{0} needs at least one vector".format(who))
    keep, ptrs, lengths = [], [], []
    for v in vectors:
        p, nb, owner = _device_vector(v, device)
        keep.append(owner)
        ptrs.append(p)
        lengths.append(nb)
    if len(set(lengths)) != 1:
        raise ValueError("the vectors differ in length: {0}".format(sorted(set(lengths))))
    if any(o is not None for o in keep):
        import torch
        torch.cuda.synchronize(int(device))              # (uploads and whatever produced the tensors: the kdb_ calls run on a stream of their own)
    return ptrs, lengths[0], keep


def _ratio(num, den2):
    """num / sqrt(den2) of two integers to 150 digits; None where den2 == 0"""
    if den2 == 0:
        return None
    return _CTX.divide(decimal.Decimal(num), _CTX.sqrt(decimal.Decimal(den2)))


def from_moments(sums, gram, nbins, metric):
    """The n x n float64 matrix of `metric` from exact integer moments (pure host code).

        num = N Gxy - Sx Sy,  vx = N Gxx - Sx^2,  vy likewise
        pearson      r = num / sqrt(vx vy)          (the reference's custom metric, without its float32 means: distance.pyx:118-119)
        correlation  1 - r                          (scipy's definition, the reference CLI's default)
        cosine       1 - Gxy / sqrt(Gxx Gyy)
        sqeuclidean  Gxx + Gyy - 2 Gxy;   euclidean  its square root

    The diagonal is the metric's identity (1.0 for pearson, 0.0 otherwise, as python_distances.identity); a zero denominator -- a constant
    vector, or an all-zero one for cosine -- gives nan.  The last step runs in integers and 150-digit decimals: each value is the float64
    nearest the true one, or its neighbour."""
    if metric not in METRICS:
        raise ValueError("unsupported metric '{0}': one of {1}".format(metric, ", ".join(METRICS)))
    n = len(sums)
    N = int(nbins)
    out = np.empty((n, n), dtype=np.float64)
    one = decimal.Decimal(1)
    for i in range(n):
        out[i][i] = IDENTITY[metric]
        for j in range(i + 1, n):
            gxx, gyy, gxy = int(gram[i][i]), int(gram[j][j]), int(gram[i][j])
            if metric in ("pearson", "correlation"):
                sx, sy = int(sums[i]), int(sums[j])
                r = _ratio(N * gxy - sx * sy, (N * gxx - sx * sx) * (N * gyy - sy * sy))
                v = float("nan") if r is None else float(r if metric == "pearson" else _CTX.subtract(one, r))
            elif metric == "cosine":
                r = _ratio(gxy, gxx * gyy)
                v = float("nan") if r is None else float(_CTX.subtract(one, r))
            else:
                d2 = gxx + gyy - 2 * gxy
                v = float(d2) if metric == "sqeuclidean" else float(_CTX.sqrt(decimal.Decimal(d2)))
            out[i][j] = out[j][i] = v
    return out


def pairstats_raw(pointers, nbins, device=0):
    """kdb_pairstats on raw device pointers -> (stats, kernel_ms); stats: a dict of Python ints -- "S" and "nnz" per vector, "L1", "Linf",
    "ne" and "both" as n x n lists with both triangles filled."""
    n = len(pointers)
    m = max(n, 1)
    arr = (ctypes.c_void_p * m)(*[ctypes.c_void_p(int(p)) for p in pointers])
    sums, nnz, l1 = (ctypes.c_uint64 * (2 * m))(), (ctypes.c_uint64 * m)(), (ctypes.c_uint64 * (2 * m * m))()
    linf, ne, both = (ctypes.c_uint64 * (m * m))(), (ctypes.c_uint64 * (m * m))(), (ctypes.c_uint64 * (m * m))()
    ms = ctypes.c_double(0)
    _abi.check(_abi.lib().kdb_pairstats(int(device), arr, n, int(nbins), sums, nnz, l1, linf, ne, both, ctypes.byref(ms)))
    square = lambda a: [[int(a[i * n + j]) for j in range(n)] for i in range(n)]
    return {"S": [sums[2 * i] | (sums[2 * i + 1] << 64) for i in range(n)], "nnz": [int(nnz[i]) for i in range(n)],
            "L1": [[l1[2 * (i * n + j)] | (l1[2 * (i * n + j) + 1] << 64) for j in range(n)] for i in range(n)],
            "Linf": square(linf), "ne": square(ne), "both": square(both)}, ms.value


def pairfloat_raw(pointers, nbins, device=0):
    """kdb_pairfloat on raw device pointers -> (C, D, kernel_ms): two n x n float64 arrays (canberra; twice the squared Jensen-Shannon distance)."""
    n = len(pointers)
    m = max(n, 1)
    arr = (ctypes.c_void_p * m)(*[ctypes.c_void_p(int(p)) for p in pointers])
    c, d = np.zeros((m, m), dtype=np.float64), np.zeros((m, m), dtype=np.float64)
    dp = ctypes.POINTER(ctypes.c_double)
    ms = ctypes.c_double(0)
    _abi.check(_abi.lib().kdb_pairfloat(int(device), arr, n, int(nbins), c.ctypes.data_as(dp), d.ctypes.data_as(dp), ctypes.byref(ms)))
    return c[:n, :n], d[:n, :n], ms.value


def pairstats(vectors, device=0):
    """-> the exact per-vector and per-pair integers of kdb_pairstats as Python ints (see pairstats_raw), computed on the device.
    `vectors` as moments() takes them: engines in place, torch tensors, host arrays; ValueError if the lengths differ."""
    ptrs, nbins, keep = _device_pointers(vectors, device, "pairstats")
    stats, _ = pairstats_raw(ptrs, nbins, device)
    del keep
    return stats


def pairfloat(vectors, device=0):
    """-> (C, D) of kdb_pairfloat, n x n float64 each: canberra, and D with jensenshannon = sqrt(D / 2).  `vectors` as moments() takes them."""
    ptrs, nbins, keep = _device_pointers(vectors, device, "pairfloat")
    c, d, _ = pairfloat_raw(ptrs, nbins, device)
    del keep
    return c, d


def _quotient(num, den):
    """num / den of two integers as the nearest float64 (fractions.Fraction rounds correctly); nan where den == 0"""
    return float("nan") if den == 0 else float(fractions.Fraction(num, den))


def from_pairstats(stats, nbins, metric):
    """The n x n float64 matrix of a SWEEP_METRICS metric from kdb_pairstats' exact integers (pure host code).  With N = nbins,
    ctt = both, ctf = nnz[i] - both, cft = nnz[j] - both, cff = N - nnz[i] - nnz[j] + both and R = ctf + cft:

        cityblock    L1                           chebyshev    Linf
        braycurtis   L1 / (S[i] + S[j])           hamming, matching   ne / N
        jaccard      R / (ctt + R)                dice         R / (2 ctt + R)
        rogerstanimoto, sokalmichener   2 R / (ctt + cff + 2 R)
        russellrao   (N - ctt) / N                sokalsneath  2 R / (ctt + 2 R)
        yule         2 ctf cft / (ctt cff + ctf cft)
        kulsinski    (R - ctt + N) / (R + N)

    The diagonal is 0.0.  A zero denominator gives nan, except where scipy returns a number for the degenerate case: jaccard of two empty
    presence sets and yule with ctf cft == 0 (identical, nested or empty sets) are 0.0.  The quotients are formed in fractions: each value
    is the float64 nearest the true one."""
    if metric not in SWEEP_METRICS:
        raise ValueError("unsupported metric '{0}': one of {1}".format(metric, ", ".join(SWEEP_METRICS)))
    S, nnz = stats["S"], stats["nnz"]
    n = len(S)
    N = int(nbins)
    out = np.empty((n, n), dtype=np.float64)
    for i in range(n):
        out[i][i] = SWEEP_IDENTITY[metric]
        for j in range(i + 1, n):
            ctt = int(stats["both"][i][j])
            ctf, cft = int(nnz[i]) - ctt, int(nnz[j]) - ctt
            cff, R = N - int(nnz[i]) - int(nnz[j]) + ctt, ctf + cft
            if metric == "cityblock":
                v = float(int(stats["L1"][i][j]))
            elif metric == "chebyshev":
                v = float(int(stats["Linf"][i][j]))
            elif metric == "braycurtis":
                v = _quotient(int(stats["L1"][i][j]), int(S[i]) + int(S[j]))
            elif metric in ("hamming", "matching"):
                v = _quotient(int(stats["ne"][i][j]), N)
            elif metric == "jaccard":
                v = 0.0 if ctt + R == 0 else _quotient(R, ctt + R)
            elif metric == "dice":
                v = _quotient(R, 2 * ctt + R)
            elif metric in ("rogerstanimoto", "sokalmichener"):
                v = _quotient(2 * R, ctt + cff + 2 * R)
            elif metric == "russellrao":
                v = _quotient(N - ctt, N)
            elif metric == "sokalsneath":
                v = _quotient(2 * R, ctt + 2 * R)
            elif metric == "yule":
                v = 0.0 if ctf * cft == 0 else _quotient(2 * ctf * cft, ctt * cff + ctf * cft)
            else:                                                                    # kulsinski
                v = _quotient(R - ctt + N, R + N)
            out[i][j] = out[j][i] = v
    return out


def from_pairfloat(c, d, metric):
    """The matrix of a FLOAT_METRICS metric from kdb_pairfloat's sums: canberra = C; jensenshannon = sqrt(D / 2), nan with an all-zero vector."""
    if metric not in FLOAT_METRICS:
        raise ValueError("unsupported metric '{0}': one of {1}".format(metric, ", ".join(FLOAT_METRICS)))
    out = np.array(c if metric == "canberra" else np.sqrt(np.asarray(d, dtype=np.float64) / 2.0), dtype=np.float64)
    np.fill_diagonal(out, SWEEP_IDENTITY[metric])
    return out


def _sweep_matrix(vectors, metric, device):
    """distance_matrix for SWEEP_METRICS and FLOAT_METRICS"""
    if metric in FLOAT_METRICS:
        return from_pairfloat(*pairfloat(vectors, device=device), metric=metric)
    return from_pairstats(pairstats(vectors, device=device), _length(vectors[0]), metric)


def rank_vectors(vectors, device=0):
    """The doubled mid-ranks of every vector, as device tensors (spectrum.ranks).  An engine's table and a caller's tensor are left as
    they are and a host array is uploaded, so n rank vectors are needed: MemoryError, before any device work, if they do not fit the
    free device memory."""
    from . import spectrum
    vectors = list(vectors)
    if not vectors:
        raise ValueError("rank_vectors needs at least one vector")
    lengths = sorted(set(_length(v) for v in vectors))
    if len(lengths) != 1:
        raise ValueError("the vectors differ in length: {0}".format(lengths))
    _check_rank_bins(lengths[0])
    _require_device(device)
    import torch
    need = 8 * lengths[0] * len(vectors)
    free_b, _ = torch.cuda.mem_get_info(int(device))
    if need > free_b:
        raise MemoryError("the rank vectors of {0} profiles of {1} bins need {2} bytes of device memory, {3} are free".format(
            len(vectors), lengths[0], need, free_b))
    return [spectrum.ranks(v, device=device) for v in vectors]


def _check_normalize(normalize):
    from . import matrix
    matrix.check_normalize(normalize)


def distance_matrix(vectors, metric="correlation", device=0, normalize=None):
    """moments() on the device, then from_moments(); for `spearman` the device ranks the vectors first (rank_vectors) and the moments are
    those of the ranks; for SWEEP_METRICS pairstats() and from_pairstats(); for FLOAT_METRICS pairfloat().  normalize="DESeq2": the
    vectors are first divided by their median-of-ratios size factors and rounded to integers (matrix.normalize: new vectors for engines and
    the caller's tensors, which stay as they are), and everything above runs on those."""
    _check_metric(metric)
    _check_normalize(normalize)
    metric = ALIAS_METRICS.get(metric, metric)
    vectors = list(vectors)
    if normalize is not None:
        if not vectors:
            raise ValueError("distance_matrix needs at least one vector")
        from . import matrix
        vectors, _ = matrix.normalize(vectors, device=device, ints=True)
    if metric in SWEEP_METRICS + FLOAT_METRICS:
        if not vectors:
            raise ValueError("distance_matrix needs at least one vector")
        return _sweep_matrix(vectors, metric, device)
    if metric in RANK_METRICS:
        vectors, metric = rank_vectors(vectors, device=device), "pearson"
    s, G = moments(vectors, device=device)
    return from_moments(s, G, _length(vectors[0]), metric)


def spearman(x, y, device=0):
    """Spearman's rho of two count vectors (the reference's python_distances.spearman, :95-114, which calls scipy.stats.spearmanr): exact
    Pearson's r of their mid-ranks, ties sharing the mean of their ranks as scipy ranks them; nan if either vector is constant.
    -> rho alone: the p-value the reference returns beside it (and drops, __init__.py:735-738) is not reproduced."""
    vecs = [np.ascontiguousarray(v, dtype=np.uint64) if isinstance(v, (np.ndarray, list, tuple)) else v for v in (x, y)]
    return float(distance_matrix(vecs, "spearman", device=device)[0][1])


def correlation(a, b, total_kmers):
    """The reference's distance.correlation(a, b, total_kmers) (distance.pyx:108-152), drop-in: Pearson's r of two count vectors of
    `total_kmers` entries -- exact moments on the device instead of the long double loop with float32 means."""
    if total_kmers != len(a) or total_kmers != len(b):
        raise ValueError("NumPy kmer count array total does not match length of arrays")
    vecs = [np.ascontiguousarray(v, dtype=np.uint64) for v in (a, b)]
    s, G = moments(vecs)
    return float(from_moments(s, G, total_kmers, "pearson")[0][1])


def format_matrix(dist, columns, output_delimiter="\t"):
    """What the reference prints (kmerdb/__init__.py:800-813): the one off-diagonal number of a 2 x 2 result; otherwise a header row and rows
    of repr(float), nan as an empty field -- pandas' DataFrame(dist, columns=columns).to_csv(sep=..., index=False)."""
    dist = np.asarray(dist, dtype=np.float64)
    if dist.shape == (2, 2):
        return "{0}\n".format(repr(float(dist[0][1])))
    if len(columns) != dist.shape[1]:
        raise ValueError("{0} column names for {1} columns".format(len(columns), dist.shape[1]))
    lines = [output_delimiter.join(str(c) for c in columns)]
    for row in dist:
        lines.append(output_delimiter.join("" if x != x else repr(float(x)) for x in row))
    return "\n".join(lines) + "\n"


def column_names_for(inputs, column_names=None):
    """basename.split(".")[0] of every input, or the lines of the names file (kmerdb/__init__.py:645-651)."""
    if column_names is None:
        columns = [os.path.basename(p).split(".")[0] for p in inputs]
    else:
        with open(column_names) as f:
            columns = [line.rstrip() for line in f]
    if len(columns) != len(inputs):
        raise RuntimeError("Number of column names {0} does not match number of input files {1}...".format(len(columns), len(inputs)))
    return columns


def distances(inputs, metric, column_names=None, output_delimiter="\t", out=None, device=0, normalize=None):
    """The reference driver for two or more .kdb files (kmerdb/__init__.py:616-661, :796-813): read the profiles, one sweep on the device,
    print the matrix.  normalize="DESeq2": the profiles are normalised where they were uploaded (`kmerdb matrix DESeq2`) first.
    -> the matrix."""
    from . import fileutil
    inputs = list(inputs)
    _check_metric(metric)
    _check_normalize(normalize)
    if len(inputs) < 2:
        raise ValueError("'kmerdb distance' requires more than one .kdb file as positional inputs")
    if not all(os.path.splitext(p)[-1] == ".kdb" for p in inputs):
        raise IOError("One or more parseable .kdb filepaths did not end in '.kdb'")
    ks = [int(fileutil._read_header(p)["k"]) for p in inputs]
    if any(k != ks[0] for k in ks):
        raise TypeError("One or more files did not have k set to be equal to {0}: {1}".format(ks[0], ks))
    columns = column_names_for(inputs, column_names)
    _require_device(device)
    profiles = [fileutil.read_kdb(p).counts for p in inputs]
    dist = distance_matrix(profiles, metric=metric, device=device, normalize=normalize)     # (host arrays: scaled where they are uploaded)
    (sys.stdout if out is None else out).write(format_matrix(dist, columns, output_delimiter))
    return dist


def profile_distances(files, k, metric="correlation", no_ambiguous=False, do_not_canonicalize=False, device=0, normalize=None):
    """Count the files of a samplesheet and compare their profiles without leaving HBM: one engine counts each file, its vector is copied
    device-to-device into row i of one n x 4^k tensor, the engine is reset; then one moments() call (for `spearman` the rows are ranked in
    place first: no further memory; the sweeps of SWEEP_METRICS and FLOAT_METRICS read the rows where they lie: none either).  MemoryError before counting if
    n * 8 * 4^k plus one engine does not fit the free device memory.  normalize="DESeq2": the rows are divided by their size factors
    and rounded, in place, before anything else (matrix.normalize).  -> (matrix, columns, per-file metadata)."""
    from . import parse
    from .engine import Engine, KDB_N_DROP, KDB_N_EXPAND
    if type(k) is not int:
        raise TypeError("k must be an int")
    _check_metric(metric)
    _check_normalize(normalize)
    metric = ALIAS_METRICS.get(metric, metric)
    if metric in RANK_METRICS:
        _check_rank_bins(4 ** k)
    files = list(files)
    if not files:
        raise ValueError("profile_distances needs at least one file")
    _require_device(device)
    import torch
    n, N = len(files), 4 ** k
    engine_bytes = 8 * N + ((6 << 30) if k >= 13 else (1 << 30))             # the vector and the engine's staging and scatter scratch
    free_b, _ = torch.cuda.mem_get_info(int(device))
    if n * 8 * N + engine_bytes > free_b:
        raise MemoryError("{0} profiles of 4^{1} bins and one engine need {2} bytes of device memory, {3} are free".format(
            n, k, n * 8 * N + engine_bytes, free_b))
    rows = torch.empty((n, N), dtype=torch.int64, device="cuda:{0}".format(int(device)))
    metadata = []
    with Engine(k, canonicalize=not do_not_canonicalize, n_mode=KDB_N_DROP if no_ambiguous else KDB_N_EXPAND, device=device) as eng:
        for i, f in enumerate(files):
            metadata.append(parse.parsefile_folded(f, k, eng, replace_with_none=bool(no_ambiguous), fold=False))
            rows[i].copy_(eng.table_tensor())
            torch.cuda.synchronize(int(device))
            eng.reset()
    if normalize is not None:                                                # the rows are this function's own: scaled where they lie
        from . import matrix
        matrix.normalize([rows[i] for i in range(n)], device=device, ints=True, inplace=True)
    if metric in RANK_METRICS:                                               # ranked where they lie, too
        from . import spectrum
        for i in range(n):
            spectrum.ranks(rows[i], out=rows[i], device=device)
        metric = "pearson"
    if metric in SWEEP_METRICS + FLOAT_METRICS:
        return _sweep_matrix([rows[i] for i in range(n)], metric, device), column_names_for(files), metadata
    s, G = moments([rows[i] for i in range(n)], device=device)
    return from_moments(s, G, N, metric), column_names_for(files), metadata
