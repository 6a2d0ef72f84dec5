"""The batch every per-record call takes (kdb_score_reads, kdb_record_tables, kdb_minimizers): concatenated residues and the nreads + 1
offsets of their records, as Engine.submit takes them."""
import numpy as np

MAX_RESIDUES = 1 << 30                     # per call


def check_batch(module, bases, offsets):
    """-> (bases: contiguous uint8[nbytes], offsets: contiguous uint64[nreads + 1]); module: the caller's name, which its messages begin with"""
    if isinstance(bases, (bytes, bytearray, memoryview)):
        bases = np.frombuffer(bases, dtype=np.uint8)
    if not isinstance(bases, np.ndarray) or bases.dtype != np.uint8 or bases.ndim != 1:
        raise TypeError("kmerdb_amd.{0}: bases must be bytes or a one-dimensional uint8 array".format(module))
    offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
    if offsets.ndim != 1 or offsets.size < 1:
        raise ValueError("kmerdb_amd.{0}: offsets must hold nreads + 1 entries".format(module))
    if int(offsets[0]) != 0 or int(offsets[-1]) != bases.size or np.any(offsets[1:] < offsets[:-1]):
        raise ValueError("read_offsets must rise from 0 to nbytes")
    if bases.size > MAX_RESIDUES:
        raise ValueError("kmerdb_amd.{0}: at most 2^30 residues per call".format(module))
    return np.ascontiguousarray(bases), offsets
