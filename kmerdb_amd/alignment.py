"""Seed-and-extend alignment of reads to a reference: minimizer seeds, banded Smith-Waterman on the device (kdb_align_banded,
csrc/kdb_align.hip.h).

align_tasks is the device call on a batch of tasks: per task a query record, a reference record, the diagonal the band is centred on
and the query's strand -> the best local score with affine gaps inside the band and where that alignment begins and ends;
align_tasks_cigar (kdb_align_traceback, csrc/kdb_align_trace.hip.h) also gives the path between the two as
run-length encoded CIGAR runs, which cigar_string and cigar_nm turn into a SAM CIGAR and its NM.  seed_tasks
turns the minimizer sketches of the queries and of the reference (minimizer.minimizers, on the device) into such tasks, in plain numpy;
finish_tasks turns the call's output into per-query result lists; align_file does all of it for a reference and a query file, and
align_table prints its results (the `alignment` subcommand).  The reference's `alignment` (kmerdb/__init__.py:454-573) exits before it
aligns anything; its argument names and score defaults (match 3, mismatch -1, its commented-out gap pair -10 / -1) are kept, nothing
else is reproduced.  There is no CPU fallback: without a device these raise.
"""
import ctypes
import sys

import numpy as np

from . import _abi
from . import minimizer

MAX_BAND, MAX_QUERY = _abi.KDB_ALIGN_MAX_BAND, _abi.KDB_ALIGN_MAX_QUERY
_MAX_RESIDUES, _MAX_TASKS = 1 << 30, 1 << 26
BATCH_RESIDUES = 1 << 27                   # query residues per device call of align_file


def _int(name, v, lo, hi):
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
        raise TypeError("kmerdb_amd.alignment: {0} must be an int, not {1}".format(name, type(v).__name__))
    if not lo <= int(v) <= hi:
        raise ValueError("kmerdb_amd.alignment: {0}={1} out of range {2}..{3}".format(name, v, lo, hi))
    return int(v)


def _check_scores(band, match, mismatch, gap_open, gap_extend):
    return (_int("band", band, 1, MAX_BAND), _int("match", match, 1, 127), _int("mismatch", mismatch, -127, 0), _int("gap_open", gap_open, -127, 0),
            _int("gap_extend", gap_extend, -127, 0))


def _check_records(what, bases, offsets):
    if isinstance(bases, (bytes, bytearray, memoryview)):
        bases = np.frombuffer(bases, dtype=np.uint8)
    if not isinstance(bases, np.ndarray) or bases.dtype != np.uint8 or bases.ndim != 1:
        raise TypeError("kmerdb_amd.alignment: {0}_bases must be bytes or a one-dimensional uint8 array".format(what))
    offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
    if offsets.ndim != 1 or offsets.size < 1:
        raise ValueError("kmerdb_amd.alignment: {0}_offsets must hold one entry more than there are records".format(what))
    if int(offsets[0]) != 0 or int(offsets[-1]) != bases.size or np.any(offsets[1:] < offsets[:-1]):
        raise ValueError("kmerdb_amd.alignment: {0}_offsets must rise from 0 to the number of residues".format(what))
    if bases.size > _MAX_RESIDUES:
        raise ValueError("kmerdb_amd.alignment: at most 2^30 residues per buffer")
    return np.ascontiguousarray(bases), offsets


def _check_tasks(task_q, task_r, task_diag, task_strand, q_offsets, nr):
    def column(name, a, dtype, hi):
        a = np.asarray(a)
        if a.ndim == 1 and a.size == 0:
            a = a.astype(dtype)
        if a.ndim != 1 or a.dtype.kind not in "iu":
            raise TypeError("kmerdb_amd.alignment: {0} must be a one-dimensional array of integers".format(name))
        if hi is not None and a.size and (int(a.min()) < 0 or int(a.max()) >= hi):
            raise ValueError("kmerdb_amd.alignment: {0} holds an entry outside 0..{1}".format(name, hi - 1))
        return np.ascontiguousarray(a, dtype=dtype)
    nq = int(q_offsets.size) - 1
    task_q, task_r = column("task_q", task_q, np.uint32, nq), column("task_r", task_r, np.uint32, nr)
    task_diag, task_strand = column("task_diag", task_diag, np.int64, None), column("task_strand", task_strand, np.uint8, 2)
    if not task_q.size == task_r.size == task_diag.size == task_strand.size:
        raise ValueError("kmerdb_amd.alignment: task_q, task_r, task_diag and task_strand must be of one length")
    if task_q.size > _MAX_TASKS:
        raise ValueError("kmerdb_amd.alignment: at most 2^26 tasks per call")
    if task_q.size:
        lens = (q_offsets[1:] - q_offsets[:-1])[task_q]
        if int(lens.max()) > MAX_QUERY:
            raise ValueError("kmerdb_amd.alignment: a query record holds {0} residues, more than 2^20".format(int(lens.max())))
    return task_q, task_r, task_diag, task_strand


def align_raw(q_bases, q_offsets, r_bases, r_offsets, task_q, task_r, task_diag, task_strand, band, match, mismatch, gap_open, gap_extend, device=0):
    """kdb_align_banded on checked arguments -> (score: int32[t], qstart, qend, rstart, rend: uint32[t], kernel_ms)"""
    n = int(task_q.size)
    score = np.zeros(n, dtype=np.int32)
    qstart, qend, rstart, rend = (np.zeros(n, dtype=np.uint32) for _ in range(4))
    ms = ctypes.c_double(0.0)
    ptr = lambda a: a.ctypes.data if a.size else None
    _abi.check(_abi.lib().kdb_align_banded(int(device), ptr(q_bases), int(q_bases.size), q_offsets.ctypes.data, int(q_offsets.size) - 1, ptr(r_bases),
                                           int(r_bases.size), r_offsets.ctypes.data, int(r_offsets.size) - 1, ptr(task_q), ptr(task_r), ptr(task_diag),
                                           ptr(task_strand), n, band, match, mismatch, gap_open, gap_extend, ptr(score), ptr(qstart), ptr(qend), ptr(rstart),
                                           ptr(rend), ctypes.byref(ms)))
    return score, qstart, qend, rstart, rend, ms.value


def align_tasks(q_bases, q_offsets, r_bases, r_offsets, task_q, task_r, task_diag, task_strand, band=16, match=3, mismatch=-1, gap_open=-10, gap_extend=-1,
                device=0):
    """A batch of banded local alignments -> (score: int32[t], qstart, qend, rstart, rend: uint32[t]).

    Task t aligns query record task_q[t] -- as it is (task_strand 0) or reverse-complemented (1) -- to reference record task_r[t] inside
    the band |(j - i) - task_diag[t]| <= band, with affine gaps: a gap of g residues costs gap_open + (g - 1) gap_extend.  The alignment
    covers [qstart, qend) of the ORIENTED query and [rstart, rend) of the reference; a task without a positive score gives five zeros.
    The definition, tie rules included, is include/kdbhip.h's.  ValueError for what the call refuses: a residue outside upper-case ACGTN."""
    band, match, mismatch, gap_open, gap_extend = _check_scores(band, match, mismatch, gap_open, gap_extend)
    q_bases, q_offsets = _check_records("q", q_bases, q_offsets)
    r_bases, r_offsets = _check_records("r", r_bases, r_offsets)
    task_q, task_r, task_diag, task_strand = _check_tasks(task_q, task_r, task_diag, task_strand, q_offsets, int(r_offsets.size) - 1)
    from .distance import _require_device
    _require_device(device)
    return align_raw(q_bases, q_offsets, r_bases, r_offsets, task_q, task_r, task_diag, task_strand, band, match, mismatch, gap_open, gap_extend, device)[:5]


# ---- the traceback ----

OP_I, OP_D, OP_EQ, OP_X = 1, 2, 7, 8           # BAM's op codes; a run is (len << 4) | op
_OP_CHAR = {OP_I: "I", OP_D: "D", OP_EQ: "=", OP_X: "X"}
RUNS_GUESS = 16                                # runs per task the lists are sized for at the first call


def traceback_raw(q_bases, q_offsets, r_bases, r_offsets, task_q, task_r, task_diag, task_strand, band, match, mismatch, gap_open, gap_extend, cap, scratch_limit=0,
                  device=0):
    """kdb_align_traceback on checked arguments, the run list sized for `cap` runs -> (score, qstart, qend, rstart, rend, nruns: uint64[t],
    runs: uint32[total] or None where total > cap, total, kernel_ms)"""
    n = int(task_q.size)
    score = np.zeros(n, dtype=np.int32)
    qstart, qend, rstart, rend = (np.zeros(n, dtype=np.uint32) for _ in range(4))
    nruns, runs = np.zeros(n, dtype=np.uint64), np.empty(cap, dtype=np.uint32)
    total, ms = ctypes.c_uint64(0), ctypes.c_double(0.0)
    ptr = lambda a: a.ctypes.data if a.size else None
    _abi.check(_abi.lib().kdb_align_traceback(int(device), ptr(q_bases), int(q_bases.size), q_offsets.ctypes.data, int(q_offsets.size) - 1, ptr(r_bases),
                                              int(r_bases.size), r_offsets.ctypes.data, int(r_offsets.size) - 1, ptr(task_q), ptr(task_r), ptr(task_diag),
                                              ptr(task_strand), n, band, match, mismatch, gap_open, gap_extend, int(scratch_limit), ptr(score), ptr(qstart),
                                              ptr(qend), ptr(rstart), ptr(rend), ptr(nruns), ptr(runs), cap, ctypes.byref(total), ctypes.byref(ms)))
    t = int(total.value)
    return score, qstart, qend, rstart, rend, nruns, (runs[:t] if t <= cap else None), t, ms.value


def _traceback(args, cap, scratch_limit, device):
    """size, then fill: the lists sized for `cap` runs, and once more with the total where that is not enough -> traceback_raw's tuple"""
    out = traceback_raw(*args, cap, scratch_limit, device)
    if out[6] is None:
        first = out[7]
        out = traceback_raw(*args, first, scratch_limit, device)
        if out[6] is None:
            raise _abi.KdbHipError("kdb_align_traceback: two calls on one batch found {0} and {1} runs".format(first, out[7]))
    return out


def align_tasks_cigar(q_bases, q_offsets, r_bases, r_offsets, task_q, task_r, task_diag, task_strand, band=16, match=3, mismatch=-1, gap_open=-10, gap_extend=-1,
                      device=0, scratch_limit=None):
    """align_tasks with the alignments' paths -> (score, qstart, qend, rstart, rend, nruns: uint64[t], runs: uint32[sum of nruns]).

    The five first are align_tasks' own.  Task t's runs are runs[S_t : S_t + nruns[t]], S the exclusive prefix sums of nruns, from the
    alignment's origin to its end: a run is (len << 4) | op with BAM's op codes I = 1 (a query residue against a gap), D = 2 (a reference
    residue against one), `=` = 7 and X = 8.  The walk that gives them is include/kdbhip.h's.  scratch_limit: the bytes of direction
    scratch per chunk of tasks (None: KDB_ALIGN_TRACE_SCRATCH); the result does not depend on it."""
    band, match, mismatch, gap_open, gap_extend = _check_scores(band, match, mismatch, gap_open, gap_extend)
    q_bases, q_offsets = _check_records("q", q_bases, q_offsets)
    r_bases, r_offsets = _check_records("r", r_bases, r_offsets)
    task_q, task_r, task_diag, task_strand = _check_tasks(task_q, task_r, task_diag, task_strand, q_offsets, int(r_offsets.size) - 1)
    scratch_limit = 0 if scratch_limit is None else _int("scratch_limit", scratch_limit, 1, (1 << 63) - 1)
    from .distance import _require_device
    _require_device(device)
    args = (q_bases, q_offsets, r_bases, r_offsets, task_q, task_r, task_diag, task_strand, band, match, mismatch, gap_open, gap_extend)
    return _traceback(args, RUNS_GUESS * int(task_q.size), scratch_limit, device)[:7]


def cigar_string(runs, qstart, qend, m, eqx=False):
    """A task's runs as a SAM CIGAR of its oriented query of m residues: qstart S first and m - qend S last (none of length 0); eqx: `=`
    and X as they are, else merged into M."""
    ops = []
    if qstart:
        ops.append([int(qstart), "S"])
    for run in np.asarray(runs).tolist():
        ch = _OP_CHAR[run & 15]
        if not eqx and ch in "=X":
            ch = "M"
        if ops and ops[-1][1] == ch and ch != "S":
            ops[-1][0] += run >> 4
        else:
            ops.append([run >> 4, ch])
    if m - qend:
        ops.append([int(m - qend), "S"])
    return "".join("{0}{1}".format(n, ch) for n, ch in ops)


def cigar_nm(runs):
    """the edit distance of the aligned part: the lengths of the X, I and D runs"""
    return sum(run >> 4 for run in np.asarray(runs).tolist() if run & 15 in (OP_X, OP_I, OP_D))


# ---- seeding: plain numpy on the two sketches ----

def _check_seeding(k, w, order, min_seeds, max_occ, max_candidates, min_score):
    k, w, _ = minimizer._check_scalars(k, w, order)
    return (k, w, _int("min_seeds", min_seeds, 1, 1 << 30), _int("max_occ", max_occ, 1, 1 << 30), _int("max_candidates", max_candidates, 1, 1 << 20),
            _int("min_score", min_score, 0, 1 << 27))


def _record_of(counts):
    return np.repeat(np.arange(counts.size, dtype=np.int64), counts.astype(np.int64))


def build_sketch(counts, ids, pos, strand, max_occ):
    """The reference sketch: every reference record's minimizers, stably sorted by id (so by (id, record, position)), without the ids that
    occur more than max_occ times -> (ids: uint64[s], ref: int64[s], pos: int64[s], strand: uint8[s])"""
    ref = _record_of(counts)
    order = np.argsort(ids, kind="stable")
    ids, ref, pos, strand = ids[order], ref[order], pos[order].astype(np.int64), strand[order]
    if ids.size:
        first = np.flatnonzero(np.concatenate(([True], ids[1:] != ids[:-1])))
        occ = np.diff(np.concatenate((first, [ids.size])))
        keep = np.repeat(occ <= max_occ, occ)
        ids, ref, pos, strand = ids[keep], ref[keep], pos[keep], strand[keep]
    return ids, ref, pos, strand


def seed_tasks(sketch, q_lens, q_counts, q_ids, q_pos, q_strand, k, band, min_seeds=2, max_candidates=4):
    """The candidates of a batch of queries -> (task_q: uint32[t], task_r: uint32[t], task_diag: int64[t], task_strand: uint8[t],
    seeds: int64[t]), by query and, inside a query, by rank: the most hits first, ties to the smaller (ref, rel, bin).

    Every equal id between a query minimizer and a sketch entry is a hit: rel = the two strands' XOR, the oriented query position is qpos
    (rel 0) or m - k - qpos (rel 1), diag = rpos - that.  The hits are grouped by (query, ref, rel, floor(diag / (band + 1))); a group of at
    least min_seeds hits is a candidate, a query keeps its max_candidates best, and a candidate's diagonal is the lower median of its hits'
    diagonals: every hit of the group then lies inside the band."""
    s_ids, s_ref, s_pos, s_strand = sketch
    empty = (np.zeros(0, dtype=np.uint32), np.zeros(0, dtype=np.uint32), np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.uint8), np.zeros(0, dtype=np.int64))
    if q_ids.size == 0 or s_ids.size == 0:
        return empty
    lo, hi = np.searchsorted(s_ids, q_ids, side="left"), np.searchsorted(s_ids, q_ids, side="right")
    n = (hi - lo).astype(np.int64)
    total = int(n.sum())
    if total == 0:
        return empty
    of = np.repeat(np.arange(q_ids.size, dtype=np.int64), n)                  # the query minimizer of every hit
    at = np.arange(total, dtype=np.int64) - np.repeat(np.cumsum(n) - n, n) + np.repeat(lo.astype(np.int64), n)    # ... and its sketch entry
    query = _record_of(q_counts)[of]
    m = np.asarray(q_lens, dtype=np.int64)[query]
    rel = (q_strand[of] ^ s_strand[at]).astype(np.int64)
    qp = q_pos[of].astype(np.int64)
    diag = s_pos[at] - np.where(rel == 0, qp, m - k - qp)
    ref = s_ref[at]
    bins = np.floor_divide(diag, band + 1)
    order = np.lexsort((diag, bins, rel, ref, query))                         # (the last key is the first: by query, ref, rel, bin, diag)
    query, ref, rel, bins, diag = query[order], ref[order], rel[order], bins[order], diag[order]
    new = np.concatenate(([True], (query[1:] != query[:-1]) | (ref[1:] != ref[:-1]) | (rel[1:] != rel[:-1]) | (bins[1:] != bins[:-1])))
    first = np.flatnonzero(new)
    hits = np.diff(np.concatenate((first, [total])))
    median = diag[first + (hits - 1) // 2]                                    # (the group's diagonals ascend: the lower median)
    g_query, g_ref, g_rel, g_bin = query[first], ref[first], rel[first], bins[first]
    keep = hits >= min_seeds
    g_query, g_ref, g_rel, g_bin, hits, median = g_query[keep], g_ref[keep], g_rel[keep], g_bin[keep], hits[keep], median[keep]
    rank = np.lexsort((g_bin, g_rel, g_ref, -hits, g_query))
    g_query, g_ref, g_rel, hits, median = g_query[rank], g_ref[rank], g_rel[rank], hits[rank], median[rank]
    if g_query.size == 0:
        return empty
    start = np.flatnonzero(np.concatenate(([True], g_query[1:] != g_query[:-1])))
    place = np.arange(g_query.size, dtype=np.int64) - np.repeat(start, np.diff(np.concatenate((start, [g_query.size]))))
    top = place < max_candidates
    return g_query[top].astype(np.uint32), g_ref[top].astype(np.uint32), median[top], g_rel[top].astype(np.uint8), hits[top]


def finish_tasks(nq, q_lens, tasks, out, min_score=0, with_task=False):
    """The results of every query, from its tasks (by query and rank, as seed_tasks gives them) and the device's output for them
    -> a list per query of (qstart, qend, rel, ref, rstart, rend, score, seeds, diag), query coordinates on the query's own strand.
    Without the tasks that found nothing or less than min_score and without a result that repeats a better-ranked one of its query in
    (ref, rel, all four coordinates); by (-score, ref, rel, rstart).  with_task: every result has the index of its task behind it."""
    task_q, task_r, task_diag, task_strand, seeds = tasks
    score, qstart, qend, rstart, rend = out
    results = [[] for _ in range(nq)]
    for t in np.flatnonzero((score > 0) & (score >= min_score)).tolist():
        q, rel, m = int(task_q[t]), int(task_strand[t]), int(q_lens[task_q[t]])
        a, b = int(qstart[t]), int(qend[t])
        if rel:
            a, b = m - b, m - a
        found = (a, b, rel, int(task_r[t]), int(rstart[t]), int(rend[t]), int(score[t]), int(seeds[t]), int(task_diag[t]))
        if not any(x[:6] == found[:6] for x in results[q]):                    # (the tasks come by rank: the better-ranked one is there already)
            results[q].append(found + (t,) if with_task else found)
    for found in results:
        found.sort(key=lambda x: (-x[6], x[3], x[2], x[4]))                   # (stable: of equal keys the better-ranked stays first)
    return results


def _sketch_of(bases, offsets, k, w, order, device):
    return minimizer.minimizers(bases, offsets, k, w, canonical=True, order=order, device=device)


def align_records(sketch, r_bases, r_offsets, q_bases, q_offsets, k, w, order, band, match, mismatch, gap_open, gap_extend, min_seeds, max_candidates, min_score,
                  device=0, times=None, cigar=False, eqx=False):
    """one batch of queries against a built sketch -> finish_tasks' lists.  times: a dict that collects the seconds of each part.
    cigar: the device call is the traceback's, and every result has its CIGAR string -- along the oriented query, as SAM has it -- and its
    NM behind it"""
    import time
    t0 = time.perf_counter()
    q_lens = np.diff(q_offsets.astype(np.int64))
    if q_lens.size and int(q_lens.max()) > MAX_QUERY:
        raise ValueError("kmerdb_amd.alignment: query record {0} holds {1} residues, more than 2^20: the banded alignment takes queries of at most "
                         "2^20".format(int(np.argmax(q_lens)), int(q_lens.max())))
    q_counts, q_ids, q_pos, q_strand = _sketch_of(q_bases, q_offsets, k, w, order, device)
    t1 = time.perf_counter()
    tasks = seed_tasks(sketch, q_lens, q_counts, q_ids, q_pos, q_strand, k, band, min_seeds, max_candidates)
    t2 = time.perf_counter()
    args = (q_bases, q_offsets, r_bases, r_offsets, tasks[0], tasks[1], tasks[2], tasks[3], band, match, mismatch, gap_open, gap_extend)
    if cigar:
        traced = _traceback(args, RUNS_GUESS * int(tasks[0].size), 0, device)
        out = traced[:5] + (traced[8],)
    else:
        out = align_raw(*args, device)
    t3 = time.perf_counter()
    results = finish_tasks(int(q_lens.size), q_lens, tasks, out[:5], min_score, with_task=cigar)
    if cigar:
        nruns, runs = traced[5].astype(np.int64), traced[6]
        ends = np.cumsum(nruns)
        for q, found in enumerate(results):
            for x, result in enumerate(found):
                t = result[-1]
                mine = runs[int(ends[t] - nruns[t]):int(ends[t])]
                found[x] = result[:-1] + (cigar_string(mine, int(out[1][t]), int(out[2][t]), int(q_lens[q]), eqx), cigar_nm(mine))
    t4 = time.perf_counter()
    if times is not None:
        for name, dt in (("sketching", t1 - t0), ("seeding", t2 - t1 + t4 - t3), ("device", t3 - t2)):
            times[name] = times.get(name, 0.0) + dt
        times["kernel_ms"] = times.get("kernel_ms", 0.0) + out[5]
        times["tasks"] = times.get("tasks", 0) + int(tasks[0].size)
    return results


def align_file(reference, query, k=15, w=10, order="hashed", band=16, match=3, mismatch=-1, gap_open=-10, gap_extend=-1, min_seeds=2, max_occ=50,
               max_candidates=4, min_score=0, best_only=False, device=0, batch_residues=None, times=None, cigar=False, eqx=False):
    """Every query record of a FASTA/FASTQ file against the records of a reference FASTA: yields, per query in file order and per result
    by (-score, ref, rel, rstart), (qname, qlen, qstart, qend, strand, rname, rlen, rstart, rend, score, seeds, diag) -- the alignment
    covers [qstart, qend) of the query as the file has it and [rstart, rend) of the reference record; strand 1: the query's reverse
    complement is what aligns; seeds: the minimizer hits of the candidate, diag: the diagonal its band was centred on.  best_only: the
    first result of every query alone.  The reference is read whole, the query in batches.  cigar: two more fields, the alignment's
    CIGAR (soft clips included; strand 1: along the reverse-complemented query, as SAM has it; eqx: `=` and X, not M) and its NM."""
    from . import reader
    if type(reference) is not str or type(query) is not str:
        raise TypeError("kmerdb_amd.alignment.align_file expects the reference and the query file as str filepaths")
    band, match, mismatch, gap_open, gap_extend = _check_scores(band, match, mismatch, gap_open, gap_extend)
    k, w, min_seeds, max_occ, max_candidates, min_score = _check_seeding(k, w, order, min_seeds, max_occ, max_candidates, min_score)
    batch_residues = _int("batch_residues", BATCH_RESIDUES if batch_residues is None else batch_residues, 1, _MAX_RESIDUES)
    import time
    t0 = time.perf_counter()
    r_bases, r_offsets, r_names = [], [np.zeros(1, dtype=np.uint64)], []
    for bases, offsets, ids in reader.BlockReader(reference, want_ids=True):
        offsets = np.asarray(offsets, dtype=np.uint64)
        r_offsets.append(offsets[1:] + r_offsets[-1][-1])
        r_bases.append(np.array(bases, dtype=np.uint8))
        r_names += [str(x) for x in ids]
    r_bases, r_offsets = np.concatenate(r_bases) if r_bases else np.zeros(0, dtype=np.uint8), np.concatenate(r_offsets)
    if r_bases.size > _MAX_RESIDUES:
        raise ValueError("kmerdb_amd.alignment: the reference holds more than 2^30 residues")
    r_lens = np.diff(r_offsets.astype(np.int64))
    sketch = build_sketch(*_sketch_of(r_bases, r_offsets, k, w, order, device), max_occ)
    if times is not None:
        times["sketching"] = times.get("sketching", 0.0) + time.perf_counter() - t0
    for bases, offsets, ids in reader.BlockReader(query, want_ids=True):
        offsets = np.asarray(offsets, dtype=np.int64)
        nrec, a = int(offsets.size) - 1, 0
        while a < nrec:                                                       # the records [a, b): whole records, batch_residues of them or one
            b = max(a + 1, int(np.searchsorted(offsets, offsets[a] + batch_residues, side="right")) - 1)
            q_bases = np.ascontiguousarray(bases[int(offsets[a]):int(offsets[b])])
            q_offsets = (offsets[a:b + 1] - offsets[a]).astype(np.uint64)
            results = align_records(sketch, r_bases, r_offsets, q_bases, q_offsets, k, w, order, band, match, mismatch, gap_open, gap_extend, min_seeds,
                                    max_candidates, min_score, device, times, cigar, eqx)
            for q, found in enumerate(results):
                qname, qlen = str(ids[a + q]), int(offsets[a + q + 1] - offsets[a + q])
                for qstart, qend, rel, ref, rstart, rend, score, seeds, diag, *path in (found[:1] if best_only else found):
                    yield (qname, qlen, qstart, qend, rel, r_names[ref], int(r_lens[ref]), rstart, rend, score, seeds, diag, *path)
            a = b


def format_line(result):
    """a result of align_file as the `alignment` subcommand prints it: tab-separated, the strand as + or -"""
    return "\t".join(str(x) if i != 4 else ("-" if x else "+") for i, x in enumerate(result)) + "\n"


def align_table(reference, query, out=None, **kw):
    """The `alignment` subcommand: one line per result of align_file, nothing for a query without one -> the number of lines."""
    out = sys.stdout if out is None else out
    n = 0
    for result in align_file(reference, query, **kw):
        out.write(format_line(result))
        n += 1
    return n
