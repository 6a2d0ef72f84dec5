"""Device time of kdb_align_banded (csrc/kdb_align.hip.h) and the wall time of kmerdb_amd.alignment.align_file:
  short    1 M tasks: reads of 150 bp with 2 % substitutions, both strands, against a 5-Mbp record, band 16
  long     10 k tasks: queries of 10 kbp with 2 % substitutions against the same record, band 63
  file     align_file on that record and the 1 M reads as FASTA files (k = 15, w = 10, hashed, band 16), split into sketching (both
           sketches, device calls included), host seeding (numpy: the join of the sketches, the candidates, the results), the device call
           and the rest (reading, formatting and writing the lines)
The kernel time is kernel_ms_out, median (min-max) over --reps passes after --warmup; cells = the sum over the tasks of m (2 band + 1).
The parent commit has no alignment: the yardstick is the numpy restatement of tests/alignment_cases.py on a sample of the same tasks,
whose outputs must equal the call's, scaled to all of them.
    python tools/bench_alignment.py [--short 1000000] [--long 10000] [--reads 1000000] [--reps 5] [--warmup 2] [--json out.json] [--traceback]
  --traceback   instead: kdb_align_traceback (csrc/kdb_align_trace.hip.h) on the short and the long workload, its passes alternating with
           kdb_align_banded's on the same tasks in the same process -- both kernel times, their ratio, the bytes of direction scratch and
           the chunks, runs per second, and whether the five scalars equal kdb_align_banded's and the runs of a sample the restatement's
           of tests/traceback_cases.py
No GPU, no number: this tool has no fallback."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

LETTERS = np.frombuffer(b"ACGT", dtype=np.uint8)
COMP = np.zeros(256, dtype=np.uint8)
for _a, _b in zip(b"ACGT", b"TGCA"):
    COMP[_a] = _b


def med_range(xs):
    return "%.2f (%.2f-%.2f)" % (statistics.median(xs), min(xs), max(xs))


def cut_reads(rng, ref, n, length, p_sub=0.02):
    """n reads of `length` residues cut from ref, with substitutions, every second one reverse-complemented
    -> (bases, offsets, start: int64[n], strand: uint8[n])"""
    start = rng.integers(0, ref.size - length, size=n)
    reads = np.empty((n, length), dtype=np.uint8)
    step = max(1, (1 << 24) // length)
    for a in range(0, n, step):                                               # (in pieces: the index array of all the reads at once is 8 bytes per residue)
        part = ref[start[a:a + step, None] + np.arange(length)[None, :]]
        sub = rng.random(part.shape) < p_sub
        part[sub] = LETTERS[rng.integers(0, 4, size=int(sub.sum()))]
        reads[a:a + step] = part
    strand = (np.arange(n) & 1).astype(np.uint8)
    reads[1::2] = COMP[reads[1::2, ::-1]]
    return np.ascontiguousarray(reads.reshape(-1)), (np.arange(n + 1, dtype=np.uint64) * np.uint64(length)), start.astype(np.int64), strand


def write_fasta(path, bases, length, prefix):
    n = bases.size // length
    rows = bases.reshape(n, length)
    with open(path, "wb") as f:
        for a in range(0, n, 100000):
            f.write(b"".join(b">%s%d\n%s\n" % (prefix, i, rows[i].tobytes()) for i in range(a, min(n, a + 100000))))


def trace_plan(starts, m, n, band, limit):
    """the direction scratch of the tasks (an oriented query of m residues on the diagonal starts[t] of a record of n) and the chunks of
    consecutive tasks a limit cuts them into, as kdbplan::align_trace_bytes / align_trace_chunks have them -> (bytes, chunks)"""
    jb = starts - band
    i_lo, i_hi = np.maximum(0, -jb - 2 * band), np.minimum(m, n - jb)
    task_bytes = np.where(i_lo < i_hi, 256 * ((i_hi + band - (i_lo // 4) * 4 + 3) // 4), 0)
    chunks, used = 1, 0
    for b in task_bytes.tolist():
        if used and (used > limit or b > limit - used):
            chunks, used = chunks + 1, 0
        used += b
    return int(task_bytes.sum()), chunks


def bench_traceback(a, rng, ref, r_offsets, scores, out):
    from kmerdb_amd import _abi, alignment
    import traceback_cases as tc
    for name, ntasks, length, band in (("short", a.short, 150, 16), ("long", a.long, 10000, 63)):
        if ntasks == 0:
            continue
        bases, offsets, start, strand = cut_reads(rng, ref, ntasks, length)
        tq, tr = np.arange(ntasks, dtype=np.uint32), np.zeros(ntasks, dtype=np.uint32)
        args = (bases, offsets, ref, r_offsets, tq, tr, start, strand, band, scores["match"], scores["mismatch"], scores["gap_open"], scores["gap_extend"])
        total = alignment.traceback_raw(*args, 0)[7]                          # the sizes alone
        banded, traced = [], []
        for rep in range(a.warmup + a.reps):                                  # the two calls alternate
            plain = alignment.align_raw(*args)
            got = alignment.traceback_raw(*args, total)
            if rep >= a.warmup:
                banded.append(plain[5])
                traced.append(got[8])
        same = all(np.array_equal(g, x) for g, x in zip(got[:5], plain[:5])) and got[7] == total == int(got[5].sum())
        rows, ends = bases.reshape(ntasks, length), np.cumsum(got[5].astype(np.int64))
        sample = min(a.sample, 200)                                           # (the restatement walks cell by cell)
        pick = np.arange(0, ntasks, max(1, ntasks // sample))[:sample] if name == "short" else np.array([0])
        for t in pick.tolist():
            lo = max(0, int(start[t]) - 2 * band)                             # (the piece of the record the band can reach, and the diagonal inside it)
            five, path = tc.trace(rows[t].tobytes(), ref[lo:int(start[t]) + length + 2 * band].tobytes(), int(start[t]) - lo, band, int(strand[t]), **scores)
            five = five[:3] + (five[3] + lo, five[4] + lo) if five[0] else five
            same = same and five == tuple(int(g[t]) for g in got[:5]) and path == got[6][int(ends[t] - got[5][t]):int(ends[t])].tolist()
        nbytes, chunks = trace_plan(start, length, ref.size, band, _abi.KDB_ALIGN_TRACE_SCRATCH)
        kb, kt = statistics.median(banded), statistics.median(traced)
        run = {"workload": name + "_traceback", "tasks": ntasks, "query": length, "band": band, "banded_kernel_ms": banded, "traceback_kernel_ms": traced,
               "traceback_over_banded": kt / kb, "direction_bytes": nbytes, "chunks": chunks, "runs": total, "runs_per_s": total / kt * 1e3,
               "restatement_sample": int(pick.size), "same_outputs": bool(same)}
        out["runs"].append(run)
        print("%-5s %8d tasks of %5d bp, band %2d: kdb_align_banded kernel %s ms; kdb_align_traceback kernels %s ms = %.2f x; %.2f GB of directions in %d chunk(s); "
              "%d runs = %.1f M runs/s; scalars equal kdb_align_banded's and the runs of %d tasks the restatement's: %s"
              % (name, ntasks, length, band, med_range(banded), med_range(traced), kt / kb, nbytes / 1e9, chunks, total, total / kt / 1e3, pick.size, same), flush=True)
        del bases, got, plain


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", type=int, default=5_000_000)
    ap.add_argument("--short", type=int, default=1_000_000)
    ap.add_argument("--long", type=int, default=10_000)
    ap.add_argument("--reads", type=int, default=1_000_000, help="reads of the align_file run (0: leave it out)")
    ap.add_argument("--sample", type=int, default=2000, help="short tasks the numpy restatement takes (of the long ones: 2)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--json", default=None)
    ap.add_argument("--traceback", action="store_true", help="kdb_align_traceback beside kdb_align_banded on the short and the long workload, nothing else")
    a = ap.parse_args()
    import kmerdb_amd
    from kmerdb_amd import _abi, alignment
    import alignment_cases as ac
    _abi.lib()
    if kmerdb_amd.device_count() < 1:
        raise SystemExit("no HIP device: nothing is measured")
    rng = np.random.Generator(np.random.PCG64(2026))
    ref = LETTERS[rng.integers(0, 4, size=a.reference)]
    r_offsets = np.array([0, ref.size], dtype=np.uint64)
    out = {"reference": a.reference, "reps": a.reps, "warmup": a.warmup, "stage": _abi.KDB_ALIGN_STAGE, "runs": []}
    scores = dict(match=3, mismatch=-1, gap_open=-10, gap_extend=-1)
    if a.traceback:
        bench_traceback(a, rng, ref, r_offsets, scores, out)
        a.short = a.long = a.reads = 0

    for name, ntasks, length, band in (("short", a.short, 150, 16), ("long", a.long, 10000, 63)):
        if ntasks == 0:
            continue
        bases, offsets, start, strand = cut_reads(rng, ref, ntasks, length)
        tq, tr = np.arange(ntasks, dtype=np.uint32), np.zeros(ntasks, dtype=np.uint32)
        kernel, wall = [], []
        for rep in range(a.warmup + a.reps):
            t0 = time.perf_counter()
            got = alignment.align_raw(bases, offsets, ref, r_offsets, tq, tr, start, strand, band, scores["match"], scores["mismatch"], scores["gap_open"],
                                      scores["gap_extend"])
            if rep >= a.warmup:
                kernel.append(got[5])
                wall.append(1e3 * (time.perf_counter() - t0))
        cells = ntasks * length * (2 * band + 1)
        # the restatement on a sample: the same outputs, and what all the tasks would take at that rate
        t0 = time.perf_counter()
        if name == "short":
            pick = np.arange(0, ntasks, max(1, ntasks // a.sample))[:a.sample]
            want = ac.banded_batch(bases, offsets, ref, r_offsets, tq[pick], tr[pick], start[pick], strand[pick], band, **scores)
        else:
            pick = np.array([0, ntasks - 1] if ntasks > 1 else [0])
            rows = bases.reshape(ntasks, length)
            want = ac.run_tasks([rows[i].tobytes() for i in pick], [ref.tobytes()], [(x, 0, int(start[i]), int(strand[i])) for x, i in enumerate(pick)], band, **scores)
        host = 1e3 * (time.perf_counter() - t0) * ntasks / pick.size
        same = all(np.array_equal(g[pick], x) for g, x in zip(got[:5], want))
        k = statistics.median(kernel)
        run = {"workload": name, "tasks": ntasks, "query": length, "band": band, "cells": cells, "kernel_ms": kernel, "call_ms": wall, "Gcells_per_s": cells / k / 1e6,
               "mean_score": float(got[0].mean()), "restatement_sample": int(pick.size), "restatement_scaled_ms": host, "restatement_over_kernel": host / k,
               "restatement_over_call": host / statistics.median(wall), "same_outputs": bool(same)}
        out["runs"].append(run)
        print("%-5s %8d tasks of %5d bp, band %2d: kernel %s ms = %.1f G cell updates/s; call %s ms; mean score %.1f; numpy restatement on %d tasks, scaled: %.0f ms = "
              "%.0f x the kernel, %.0f x the call; same outputs: %s" % (name, ntasks, length, band, med_range(kernel), run["Gcells_per_s"], med_range(wall),
                                                                       run["mean_score"], pick.size, host, host / k, run["restatement_over_call"], same), flush=True)
        del bases, got

    if a.reads:
        bases, offsets, start, strand = cut_reads(rng, ref, a.reads, 150)
        with tempfile.TemporaryDirectory() as where:
            rpath, qpath, opath = os.path.join(where, "reference.fa"), os.path.join(where, "reads.fa"), os.path.join(where, "out.tsv")
            with open(rpath, "wb") as f:
                f.write(b">reference\n")
                f.write(b"\n".join(ref[i:i + 70].tobytes() for i in range(0, ref.size, 70)) + b"\n")
            write_fasta(qpath, bases, 150, b"read")
            print("file  %d reads written" % a.reads, flush=True)
            times = {}
            t0 = time.perf_counter()
            with open(opath, "w") as f:
                lines = alignment.align_table(rpath, qpath, out=f, k=15, w=10, order="hashed", band=16, times=times)
            wall = time.perf_counter() - t0
        rest = wall - times["sketching"] - times["seeding"] - times["device"]
        run = {"workload": "file", "reads": a.reads, "lines": lines, "tasks": times["tasks"], "wall_s": wall, "sketching_s": times["sketching"], "seeding_s": times["seeding"],
               "device_s": times["device"], "kernel_ms": times["kernel_ms"], "read_and_write_s": rest, "seeding_share": times["seeding"] / wall}
        out["runs"].append(run)
        print("file  %d reads of 150 bp against %d bp: %d tasks, %d lines; wall %.1f s = sketching %.1f + host seeding %.1f (%.0f %%) + device call %.2f (kernel %.1f ms) "
              "+ reading, formatting, writing %.1f" % (a.reads, a.reference, times["tasks"], lines, wall, times["sketching"], times["seeding"], 100 * run["seeding_share"],
                                                       times["device"], times["kernel_ms"], rest), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
