"""Device and call time of kdb_minimizers (csrc/kdb_minimizers.hip.h) on three workloads:
  reads    10 M reads of 150 bp, k = 15, w = 10, canonical, hashed order
  genome   one record of 100 Mbp, k = 19, w = 19, canonical, lexicographic order
  polya    one poly-A record of 100 Mbp, k = 15, w = 10: every position but the last w - 1 is selected, the densest output
next to two yardsticks from the same process on the same device:
  * what the engine allowed before for the same lists: kdb_window_ids (8 bytes per residue back to the host), then a sliding minimum
    in numpy, on the records of one call, at k = 15 (that path stops at k = 17) and the workload's w and order; its lists must equal
    the call's bit for bit;
  * the streamed rates of kdb_hbm_pattern_probe, against the bytes each kernel reads and writes by the piece layout.
    python tools/bench_minimizers.py [--records 10000000] [--call-records 1000000] [--genome 100000000] [--reps 5] [--warmup 2] [--json out.json]
A call takes at most 2^30 residues, so the reads go through in calls of --call-records and the times of the calls are added; the calls
of a pass take the same --call-records synthetic records.  "select" is kernel_ms_out of a call that asks for the sizes alone (cap = 0:
keys, selection, the scan, the records' counts), "kernel" that of a full call (the emit pass too).  "call" is the host clock around the
full call: upload of the residues and offsets, scratch, kernels, the lists back into host buffers that are reused.  No GPU, no number:
this tool has no fallback."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

NONE = np.uint64(2 ** 64 - 1)


def med_range(xs):
    return "%.2f (%.2f-%.2f)" % (statistics.median(xs), min(xs), max(xs))


def mix(x, k):
    """the invertible mix of KDB_MINIMIZER_HASHED on a uint64 array"""
    m, u = np.uint64(4 ** k - 1), np.uint64
    with np.errstate(over="ignore"):
        x = (~x + (x << u(21))) & m
        x ^= x >> u(24)
        x = (x + (x << u(3)) + (x << u(8))) & m
        x ^= x >> u(14)
        x = (x + (x << u(2)) + (x << u(4))) & m
        x ^= x >> u(28)
        x = (x + (x << u(31))) & m
    return x


def host_minimizers(ids_engine, bases, offsets, k, w, hashed, length, block=1 << 24):
    """the same lists from kdb_window_ids and numpy, for records of one length: the leftmost minimum of every run of w keys, `block`
    runs at a time -> (counts, ids, pos)"""
    n, nwin = offsets.size - 1, length - k + 1
    ids = ids_engine.window_ids(bases, offsets).reshape(n, length)[:, :nwin]
    we = min(w, nwin)
    nruns = nwin - we + 1
    chosen = np.zeros((n, nwin), dtype=bool)
    rows_per = max(1, block // nruns)
    for r0 in range(0, n, rows_per):
        for c0 in range(0, nruns, block):
            c1 = min(nruns, c0 + block)
            part = ids[r0:r0 + rows_per, c0:c1 + we - 1]
            keys = np.where(part != NONE, mix(part, k), NONE) if hashed else part
            runs = np.lib.stride_tricks.sliding_window_view(keys, we, axis=1)
            p = runs.argmin(axis=2) + np.arange(c1 - c0)[None, :]            # (argmin: the first of equal keys)
            finite = np.take_along_axis(keys, p, axis=1) != NONE
            rows = np.broadcast_to(np.arange(part.shape[0])[:, None], p.shape)
            chosen[r0:r0 + rows_per, c0:c1 + we - 1][rows[finite], p[finite]] = True
    rec, pos = np.nonzero(chosen)
    return np.bincount(rec, minlength=n).astype(np.uint64), ids[rec, pos], pos.astype(np.uint32)


def plan_bytes(nrec, length, k, w, piece, total):
    """bytes read and written by the select and the emit kernel, by the piece layout (records of one length)"""
    nwin = max(0, length - k + 1)
    npieces = max(1, -(-nwin // piece))
    staged = 0
    for p in range(npieces):
        first = p * piece
        count = min(piece, nwin - first)
        lo, hi = max(0, first - (w - 1)), min(nwin, first + count + w - 1)
        staged += -(-(hi - lo + k - 1 + 3) // 4) * 4 if count else 0
    return {"select_read": nrec * (staged + 16 + 8 * npieces), "select_write": nrec * (nwin + 4 * npieces),
            "emit_read": nrec * (nwin + 8 * npieces + 8) + total * k, "emit_write": total * 13}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=10_000_000)
    ap.add_argument("--call-records", type=int, default=1_000_000)
    ap.add_argument("--genome", type=int, default=100_000_000)
    ap.add_argument("--workloads", default="reads,genome,polya")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-host", action="store_true", help="leave out the kdb_window_ids + numpy comparison")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    import kmerdb_amd
    from kmerdb_amd import _abi, synth
    from kmerdb_amd.engine import IdsEngine
    lib = _abi.lib()
    if kmerdb_amd.device_count() < 1:
        raise SystemExit("no HIP device: nothing is measured")
    out = {"records": a.records, "call_records": a.call_records, "genome": a.genome, "reps": a.reps, "warmup": a.warmup, "piece": _abi.KDB_MINIMIZER_PIECE, "runs": []}

    n = lib.kdb_hbm_pattern_count()
    rates = (ctypes.c_double * n)()
    _abi.check(lib.kdb_hbm_pattern_probe(0, rates, n))
    out["pattern_GBps"] = {lib.kdb_hbm_pattern_name(i).decode(): rates[i] for i in range(n)}
    stream_read, stream_write = out["pattern_GBps"]["stream_read"], out["pattern_GBps"]["stream_write"]
    print("pattern stream_write %8.1f GB/s, stream_read %8.1f GB/s" % (stream_write, stream_read))

    HOST_K = 15
    shapes = {"reads": (150, 15, 10, True), "genome": (a.genome, 19, 19, False), "polya": (a.genome, 15, 10, False)}
    for name in a.workloads.split(","):
        length, k, w, hashed = shapes[name]
        nrec = 1 if name != "reads" else min(a.call_records, a.records)
        ncalls = 1 if name != "reads" else -(-a.records // nrec)
        if name == "polya":
            bases, offsets = np.full(length, ord("A"), dtype=np.uint8), np.array([0, length], dtype=np.uint64)
        else:
            bases, offsets = synth.reads(nrec, length, seed=synth.SEED0 + k)
        bases, offsets = np.ascontiguousarray(bases, dtype=np.uint8), np.ascontiguousarray(offsets, dtype=np.uint64)
        counts = np.zeros(nrec, dtype=np.uint64)
        total, ms = ctypes.c_uint64(0), ctypes.c_double(0.0)

        def call(kk, cap, ids, pos, strand):
            _abi.check(lib.kdb_minimizers(0, kk, w, 1, 1 if hashed else 0, bases.ctypes.data, bases.size, offsets.ctypes.data, nrec, counts.ctypes.data,
                                          ids.ctypes.data if cap else None, pos.ctypes.data if cap else None, strand.ctypes.data if cap else None, cap,
                                          ctypes.byref(total), ctypes.byref(ms)))
            return ms.value

        empty = np.zeros(0, dtype=np.uint8)
        call(k, 0, empty, empty, empty)
        cap = int(total.value)
        ids, pos, strand = np.zeros(cap, dtype=np.uint64), np.zeros(cap, dtype=np.uint32), np.zeros(cap, dtype=np.uint8)   # (touched once)
        select, kernel, wall = [], [], []
        for rep in range(a.warmup + a.reps):
            sms = sum(call(k, 0, empty, empty, empty) for _ in range(ncalls))
            t0, kms = time.perf_counter(), 0.0
            for _ in range(ncalls):
                kms += call(k, cap, ids, pos, strand)
            if rep >= a.warmup:
                select.append(sms)
                kernel.append(kms)
                wall.append(1e3 * (time.perf_counter() - t0))
        assert int(total.value) == cap == int(counts.sum())
        density = cap / float(nrec * max(1, length - k + 1))
        by = plan_bytes(nrec * ncalls, length, k, w, _abi.KDB_MINIMIZER_PIECE, cap * ncalls)
        sel, emit = statistics.median(select), max(1e-6, statistics.median(kernel) - statistics.median(select))
        run = {"workload": name, "records": ncalls * nrec, "length": length, "k": k, "w": w, "order": "hashed" if hashed else "lexicographic", "calls": ncalls,
               "residues": ncalls * int(bases.size), "minimizers": ncalls * cap, "density": density, "select_ms": select, "kernel_ms": kernel, "call_ms": wall,
               "plan_bytes": by, "select_GBps": (by["select_read"] + by["select_write"]) / 1e6 / sel, "emit_GBps": (by["emit_read"] + by["emit_write"]) / 1e6 / emit,
               "bytes_per_residue": {key: v / float(ncalls * bases.size) for key, v in by.items()}}
        line = ("%-6s %9d records of %9d bp, k=%d w=%d %s, %d call(s): %d minimizers (%.4f of the positions); select+scan %s ms, all kernels %s ms, "
                "%.2f G residues/s; select moves %.2f + %.2f bytes per residue = %.0f GB/s, emit %.2f + %.2f = %.0f GB/s (stream_read %.0f, stream_write %.0f); "
                "call %s ms" % (name, run["records"], length, k, w, run["order"], ncalls, run["minimizers"], density, med_range(select), med_range(kernel),
                                run["residues"] / statistics.median(kernel) / 1e6, run["bytes_per_residue"]["select_read"], run["bytes_per_residue"]["select_write"],
                                run["select_GBps"], run["bytes_per_residue"]["emit_read"], run["bytes_per_residue"]["emit_write"], run["emit_GBps"], stream_read,
                                stream_write, med_range(wall)))
        if not a.no_host:
            # the lists the parent allowed, on one call's records, at k = 15; the call itself at that k to compare with
            t0 = time.perf_counter()
            call(HOST_K, 0, empty, empty, empty)
            cap15 = int(total.value)
            ids15, pos15, strand15 = np.zeros(cap15, dtype=np.uint64), np.zeros(cap15, dtype=np.uint32), np.zeros(cap15, dtype=np.uint8)
            call(HOST_K, cap15, ids15, pos15, strand15)
            t1 = time.perf_counter()
            call(HOST_K, cap15, ids15, pos15, strand15)
            call15 = 1e3 * (time.perf_counter() - t1) * ncalls
            counts15 = counts.copy()
            with IdsEngine(HOST_K, canonicalize=True) as ids_engine:
                t0 = time.perf_counter()
                hc, hi, hp = host_minimizers(ids_engine, bases, offsets, HOST_K, w, hashed, length)
                host = 1e3 * (time.perf_counter() - t0) * ncalls
            same = bool(np.array_equal(hc, counts15) and np.array_equal(hi, ids15) and np.array_equal(hp, pos15))
            run.update({"host_k": HOST_K, "host_ms": host, "call_at_host_k_ms": call15, "host_over_call": host / call15, "host_gives_the_same_lists": same})
            line += "; k=%d: window_ids + numpy %.0f ms = %.1f x the call (%.1f ms); same lists: %s" % (HOST_K, host, host / call15, call15, same)
            del hc, hi, hp, ids15, pos15, strand15
        out["runs"].append(run)
        print(line, flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
