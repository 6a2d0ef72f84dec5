"""Device and call time of kdb_record_tables (csrc/kdb_tables.hip.h) on three workloads:
  reads    10 M reads of 150 bp, k = 4, stride 1, canonical: the composition vector of every read (1 KiB of row per 150 residues)
  cds      10 M CDS-like records of 999 bp, k = 3, stride 3: the codon table of every record (256 bytes of row per 999 residues)
  genome   one record of 100 Mbp, k = 4, stride 1, canonical: every piece adds its bins to one row
next to two yardsticks from the same process on the same device:
  * what the engine allowed before for the same result: kdb_window_ids (8 bytes per residue back to the host), then one np.bincount over
    (record, id) on the host -- the fastest host form of a bincount per record -- on the records of one call;
  * the streamed-write rate of kdb_hbm_pattern_probe: for short records the rows are most of the bytes the kernel moves.
    python tools/bench_tables.py [--records 10000000] [--call-records 1000000] [--genome 100000000] [--reps 5] [--warmup 2] [--json out.json]
A call takes at most 2^30 residues and 2^31 table entries, so the records go through in calls of --call-records and the times of the
calls are added; the calls of a pass take the same --call-records synthetic records (the work does not depend on their letters, and
10 M x 999 residues would not fit a host buffer comfortably).  "kernel" is kernel_ms_out: HIP events around the call's kernels.  "call"
is the host clock around the whole call: upload of the residues and offsets, scratch, kernels, rows back into a host buffer that is
reused.  "upload" and "rows back" are torch copies of the same sizes between pageable host memory and the device, timed alone, to say
which part of a call dominates.  "row rate" is the bytes of rows over the kernel time.  No GPU, no number: this tool has no fallback."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def med_range(xs):
    return "%.2f (%.2f-%.2f)" % (statistics.median(xs), min(xs), max(xs))


def host_composition(ids_engine, bases, offsets, k, stride, length):
    """the same rows from kdb_window_ids and numpy: records of one length, so the windows of the stride are a slice"""
    n = offsets.size - 1
    ids = ids_engine.window_ids(bases, offsets).reshape(n, length)[:, 0:length - k + 1:stride]
    keys = (np.arange(n, dtype=np.int64)[:, None] << (2 * k)) + ids.view(np.int64)
    return np.bincount(keys.ravel(), minlength=n << (2 * k)).astype(np.uint32).reshape(n, 4 ** k)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=10_000_000)
    ap.add_argument("--call-records", type=int, default=1_000_000)
    ap.add_argument("--genome", type=int, default=100_000_000)
    ap.add_argument("--workloads", default="reads,cds,genome")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    import torch
    import kmerdb_amd
    from kmerdb_amd import _abi, synth
    from kmerdb_amd.engine import IdsEngine
    lib = _abi.lib()
    if kmerdb_amd.device_count() < 1:
        raise SystemExit("no HIP device: nothing is measured")
    out = {"records": a.records, "call_records": a.call_records, "genome": a.genome, "reps": a.reps, "warmup": a.warmup, "runs": []}

    n = lib.kdb_hbm_pattern_count()
    rates = (ctypes.c_double * n)()
    _abi.check(lib.kdb_hbm_pattern_probe(0, rates, n))
    out["pattern_GBps"] = {lib.kdb_hbm_pattern_name(i).decode(): rates[i] for i in range(n)}
    stream_write = out["pattern_GBps"]["stream_write"]
    print("pattern stream_write %8.1f GB/s, stream_read %8.1f GB/s" % (stream_write, out["pattern_GBps"]["stream_read"]))

    shapes = {"reads": (150, 4, 1, True), "cds": (999, 3, 3, False), "genome": (a.genome, 4, 1, True)}
    for name in a.workloads.split(","):
        length, k, stride, canonical = shapes[name]
        nrec = 1 if name == "genome" else min(a.call_records, a.records)
        ncalls = 1 if name == "genome" else -(-a.records // nrec)
        bases, offsets = synth.reads(nrec, length, seed=synth.SEED0 + k)
        bases, offsets = np.ascontiguousarray(bases, dtype=np.uint8), np.ascontiguousarray(offsets, dtype=np.uint64)
        tables = np.zeros((nrec, 4 ** k), dtype=np.uint32)                    # (touched once: the timed calls do not fault its pages in)
        windows, skipped = np.zeros(nrec, dtype=np.uint64), np.zeros(nrec, dtype=np.uint64)
        first, last = np.zeros(nrec, dtype=np.int32), np.zeros(nrec, dtype=np.int32)
        ms = ctypes.c_double(0.0)

        def call():
            _abi.check(lib.kdb_record_tables(0, k, stride, 1 if canonical else 0, 0, bases.ctypes.data, bases.size, offsets.ctypes.data, nrec, 0,
                                             tables.ctypes.data, windows.ctypes.data, skipped.ctypes.data, first.ctypes.data, last.ctypes.data, ctypes.byref(ms)))
            return ms.value

        kernel, wall = [], []
        for rep in range(a.warmup + a.reps):
            t0, kms = time.perf_counter(), 0.0
            for _ in range(ncalls):
                kms += call()
            if rep >= a.warmup:
                kernel.append(kms)
                wall.append(1e3 * (time.perf_counter() - t0))
        # the parts of a call, alone: residues up, rows back (pageable host memory on both sides, as in the call)
        up, back = [], []
        dev_rows = torch.zeros(tables.shape, dtype=torch.int32, device="cuda:0")
        host_rows = torch.from_numpy(tables.view(np.int32))
        for rep in range(1 + a.reps):
            torch.cuda.synchronize(0)
            t0 = time.perf_counter()
            d = torch.from_numpy(bases).to("cuda:0")
            torch.cuda.synchronize(0)
            t1 = time.perf_counter()
            host_rows.copy_(dev_rows)
            torch.cuda.synchronize(0)
            t2 = time.perf_counter()
            del d
            if rep >= 1:
                up.append(1e3 * (t1 - t0) * ncalls)
                back.append(1e3 * (t2 - t1) * ncalls)
        del dev_rows
        call()                                                                # (the copy test wrote zeros over the rows)
        # the composition the parent allowed, on one call's records
        comp = []
        with IdsEngine(k, canonicalize=canonical) as ids_engine:
            for rep in range(2):
                t0 = time.perf_counter()
                want = host_composition(ids_engine, bases, offsets, k, stride, length)
                comp.append(1e3 * (time.perf_counter() - t0) * ncalls)
        same = bool(np.array_equal(want, tables))
        del want
        torch.cuda.empty_cache()
        nwin = ncalls * nrec * ((length - k) // stride + 1)
        row_bytes = ncalls * nrec * 4 ** k * 4
        med = statistics.median(kernel)
        run = {"workload": name, "records": ncalls * nrec, "length": length, "k": k, "stride": stride, "canonical": canonical, "calls": ncalls, "windows": nwin,
               "residue_bytes": ncalls * int(bases.size), "row_bytes": row_bytes, "kernel_ms": kernel, "call_ms": wall, "upload_ms": up, "rows_back_ms": back,
               "composition_ms": comp, "row_GBps": row_bytes / 1e6 / med, "share_of_stream_write": row_bytes / 1e6 / med / stream_write,
               "windows_per_s": nwin / med * 1e3, "composition_gives_the_same_rows": same}
        out["runs"].append(run)
        print("%-6s %9d records of %9d bp, k=%d stride %d %s, %d call(s): kernel %s ms, %.2f G windows/s, rows %.1f GB/s = %.0f %% of stream_write; "
              "call %s ms; upload alone %s ms; rows back alone %s ms; window_ids + bincount %.0f ms (min %.0f) = %.1f x the call; same rows: %s" % (
                  name, run["records"], length, k, stride, "canonical" if canonical else "forward", ncalls, med_range(kernel), run["windows_per_s"] / 1e9,
                  run["row_GBps"], 100 * run["share_of_stream_write"], med_range(wall), med_range(up), med_range(back), statistics.median(comp), min(comp),
                  statistics.median(comp) / statistics.median(wall), same))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
