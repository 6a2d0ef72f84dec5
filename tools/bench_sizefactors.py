"""Device time of kdb_size_factors (the geomean sweep and the six passes of the radix select) and of kdb_scale_counts, both of
csrc/kdb_sizefactors.hip.h, at k = 12 for n = 2, 4, 16 vectors, next to the memory system's streamed-read rate from the same process
(kdb_hbm_pattern_probe).
    python tools/bench_sizefactors.py [--k 12] [--n 2,4,16] [--reps 20] [--warmup 3] [--json out.json]
Vectors: tools/bench_pairstats.py's -- seeded counts of a read set's sparsity, about a third of the bins empty, small counts elsewhere, a
few large ones.
Time: kernel_ms_out (HIP events around each kernel, added up; the host's narrowing between the passes is not in it), median and spread
over --reps calls after --warmup.  "call" is the host clock around the whole call, scratch allocation and the round trips of the select
included.
Read rate: bytes the kernels load per call over the median device time.  The geomean sweep reads the n vectors once and writes L; each of
the NPASS = 6 select passes reads every vector and L once per vector: n * 8 N + 6 * n * 16 N bytes loaded, 8 N stored.  kdb_scale_counts
reads and writes a vector once (twice read when the size factor is 2 or less: the sweep that looks for a quotient of 2^63 comes first).
No GPU, no number: this tool has no fallback."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

NPASS = 6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=12)
    ap.add_argument("--n", default="2,4,16")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    import torch
    import kmerdb_amd
    from kmerdb_amd import _abi, matrix
    lib = _abi.lib()
    if kmerdb_amd.device_count() < 1:
        raise SystemExit("no HIP device: nothing is measured")
    nbins = 4 ** a.k
    ns = [int(x) for x in a.n.split(",")]
    rng = np.random.default_rng(12)
    tensors = []
    for i in range(max(ns)):
        v = rng.poisson(2.0 + i % 5, nbins).astype(np.uint64) * (rng.integers(0, 3, nbins) > 0).astype(np.uint64)
        v[rng.integers(0, nbins, 64)] = np.uint64(100000)
        tensors.append(torch.from_numpy(v.view(np.int64)).to("cuda:0"))
    torch.cuda.synchronize(0)
    out = {"k": a.k, "nbins": nbins, "reps": a.reps, "warmup": a.warmup, "runs": []}

    def report(name, n, ms, wall, loaded, stored, extra=""):
        med = statistics.median(ms)
        run = {"call": name, "n": n, "ms_median": med, "ms_min": min(ms), "ms_max": max(ms), "ms_spread_pct": 100.0 * (max(ms) - min(ms)) / med,
               "call_ms_median": statistics.median(wall), "bytes_loaded": loaded, "bytes_stored": stored, "read_GBps": loaded / 1e6 / med}
        out["runs"].append(run)
        print("%-13s n=%2d  %8.3f ms median (min %.3f, max %.3f, spread %.1f %%)  whole call %8.3f ms  loads %6.2f GiB -> %7.1f GB/s%s" % (
            name, n, med, min(ms), max(ms), run["ms_spread_pct"], run["call_ms_median"], loaded / 2 ** 30, run["read_GBps"], extra))

    for n in ns:
        ptrs = [t.data_ptr() for t in tensors[:n]]
        ms, wall, eligible = [], [], 0
        for i in range(a.warmup + a.reps):
            t0 = time.perf_counter()
            _, eligible, kernel_ms = matrix.size_factors_raw(ptrs, nbins)
            if i >= a.warmup:
                ms.append(kernel_ms)
                wall.append(1e3 * (time.perf_counter() - t0))
        report("size_factors", n, ms, wall, n * 8 * nbins + NPASS * n * 16 * nbins, 8 * nbins, "  (%d eligible bins)" % eligible)
    dst = torch.empty(nbins, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize(0)
    for s, sweeps in ((3.0, 1), (0.75, 2)):
        ms, wall = [], []
        for i in range(a.warmup + a.reps):
            t0 = time.perf_counter()
            kernel_ms = matrix.scale_counts_raw(tensors[0].data_ptr(), nbins, s, dst.data_ptr())
            if i >= a.warmup:
                ms.append(kernel_ms)
                wall.append(1e3 * (time.perf_counter() - t0))
        report("scale s=%g" % s, 1, ms, wall, sweeps * 8 * nbins, 8 * nbins)
    del tensors, dst
    torch.cuda.empty_cache()
    npat = lib.kdb_hbm_pattern_count()
    rates = (ctypes.c_double * npat)()
    _abi.check(lib.kdb_hbm_pattern_probe(0, rates, npat))
    out["pattern_ceilings_GBps"] = {lib.kdb_hbm_pattern_name(i).decode(): rates[i] for i in range(npat)}
    print("kdb_hbm_pattern_probe (same process): " + ", ".join("%s %.0f GB/s" % kv for kv in out["pattern_ceilings_GBps"].items()))
    print(json.dumps(out))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
