"""Device time of kdb_gram (exact sums + Gram matrix of count vectors, csrc/kdb_gram.hip.h) at k = 12 for n = 2, 4, 16 vectors, next to the
memory system's streamed-read rate from the same process (kdb_hbm_pattern_probe).
    python tools/bench_gram.py [--k 12] [--n 2,4,16] [--reps 20] [--warmup 3] [--json out.json]
Vectors: seeded counts of a read set's sparsity -- about a third of the bins empty, small counts elsewhere, a few large ones -- all below
2^32, so the sweep takes its short multiply; --wide puts one count of 2^33 into every vector's every 4096th bin (every wave's full multiply).
Time: kernel_ms_out of kdb_gram (HIP events around the sweep and the combine), median and spread over --reps calls after --warmup.
Read rate: bytes the kernels load per call -- every row of vector blocks reads its own blocks' vectors (a block of 4 on the diagonal, two
blocks off it) -- over the median time.  "useful" rate: n vectors once over the same time.  No GPU, no number: this tool has no fallback."""
import argparse
import ctypes
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def vectors_read(n, B):
    """vector sweeps a call makes: per pair of blocks (bi <= bj) the vectors of both blocks (of the one block on the diagonal)"""
    sizes = [min(B, n - b) for b in range(0, n, B)]
    return sum(sizes[i] if i == j else sizes[i] + sizes[j] for i in range(len(sizes)) for j in range(i, len(sizes)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=12)
    ap.add_argument("--n", default="2,4,16")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--wide", action="store_true")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    import torch
    import kmerdb_amd
    from kmerdb_amd import _abi, distance
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
        if a.wide:
            v[::4096] = np.uint64(1 << 33)
        tensors.append(torch.from_numpy(v.view(np.int64)).to("cuda:0"))
    torch.cuda.synchronize(0)
    out = {"k": a.k, "nbins": nbins, "reps": a.reps, "warmup": a.warmup, "wide": bool(a.wide), "runs": []}
    for n in ns:
        ptrs = [t.data_ptr() for t in tensors[:n]]
        for _ in range(a.warmup):
            distance.gram(ptrs, nbins)
        ms = [distance.gram(ptrs, nbins)[2] for _ in range(a.reps)]
        med = statistics.median(ms)
        read_bytes = vectors_read(n, _abi.KDB_GRAM_BLOCK) * nbins * 8
        run = {"n": n, "pairs": n * (n + 1) // 2, "ms_median": med, "ms_min": min(ms), "ms_max": max(ms),
               "ms_spread_pct": 100.0 * (max(ms) - min(ms)) / med, "bytes_loaded": read_bytes,
               "read_GBps": read_bytes / 1e6 / med, "useful_GBps": n * nbins * 8 / 1e6 / med}
        out["runs"].append(run)
        print("n=%2d  %8.3f ms median (min %.3f, max %.3f, spread %.1f %%)  loads %6.2f GiB -> %7.1f GB/s  (the n vectors once: %7.1f GB/s)" % (
            n, med, min(ms), max(ms), run["ms_spread_pct"], read_bytes / 2 ** 30, run["read_GBps"], run["useful_GBps"]))
    del tensors
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
