"""Device time of kdb_pairstats (the exact pairwise integers) and kdb_pairfloat (canberra / Jensen-Shannon in float64), both of
csrc/kdb_pairstats.hip.h, at k = 12 for n = 2, 4, 16 vectors, next to the memory system's streamed-read rate from the same process
(kdb_hbm_pattern_probe).
    python tools/bench_pairstats.py [--k 12] [--n 2,4,16] [--reps 20] [--warmup 3] [--no-float] [--json out.json]
Vectors: tools/bench_gram.py's -- seeded counts of a read set's sparsity, about a third of the bins empty, small counts elsewhere, a few
large ones.
Time: kernel_ms_out (HIP events around the sweep, its tail and the combine), median and spread over --reps calls after --warmup.
Read rate: bytes the kernels load per call over the median time.  The integer sweep reads a block of 4 vectors per diagonal row and 4 + 2
(4 + 1) per row off the diagonal; the float sweep reads two vectors per pair.  "useful" rate: the n vectors once over the same time.
No GPU, no number: this tool has no fallback."""
import argparse
import ctypes
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def vectors_read(n, B, half):
    """vector sweeps a kdb_pairstats call makes: a diagonal row reads its block; every earlier block is read once more against each `half`
    (or fewer) vectors of a later block, with those"""
    sizes = [min(B, n - b) for b in range(0, n, B)]
    total = sum(sizes)
    for bj in range(1, len(sizes)):
        for h in range(0, sizes[bj], half):
            total += bj * (B + min(half, sizes[bj] - h))
    return total


def measure(call, ptrs, nbins, reps, warmup):
    for _ in range(warmup):
        call(ptrs, nbins)
    return [call(ptrs, nbins)[-1] for _ in range(reps)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=12)
    ap.add_argument("--n", default="2,4,16")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-float", action="store_true", help="the integer sweep only")
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
        tensors.append(torch.from_numpy(v.view(np.int64)).to("cuda:0"))
    torch.cuda.synchronize(0)
    out = {"k": a.k, "nbins": nbins, "reps": a.reps, "warmup": a.warmup, "runs": []}
    sweeps = [("pairstats", distance.pairstats_raw)] + ([] if a.no_float else [("pairfloat", distance.pairfloat_raw)])
    for n in ns:
        ptrs = [t.data_ptr() for t in tensors[:n]]
        for name, call in sweeps:
            ms = measure(call, ptrs, nbins, a.reps, a.warmup)
            med = statistics.median(ms)
            reads = vectors_read(n, _abi.KDB_PAIRSTATS_BLOCK, _abi.KDB_PAIRSTATS_HALF) if name == "pairstats" else n * (n - 1)
            read_bytes = reads * nbins * 8
            run = {"sweep": name, "n": n, "pairs": n * (n - 1) // 2, "ms_median": med, "ms_min": min(ms), "ms_max": max(ms),
                   "ms_spread_pct": 100.0 * (max(ms) - min(ms)) / med, "bytes_loaded": read_bytes,
                   "read_GBps": read_bytes / 1e6 / med, "useful_GBps": n * nbins * 8 / 1e6 / med,
                   "pair_bins_per_ns": n * (n - 1) // 2 * nbins / 1e6 / med}
            out["runs"].append(run)
            print("%-9s n=%2d  %8.3f ms median (min %.3f, max %.3f, spread %.1f %%)  loads %6.2f GiB -> %7.1f GB/s  (the n vectors once: %7.1f GB/s; "
                  "%.2f pair-bins/ns)" % (name, n, med, min(ms), max(ms), run["ms_spread_pct"], read_bytes / 2 ** 30, run["read_GBps"],
                                          run["useful_GBps"], run["pair_bins_per_ns"]))
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
