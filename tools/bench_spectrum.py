"""Device time of kdb_spectrum and kdb_rank_transform (csrc/kdb_spectrum.hip.h) at k = 12 and k = 15, on a vector with a read set's sparsity
and on an all-zero vector, next to the memory system's streamed-read rate from the same process (kdb_hbm_pattern_probe).
    python tools/bench_spectrum.py [--k 12,15] [--reps 20] [--warmup 3] [--json out.json]
Vectors: `reads` -- seeded counts, about a third of the bins empty, small counts elsewhere, 64 bins at 100000 (the list of large values is
not empty); `zeros` -- every lane of every wave wants the same counter: the case a shared histogram serialises on.
Time: kernel_ms_out of the two entry points (HIP events around the sweeps; for kdb_rank_transform the spectrum sweep plus the rank map,
without the host's table work between them), median and spread over --reps calls after --warmup.
Rate: bytes the kernels move per call -- the vector once for the spectrum; for the ranks the vector twice and the ranks once -- over the
median time.  The yardstick is the probe's stream_read; the rank map also writes, so its share is below it by construction.
No GPU, no number: this tool has no fallback."""
import argparse
import ctypes
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", default="12,15")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    import torch
    import kmerdb_amd
    from kmerdb_amd import _abi, spectrum
    lib = _abi.lib()
    if kmerdb_amd.device_count() < 1:
        raise SystemExit("no HIP device: nothing is measured")
    out = {"reps": a.reps, "warmup": a.warmup, "runs": []}
    for k in [int(x) for x in a.k.split(",")]:
        nbins = 4 ** k
        for name in ("reads", "zeros"):
            if name == "reads":
                g = torch.Generator(device="cuda:0")
                g.manual_seed(12 + k)
                t = torch.poisson(torch.full((nbins,), 3.0, device="cuda:0"), generator=g).to(torch.int64)
                t *= (torch.rand(nbins, device="cuda:0", generator=g) < 2.0 / 3.0).to(torch.int64)
                t[torch.randint(0, nbins, (64,), device="cuda:0", generator=g)] = 100000
            else:
                t = torch.zeros(nbins, dtype=torch.int64, device="cuda:0")
            r = torch.empty_like(t)
            torch.cuda.synchronize(0)
            for entry, call, nbytes in (("kdb_spectrum", lambda: spectrum.spectrum_raw(t.data_ptr(), nbins)[2], 8 * nbins),
                                        ("kdb_rank_transform", lambda: spectrum.rank_transform_raw(t.data_ptr(), nbins, r.data_ptr()), 24 * nbins)):
                for _ in range(a.warmup):
                    call()
                ms = [call() for _ in range(a.reps)]
                med = statistics.median(ms)
                run = {"k": k, "vector": name, "entry": entry, "ms_median": med, "ms_min": min(ms), "ms_max": max(ms),
                       "ms_spread_pct": 100.0 * (max(ms) - min(ms)) / med, "bytes_moved": nbytes, "GBps": nbytes / 1e6 / med}
                out["runs"].append(run)
                print("k=%2d %-5s %-18s %8.3f ms median (min %.3f, max %.3f, spread %.1f %%)  moves %6.2f GiB -> %7.1f GB/s" % (
                    k, name, entry, med, min(ms), max(ms), run["ms_spread_pct"], nbytes / 2 ** 30, run["GBps"]))
            if name == "zeros":
                assert int(r[0]) == nbins + 1 and int(r[-1]) == nbins + 1            # (all tied: every doubled mid-rank is N + 1)
            del t, r
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
