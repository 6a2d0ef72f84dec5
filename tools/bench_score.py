"""Device time of kdb_score_reads (csrc/kdb_score.hip.h) on the headline read set -- 10 M reads of 150 bp -- at k = 12 forward (the
128 MiB vector sits in the memory-side cache), k = 15 forward (8 GiB, beyond it) and k = 12 canonical, next to two yardsticks from the
same process on the same device:
  * the composition the engine allowed before: kdb_window_ids (8 bytes per residue back to the host) + torch index_select / log /
    index_add_ on the ids (uploaded again), the same score;
  * the memory system's rates for the access patterns of kdb_hbm_pattern_probe.
    python tools/bench_score.py [--reads 10000000] [--len 150] [--configs 12f,15f,12c] [--reps 5] [--warmup 2] [--comp-reps 2] [--json out.json]
A call takes at most 2^30 residues, so the reads go through in calls of --call-reads (5 M) and the times of the calls are added.
"kernel" is kernel_ms_out: HIP events around the residue check and the two scoring kernels.  "call" is the host clock around the whole
call: upload of the residues, scratch, kernels, results back.  "gather" is windows x 32 bytes (four lookups of 8 bytes on a canonical
profile) over the kernel time -- the bytes the score needs from the vector, not what the memory system moved.  The composition has no
kernel time of its own: its host clock is set against the fused call's.  No GPU, no number: this tool has no fallback."""
import argparse
import ctypes
import json
import math
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def rc_torch(x, k):
    out = x.new_zeros(x.shape)
    for _ in range(k):
        out = (out << 2) | (3 - (x & 3))
        x = x >> 2
    return out


def composition(torch, ids_engine, bases, offsets, vt, k, canonical, total):
    """the same score from kdb_window_ids and torch on the device -> log10_p per record (float64 tensor)"""
    ids = ids_engine.window_ids(bases, offsets)
    t = torch.from_numpy(ids.view(np.int64)).to("cuda:0")
    offs = torch.from_numpy(offsets.astype(np.int64)).to("cuda:0")
    pos = torch.nonzero(t != -1).squeeze(1)
    wid = t[pos]
    del t
    rec = torch.bucketize(pos, offs[1:], right=True)
    look = (lambda i: vt.index_select(0, torch.minimum(i, rc_torch(i, k)))) if canonical else (lambda i: vt.index_select(0, i))
    c = look(wid).double()
    base = wid & ~3
    d = look(base).double()
    for x in (1, 2, 3):
        d += look(base + x).double()
    first = torch.ones_like(rec, dtype=torch.bool)
    first[1:] = rec[1:] != rec[:-1]
    d[first] = float(total)
    term = torch.log(c) - torch.log(d)
    out = torch.zeros(offsets.size - 1, dtype=torch.float64, device="cuda:0").index_add_(0, rec, term)
    torch.cuda.synchronize(0)
    return out / math.log(10.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--len", type=int, default=150)
    ap.add_argument("--call-reads", type=int, default=5_000_000)
    ap.add_argument("--configs", default="12f,15f,12c")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--comp-reps", type=int, default=2)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    import torch
    import kmerdb_amd
    from kmerdb_amd import _abi, probability, synth
    from kmerdb_amd.engine import IdsEngine
    lib = _abi.lib()
    if kmerdb_amd.device_count() < 1:
        raise SystemExit("no HIP device: nothing is measured")
    out = {"reads": a.reads, "read_len": a.len, "call_reads": a.call_reads, "reps": a.reps, "warmup": a.warmup, "runs": []}

    n = lib.kdb_hbm_pattern_count()
    rates = (ctypes.c_double * n)()
    _abi.check(lib.kdb_hbm_pattern_probe(0, rates, n))
    out["pattern_GBps"] = {lib.kdb_hbm_pattern_name(i).decode(): rates[i] for i in range(n)}
    for name, r in out["pattern_GBps"].items():
        print("pattern %-28s %8.1f GB/s" % (name, r))

    bases, offsets = synth.reads(a.reads, a.len, seed=synth.SEED0)
    calls = []
    for r0 in range(0, a.reads, a.call_reads):
        r1 = min(a.reads, r0 + a.call_reads)
        calls.append((bases[r0 * a.len:r1 * a.len], offsets[r0:r1 + 1] - offsets[r0]))

    for cfg in a.configs.split(","):
        k, canonical = int(cfg[:-1]), cfg[-1] == "c"
        g = torch.Generator(device="cuda:0")
        g.manual_seed(k)
        vt = torch.randint(1, 1000, (4 ** k,), dtype=torch.int64, device="cuda:0", generator=g)      # every bin occupied: every term finite
        total = int(vt.sum().item())
        torch.cuda.synchronize(0)
        windows = a.reads * (a.len - k + 1)
        kernel, wall, fused = [], [], None
        for rep in range(a.warmup + a.reps):
            ms, t0, res = 0.0, time.perf_counter(), []
            for b, o in calls:
                got = probability.score_reads_raw(vt.data_ptr(), k, canonical, total, 0, b, o)
                ms += got[4]
                res.append(got[0])
            if rep >= a.warmup:
                kernel.append(ms)
                wall.append(1e3 * (time.perf_counter() - t0))
            fused = np.concatenate(res)
        comp_wall, worst = [], 0.0
        with IdsEngine(k, canonicalize=False) as ids_engine:
            for rep in range(1 + a.comp_reps):
                t0, res = time.perf_counter(), []
                for b, o in calls:
                    res.append(composition(torch, ids_engine, b, o, vt, k, canonical, total).cpu().numpy())
                if rep >= 1:
                    comp_wall.append(1e3 * (time.perf_counter() - t0))
                worst = float(np.max(np.abs(np.concatenate(res) - fused)))
        torch.cuda.empty_cache()
        med = statistics.median(kernel)
        run = {"k": k, "canonical": canonical, "vector_MiB": 4 ** k * 8 / 2 ** 20, "windows": windows, "kernel_ms_median": med, "kernel_ms_min": min(kernel),
               "kernel_ms_max": max(kernel), "call_ms_median": statistics.median(wall), "gather_GBps": windows * 32 / 1e6 / med,
               "windows_per_s": windows / med * 1e3, "composition_ms_median": statistics.median(comp_wall), "composition_ms_min": min(comp_wall),
               "max_abs_difference_of_log10_p": worst}
        out["runs"].append(run)
        print("k=%2d %-9s vector %7.0f MiB  kernel %8.3f ms median (min %.3f, max %.3f)  %6.2f G windows/s  gather %7.1f GB/s  whole call %9.1f ms  "
              "composition %9.1f ms (min %.1f): %5.1f x the call  |log10_p difference| <= %.3g" % (
                  k, "canonical" if canonical else "forward", run["vector_MiB"], med, min(kernel), max(kernel), run["windows_per_s"] / 1e9, run["gather_GBps"],
                  run["call_ms_median"], run["composition_ms_median"], min(comp_wall), run["composition_ms_median"] / run["call_ms_median"], worst))
        del vt
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
