#!/usr/bin/env python3
"""Per-dispatch table of a counting step from a rocprofv3 --kernel-trace run (csv):

    rocprofv3 --kernel-trace --output-format csv -d DIR -- python3 bench.py --steps 24 --warmup 4 ...
    python3 tools/step_dispatches.py DIR [label]

For every kernel of the steady state (the last TAIL dispatches of the trace: the timed steps, whatever came before them):
launches, average and total duration, and the idle time in front of it -- from the end of the dispatch before it on the device
to its own start.  hipMemsetAsync shows as the runtime's fill kernel; its launches are told apart by their grid size.
"""
import csv
import glob
import os
import sys

TAIL = 260             # dispatches looked at: 40 steps of the one-level path (26 dispatches per cycle of four batches)


def short(name):
    n = name.split("(")[0].replace("void ", "").replace("kdb::", "")
    if "<" in n:
        head, args = n.split("<", 1)
        n = head + "<" + args[:28] + ("..." if len(args) > 28 else "")
    return n[:64]


def main():
    d = sys.argv[1]
    label = sys.argv[2] if len(sys.argv) > 2 else d
    files = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        sys.exit("no kernel_trace.csv under " + d)
    rows = []
    for f in files:
        rows += [(int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"], r.get("Grid_Size_X") or r.get("Grid_Size") or "?") for r in csv.DictReader(open(f))]
    rows.sort()
    rows = rows[-TAIL:]
    table = {}
    prev_end = None
    span = rows[-1][1] - rows[0][0]
    busy = idle = 0
    for s, e, name, grid in rows:
        key = short(name)
        dur = e - s
        if "fillBuffer" in name or "FillBuffer" in name:
            key = "memset (fill kernel, grid %s)" % grid
        elif "scatter_bases_kernel" in name and dur < 8000:
            key += " [returns at once]"
        gap = max(s - prev_end, 0) if prev_end is not None else 0
        t = table.setdefault(key, [0, 0, 0])
        t[0] += 1; t[1] += dur; t[2] += gap
        busy += dur; idle += gap
        prev_end = max(prev_end, e) if prev_end is not None else e
    print("== %s: last %d dispatches, %.3f ms from first start to last end, busy %.3f ms, idle between dispatches %.3f ms ==" %
          (label, len(rows), span / 1e6, busy / 1e6, idle / 1e6))
    print("%-66s %8s %10s %10s %12s %12s" % ("kernel", "launches", "avg us", "total ms", "gap before us", "gaps ms"))
    for key, (n, dur, gap) in sorted(table.items(), key=lambda kv: -kv[1][1]):
        print("%-66s %8d %10.2f %10.4f %12.2f %12.4f" % (key, n, dur / n / 1e3, dur / 1e6, gap / n / 1e3, gap / 1e6))


if __name__ == "__main__":
    main()
