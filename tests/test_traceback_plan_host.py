"""CPU: kdbplan::align_trace_bytes and align_trace_chunks -- the direction scratch of a task of kdb_align_traceback and the chunks of
consecutive tasks the call works through -- built alone from tests/c/traceback_plan_check.cpp with AddressSanitizer + UBSan and run as a
program (never loaded into Python); its printed plans against the definition.  Where this g++ has no sanitizer runtime the program is
built plainly."""
import atexit
import functools
import os
import re
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]


def _header_constant(name):
    text = open(os.path.join(ROOT, "include", "kdbhip.h")).read()
    return int(re.search(r"#define\s+%s\s+(\d+)" % name, text).group(1))


STAGE, MAX_BAND, MAX_QUERY = (_header_constant("KDB_ALIGN_" + x) for x in ("STAGE", "MAX_BAND", "MAX_QUERY"))


@functools.lru_cache(maxsize=None)
def program():
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    where = tempfile.mkdtemp(prefix="traceback_plan_check_")
    atexit.register(shutil.rmtree, where, ignore_errors=True)
    exe = os.path.join(where, "traceback_plan_check")
    src = os.path.join(ROOT, "tests", "c", "traceback_plan_check.cpp")
    done = subprocess.run([gxx, "-std=c++17", "-O1", "-g"] + SANITIZE + ["-o", exe, src], capture_output=True, text=True)
    if done.returncode != 0 and "sanitize" in done.stderr:
        done = subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-o", exe, src], capture_output=True, text=True)
    assert done.returncode == 0, done.stderr
    return exe


def run(args):
    done = subprocess.run([program()] + [str(a) for a in args], capture_output=True, text=True, timeout=120)
    assert done.returncode == 0, done.stdout[-2000:] + done.stderr[-2000:]
    assert "ERROR" not in done.stderr and "runtime error" not in done.stderr and "FAILED" not in done.stdout, done.stdout[-2000:] + done.stderr[-2000:]
    lines = done.stdout.splitlines()
    assert lines[-1] == "traceback plan check ok"
    out = []
    for line in lines[:-1]:
        fields = dict(x.split("=", 1) for x in line.split()[1:])
        out.append({a: [int(v) for v in b.split(",")] if a == "first" else int(b) for a, b in fields.items()})
    return out


def task_bytes(cases):
    """cases: (m, n, d, band) -> the printed line of each"""
    args = []
    for m, n, d, band in cases:
        args += ["bytes", m, n, d, band]
    out = run(args)
    assert len(out) == len(cases)
    return out


def expected_bytes(m, n, d, band):
    """from the definition: 64 bytes per step T = i + c // 2 of the band's cells in the rows that reach the record, in whole groups of 4
    steps that begin at multiples of 4"""
    rows = [i for i in range(m) if max(0, i + d - band) <= min(n - 1, i + d + band)]
    if not rows:
        return 0
    groups = {(i + c // 2) // 4 for i in (rows[0], rows[-1]) for c in (0, 2 * band)}
    return 256 * (max(groups) - min(groups) + 1)


def test_bytes_are_the_groups_of_steps_a_task_takes():
    cases = []
    for band in (1, 2, 16, MAX_BAND):
        for m, n in [(150, 5000), (40, 30), (1, 1), (3, 9), (4, 9), (5, 9), (2 * band + 1, band), (STAGE + 1, 2 * STAGE + 7), (300, 100)]:
            for d in (0, 1, -1, band, -band, -(m - 1), n - 1, -(m - 1) - band, n - 1 + band, -(m - 1) - band - 1, n + band, -20, n - m + 5, 2 ** 40, -2 ** 40):
                cases.append((m, n, d, band))
    got = task_bytes(cases)
    empty = 0
    for case, line in zip(cases, got):
        want = expected_bytes(*case)
        assert line["bytes"] == want == 256 * line["groups"] == 256 * line["brute"] and line["empty"] == (want == 0), (case, line)
        empty += want == 0
    assert empty > 20
    # the figures of the header: a read of 150 residues at band 16 takes about 11 KB
    line, = task_bytes([(150, 5000, 100, 16)])
    assert line["bytes"] == 256 * -(-(150 + 16) // 4) == 10752


def test_the_largest_task():
    line, = task_bytes([(MAX_QUERY, 2 ** 30, 2 ** 30 - MAX_QUERY, MAX_BAND)])
    assert line["bytes"] == 256 * -(-(MAX_QUERY + MAX_BAND) // 4) == 256 * line["brute"] and 67 * 10 ** 6 < line["bytes"] < 68 * 10 ** 6


def chunks(limit, sizes):
    out, = run(["chunks", limit, ",".join(map(str, sizes)) if sizes else "-"])
    return out


def expected_chunks(limit, sizes):
    first, used = [0], 0
    for t, b in enumerate(sizes):
        if t > first[-1] and used + b > limit or (t > first[-1] and used > limit):
            first.append(t)
            used = 0
        used += b
    return first + [len(sizes)]


def test_chunk_cuts():
    big = 256 * -(-(MAX_QUERY + MAX_BAND) // 4)
    sizes = [10752, 0, 0, 768, 10752, 0, 256, big, 0, 10752, 10752, 0]
    total = sum(sizes)
    for limit in (1, 10752, 10753, 10752 + 768, 10752 + 767, 2 * 10752 + 768 + 256, big, big + 1, big - 1, total - 1, total, 2 ** 31, 2 ** 64 - 1):
        got = chunks(limit, sizes)
        assert got["first"] == expected_chunks(limit, sizes) and got["n"] == len(got["first"]) - 1 and got["bytes"] == total, (limit, got)
    # a limit of one byte: every task with bytes is a chunk of its own, and only an empty task joins an empty one
    assert chunks(1, sizes)["first"] == [0, 1, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12]
    # exactly one task, one task plus one byte, the sum minus one, the sum
    four = [512, 512, 512, 512]
    assert chunks(512, four)["first"] == [0, 1, 2, 3, 4] and chunks(513, four)["first"] == [0, 1, 2, 3, 4] and chunks(1024, four)["first"] == [0, 2, 4]
    assert chunks(2047, four)["first"] == [0, 3, 4] and chunks(2048, four) == {"n": 1, "largest": 2048, "bytes": 2048, "first": [0, 4]}
    assert chunks(2047, four)["largest"] == 1536 and chunks(1, four)["largest"] == 512
    # empty tasks between full ones stay with the chunk before them while that is within its limit
    assert chunks(512, [512, 0, 0, 512, 0])["first"] == [0, 3, 5] and chunks(100, [512, 0, 0, 512, 0])["first"] == [0, 1, 3, 4, 5]
    assert chunks(100, [0, 0, 0]) == {"n": 1, "largest": 0, "bytes": 0, "first": [0, 3]}
    assert chunks(100, []) == {"n": 0, "largest": 0, "bytes": 0, "first": [0]}
    # the largest task among short ones, under the default limit and under its own size
    many = [10752] * 300 + [big] + [10752] * 300
    assert chunks(2 ** 31, many)["n"] == 1 and chunks(big, many)["first"] == [0, 300, 301, 601] and chunks(big + 10752, many)["first"] == [0, 300, 302, 601]
