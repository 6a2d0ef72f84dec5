"""CPU: kdbplan::align_window and align_layout -- the task windows, the LDS of a stage and the refusals kdb_align_banded settles on the host
before anything is launched -- built alone from tests/c/alignment_plan_check.cpp with AddressSanitizer + UBSan and run as a program (never
loaded into Python); its printed plans against the definition.  Where this g++ has no sanitizer runtime the program is built plainly."""
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


STAGE, MAX_BAND, MAX_QUERY, GRID_MAX = (_header_constant("KDB_ALIGN_" + x) for x in ("STAGE", "MAX_BAND", "MAX_QUERY", "GRID_MAX"))


@functools.lru_cache(maxsize=None)
def program():
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    where = tempfile.mkdtemp(prefix="alignment_plan_check_")
    atexit.register(shutil.rmtree, where, ignore_errors=True)
    exe = os.path.join(where, "alignment_plan_check")
    src = os.path.join(ROOT, "tests", "c", "alignment_plan_check.cpp")
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
    assert lines[-1] == "alignment plan check ok"
    out = []
    for line in lines[:-1]:
        words = line.split()
        out.append(tuple(words) if words[0] == "refused" else {a: int(b) for a, b in (x.split("=", 1) for x in words[1:])})
    return out


def windows(cases, stage=STAGE):
    """cases: (m, n, d, band) -> the printed window of each"""
    args = []
    for m, n, d, band in cases:
        args += ["window", m, n, d, band, stage]
    out = run(args)
    assert len(out) == len(cases)
    return out


def expected_window(m, n, d, band):
    """from the definition: the rows and columns of the cells 0 <= i < m, 0 <= j < n with |(j - i) - d| <= band"""
    rows = [i for i in range(m) if max(0, i + d - band) <= min(n - 1, i + d + band)]
    if not rows:
        return None
    return {"i_lo": rows[0], "i_hi": rows[-1] + 1, "r_lo": max(0, rows[0] + d - band), "r_hi": min(n, rows[-1] + d + band + 1), "jb": d - band}


def test_windows_are_the_definition():
    cases = []
    for band in (1, 2, 16, MAX_BAND):
        for m, n in [(150, 5000), (40, 30), (1, 1), (2 * band + 1, band), (STAGE + 1, 2 * STAGE + 7), (300, 100)]:
            for d in (0, 1, -1, band, -band, -(m - 1), n - 1, -(m - 1) - band, n - 1 + band, -(m - 1) - band - 1, n + band, -20, n - m + 5, n - 100, 10 ** 6, -10 ** 6):
                cases.append((m, n, d, band))
    got = windows(cases)
    hang_start = hang_end = missed = 0
    for (m, n, d, band), w in zip(cases, got):
        want = expected_window(m, n, d, band)
        if want is None:
            assert w["empty"] == 1 and w["stages"] == 0, (m, n, d, band)
            missed += 1
            continue
        assert w["empty"] == 0 and {key: w[key] for key in want} == want, (m, n, d, band, w)
        assert w["t_lo"] == want["i_lo"] // 4 * 4 and w["t_hi"] == want["i_hi"] + band
        assert w["stages"] == -(-(w["t_hi"] - w["t_lo"]) // STAGE)
        hang_start += d < 0 and w["r_lo"] == 0
        hang_end += d + m > n and w["r_hi"] == n
    assert hang_start > 20 and hang_end > 20 and missed > 20


def test_one_cell_in_the_band_and_none():
    m, n, band = 37, 91, 5
    one_a, one_b, none_a, none_b = windows([(m, n, -(m - 1) - band, band), (m, n, n - 1 + band, band), (m, n, -(m - 1) - band - 1, band), (m, n, n + band, band)])
    assert (one_a["i_lo"], one_a["i_hi"], one_a["r_lo"], one_a["r_hi"]) == (m - 1, m, 0, 1)
    assert (one_b["i_lo"], one_b["i_hi"], one_b["r_lo"], one_b["r_hi"]) == (0, 1, n - 1, n)
    assert none_a["empty"] == none_b["empty"] == 1


def test_empty_records_and_far_diagonals():
    got = windows([(0, 100, 0, 3), (100, 0, 0, 3), (0, 0, 0, 3), (100, 100, 2 ** 62, 3), (100, 100, -2 ** 63, MAX_BAND), (100, 100, 2 ** 63 - 1, MAX_BAND),
                   (100, 100, 2 ** 32, 1), (100, 100, -2 ** 31, 1)])
    assert all(w["empty"] == 1 and w["jb"] == 0 for w in got)


def test_the_largest_task_and_the_lds_of_a_stage():
    big, = windows([(MAX_QUERY, 2 ** 30, 2 ** 30 - MAX_QUERY, MAX_BAND)])
    assert big["empty"] == 0 and big["i_hi"] == MAX_QUERY and big["r_hi"] == 2 ** 30 and big["jb"] == 2 ** 30 - MAX_QUERY - MAX_BAND
    assert big["stages"] == -(-(MAX_QUERY + MAX_BAND) // STAGE)
    # per wave: the rows of a stage and 64 before them, and the columns those rows reach over 127 diagonals, in whole words
    assert 2 * STAGE + 64 + 128 <= big["lds_wave"] <= 2 * STAGE + 64 + 128 + 32 and 4 * big["lds_wave"] <= 64 * 1024
    small, = windows([(100, 100, 0, MAX_BAND)], stage=8)                      # (the stage is an argument: the smallest)
    assert small["stages"] == -(-(100 + MAX_BAND) // 8) and small["lds_wave"] == 2 * 8 + big["lds_wave"] - 2 * STAGE


def layout(band, q_offs, r_offs, tasks, q_nbytes=None, r_nbytes=None, max_query=MAX_QUERY, waves=4, grid_max=GRID_MAX):
    col = lambda i: ",".join(str(t[i]) for t in tasks) if tasks else "-"
    out, = run(["layout", band, max_query, waves, grid_max, q_offs[-1] if q_nbytes is None else q_nbytes, ",".join(map(str, q_offs)),
                r_offs[-1] if r_nbytes is None else r_nbytes, ",".join(map(str, r_offs)), col(0), col(1), col(2), col(3)])
    return out


def test_layout_and_refusals():
    q, r = [0, 10, 10, 30], [0, 50, 80]
    tasks = [(0, 0, 0, 0), (2, 1, 5, 1), (1, 0, 0, 0), (2, 0, 500, 0), (0, 1, -9 - 16, 1)]
    ok = layout(16, q, r, tasks)
    assert ok == {"grid": 2, "cells": (10 + 20 + 0 + 20 + 10) * 33, "nonempty": 3}
    assert layout(16, q, r, [])["grid"] == 1
    assert layout(1, q, r, tasks * 5000, grid_max=100)["grid"] == 100 and layout(1, q, r, tasks * 50, waves=4)["grid"] == 63
    assert layout(16, [1, 10, 30], r, tasks[:1]) == ("refused", "ends") and layout(16, q, r, tasks, q_nbytes=31) == ("refused", "ends")
    assert layout(16, q, r, tasks, r_nbytes=79) == ("refused", "ends") and layout(16, q, [2, 80], tasks[:1]) == ("refused", "ends")
    assert layout(16, [0, 12, 10, 30], r, tasks) == ("refused", "rise") and layout(16, q, [0, 90, 80], tasks) == ("refused", "rise")
    assert layout(16, q, r, tasks[:2] + [(3, 0, 0, 0)]) == ("refused", "task", "2") and layout(16, q, r, [(0, 2, 0, 0)]) == ("refused", "task", "0")
    assert layout(16, q, r, tasks[:1] + [(0, 0, 0, 2)]) == ("refused", "strand", "1")
    assert layout(16, q, r, tasks, max_query=19) == ("refused", "query", "1") and layout(16, q, r, tasks, max_query=20) == ok
