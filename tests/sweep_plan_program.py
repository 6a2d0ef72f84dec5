"""tests/c/sweep_plan_check.cpp built and run: the plans of kmerdb_amd/csrc/kdb_sweep_plan.cpp.h -- the code the entry points run -- as
Python values, for the CPU tests to compare with tests/sweep_cases.py.  One build and one run per command line, per pytest process."""
import atexit
import functools
import os
import shutil
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]
ROW_NS = tuple(range(1, 18)) + (64,)


class NoCompiler(Exception):
    pass


@functools.lru_cache(maxsize=None)
def build(sanitize):
    """-> the program's path.  sanitize: under ASan + UBSan, NoCompiler where this g++ has no sanitizer runtime"""
    gxx = shutil.which("g++")
    if gxx is None:
        raise NoCompiler("no g++")
    where = tempfile.mkdtemp(prefix="sweep_plan_check_")
    atexit.register(shutil.rmtree, where, ignore_errors=True)
    exe = os.path.join(where, "sweep_plan_check")
    done = subprocess.run([gxx, "-std=c++17", "-O1", "-g"] + (SANITIZE if sanitize else []) + ["-o", exe, os.path.join(ROOT, "tests/c/sweep_plan_check.cpp")],
                          capture_output=True, text=True)
    if done.returncode != 0 and sanitize and "sanitize" in done.stderr:
        raise NoCompiler("this g++ has no sanitizer runtime")
    assert done.returncode == 0, done.stderr
    return exe


@functools.lru_cache(maxsize=None)
def run(commands, sanitize=True):
    """commands: a tuple of strings, the program's command line -> its output lines, the closing line taken off"""
    done = subprocess.run([build(sanitize)] + list(commands), capture_output=True, text=True, timeout=120)
    assert done.returncode == 0, done.stdout[-2000:] + done.stderr[-2000:]
    assert "ERROR" not in done.stderr and "runtime error" not in done.stderr and "FAILED" not in done.stdout, done.stdout[-2000:] + done.stderr[-2000:]
    lines = done.stdout.splitlines()
    assert lines[-1] == "sweep plan check ok"
    return lines[:-1]


def _fields(line):
    return {k: v for k, v in (word.split("=", 1) for word in line.split()[1:] if "=" in word)}


def rows(B, HALF, sanitize=True):
    """{n: (gram, pair, float)} for ROW_NS: gram and pair as sweep_cases.Row lists have them -- (inst, a, b) with the vectors of either
    side -- and float as (i, j) pairs, all in launch order"""
    commands = tuple(str(x) for n in ROW_NS for x in ("rows", B, HALF, n))
    out = {n: ([], [], []) for n in ROW_NS}
    for line in run(commands, sanitize):
        f = {k: tuple(int(x) for x in v.split(",")) for k, v in _fields(line).items()}
        n, kind = f["n"][0], line.split()[0]
        which = out[n][("gram", "pair", "float").index(kind)]
        assert f["row"][0] == len(which)
        if kind == "float":
            which.append((f["i"][0], f["j"][0]))
            continue
        na, nb, diag = f["inst"]
        a0, b0 = (f["bi"][0] * B, f["bj"][0] * B) if kind == "gram" else (f["a0"][0], f["b0"][0])
        if kind == "pair":
            assert (f["na"][0], f["nb"][0]) == (na, nb)
        which.append(((na, nb, bool(diag)), tuple(range(a0, a0 + na)), tuple(range(b0, b0 + nb))))
    return out
