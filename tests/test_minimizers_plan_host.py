"""CPU: kdbplan::minimizers_layout -- the piece layout kdb_minimizers settles on the host before anything is launched -- built alone from
tests/c/minimizers_plan_check.cpp with AddressSanitizer + UBSan and run as a program (never loaded into Python); its printed plans
against the definition.  Where this g++ has no sanitizer runtime the program is built plainly."""
import atexit
import functools
import os
import shutil
import subprocess
import tempfile

import pytest

import minimizer_cases as mc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]
PIECE = 8                                   # (an argument of the layout: the header has the real one)


@functools.lru_cache(maxsize=None)
def program():
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    where = tempfile.mkdtemp(prefix="minimizers_plan_check_")
    atexit.register(shutil.rmtree, where, ignore_errors=True)
    exe = os.path.join(where, "minimizers_plan_check")
    src = os.path.join(ROOT, "tests", "c", "minimizers_plan_check.cpp")
    done = subprocess.run([gxx, "-std=c++17", "-O1", "-g"] + SANITIZE + ["-o", exe, src], capture_output=True, text=True)
    if done.returncode != 0 and "sanitize" in done.stderr:
        done = subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-o", exe, src], capture_output=True, text=True)
    assert done.returncode == 0, done.stderr
    return exe


def run(cases):
    """cases: (k, w, piece, nbytes, offsets) -> per case ("refused", why) or (header fields, [piece fields])"""
    args = []
    for k, w, piece, nbytes, offsets in cases:
        args += ["minimizers", k, w, piece, nbytes, ",".join(str(o) for o in offsets)]
    done = subprocess.run([program()] + [str(a) for a in args], capture_output=True, text=True, timeout=120)
    assert done.returncode == 0, done.stdout[-2000:] + done.stderr[-2000:]
    assert "ERROR" not in done.stderr and "runtime error" not in done.stderr and "FAILED" not in done.stdout, done.stdout[-2000:] + done.stderr[-2000:]
    lines = done.stdout.splitlines()
    assert lines[-1] == "minimizers plan check ok"
    out = []
    for line in lines[:-1]:
        words = line.split()
        fields = {a: int(b) for a, b in (x.split("=", 1) for x in words[1:])} if words[0] != "refused" else {}
        if words[0] == "refused":
            out.append(("refused", words[1]))
        elif words[0] == "layout":
            out.append((fields, []))
        else:
            out[-1][1].append(fields)
    assert len(out) == len(cases)
    return out


def offsets_of(lengths):
    o = [0]
    for n in lengths:
        o.append(o[-1] + n)
    return o


def expected_pieces(lengths, k, w, piece):
    want = []
    for r, n in enumerate(lengths):
        nwin = max(0, n - k + 1)
        firsts = list(range(0, nwin, piece)) or [0]
        for first in firsts:
            count = min(piece, nwin - first)
            lo, hi = (max(0, first - (w - 1)), min(nwin, first + count + w - 1)) if count else (first, first)
            want.append({"p": len(want), "rec": r, "first": first, "count": count, "lo": lo, "hi": hi})
    return want


@pytest.mark.parametrize("k,w", [(1, 1), (3, 2), (5, PIECE), (4, PIECE + 1), (31, 3), (2, 3 * PIECE)])
def test_layout_is_the_definition_cut_into_pieces(k, w):
    lengths = mc.ladder_lengths(k, w, PIECE) + [0, mc.length_for(5 * PIECE + 3, k), k]
    o = offsets_of(lengths)
    (header, pieces), = run([(k, w, PIECE, o[-1], o)])
    want = expected_pieces(lengths, k, w, PIECE)
    assert pieces == want
    keys = max(p["hi"] - p["lo"] for p in want)
    assert header["npieces"] == len(want) > len(lengths) and header["piece_rec"] == 1 and header["max_keys"] == keys
    assert 9 * keys + k <= header["lds_wave"] <= 9 * keys + k + 16


def test_single_piece_batches_have_no_piece_rec_and_the_lds_follows_the_batch():
    lengths = [0, 2, 3, 9, 1, PIECE + 2, 0]
    o = offsets_of(lengths)
    (header, pieces), = run([(3, 4, PIECE, o[-1], o)])
    assert header["npieces"] == len(lengths) and header["piece_rec"] == 0 and header["max_keys"] == PIECE
    assert [(p["rec"], p["count"]) for p in pieces] == [(0, 0), (1, 0), (2, 1), (3, 7), (4, 0), (5, PIECE), (6, 0)]
    (short, _), (empty, _) = run([(3, 200, PIECE, 10, [0, 5, 10]), (3, 200, PIECE, 0, [0, 0, 0])])
    assert short["max_keys"] == 3 and empty["max_keys"] == 0 and empty["npieces"] == 2


def test_the_real_piece_and_the_widest_window():
    P, w, k = 2048, 256, 31
    n = mc.length_for(3 * P, k)
    (header, pieces), = run([(k, w, P, n, [0, n])])
    assert [(p["lo"], p["hi"]) for p in pieces] == [(0, P + 255), (P - 255, 2 * P + 255), (2 * P - 255, 3 * P)]
    assert header["max_keys"] == P + 510 and 2 * header["lds_wave"] <= 64 * 1024


@pytest.mark.parametrize("k,w", [(3, 1), (3, 4), (2, PIECE + 1)])
def test_layout_edges(k, w):
    edges = mc.layout_edges(k, PIECE)
    got = run([(k, w, PIECE, sum(lens), offsets_of(lens)) for lens, _ in edges])
    for (lens, windows), (header, pieces) in zip(edges, got):
        want = expected_pieces(lens, k, w, PIECE)
        assert pieces == want, lens
        assert [sum(p["count"] for p in pieces if p["rec"] == r) for r in range(len(lens))] == windows, lens
        cut = sum(1 for n in windows if n > PIECE)
        assert header["npieces"] == len(lens) + cut and header["piece_rec"] == (1 if cut else 0), lens
        assert header["max_keys"] == max(p["hi"] - p["lo"] for p in want) <= PIECE + 2 * (w - 1), lens


def test_refusals():
    got = run([(3, 2, PIECE, 9, [1, 9]),                # does not start at 0
               (3, 2, PIECE, 9, [0, 8]),                # does not end at nbytes
               (3, 2, PIECE, 9, [0, 6, 5, 9]),          # falls
               (3, 2, PIECE, 9, [0, 12, 9]),            # passes nbytes on the way
               (3, 2, PIECE, 9, [0, 9]),
               (3, 2, PIECE, 9, [1, 12, 8])])           # starts past 0, ends before nbytes and falls: the ends are named
    assert [g if g[0] == "refused" else "ok" for g in got] == [("refused", "ends"), ("refused", "ends"), ("refused", "rise"), ("refused", "rise"), "ok",
                                                               ("refused", "ends")]
