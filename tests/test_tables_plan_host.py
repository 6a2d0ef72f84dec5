"""CPU: kdbplan::tables_layout -- the piece layout kdb_record_tables settles on the host before anything is launched -- built alone from
tests/c/tables_plan_check.cpp with AddressSanitizer + UBSan and run as a program (never loaded into Python); its printed plans against
the window definition of tests/tables_cases.py.  Where this g++ has no sanitizer runtime the program is built plainly."""
import atexit
import functools
import os
import shutil
import subprocess
import tempfile

import pytest

import tables_cases as tc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]
PIECE = 8                                   # (an argument of the layout: the kernel header has the real one)


@functools.lru_cache(maxsize=None)
def program():
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    where = tempfile.mkdtemp(prefix="tables_plan_check_")
    atexit.register(shutil.rmtree, where, ignore_errors=True)
    exe = os.path.join(where, "tables_plan_check")
    src = os.path.join(ROOT, "tests", "c", "tables_plan_check.cpp")
    done = subprocess.run([gxx, "-std=c++17", "-O1", "-g"] + SANITIZE + ["-o", exe, src], capture_output=True, text=True)
    if done.returncode != 0 and "sanitize" in done.stderr:
        done = subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-o", exe, src], capture_output=True, text=True)
    assert done.returncode == 0, done.stderr
    return exe


def run(cases):
    """cases: (k, stride, phase, piece, max_entries, nbytes, offsets) -> per case ("refused", why) or (header fields, [piece fields])"""
    args = []
    for k, stride, phase, piece, max_entries, nbytes, offsets in cases:
        args += ["tables", k, stride, phase, piece, max_entries, nbytes, ",".join(str(o) for o in offsets)]
    done = subprocess.run([program()] + [str(a) for a in args], capture_output=True, text=True, timeout=120)
    assert done.returncode == 0, done.stdout[-2000:] + done.stderr[-2000:]
    assert "ERROR" not in done.stderr and "runtime error" not in done.stderr and "FAILED" not in done.stdout, done.stdout[-2000:] + done.stderr[-2000:]
    lines = done.stdout.splitlines()
    assert lines[-1] == "tables plan check ok"
    out = []
    for line in lines[:-1]:
        words = line.split()
        fields = {a: b for a, b in (w.split("=", 1) for w in words[1:] if "=" in w)}
        if words[0] == "refused":
            out.append(("refused", words[1]))
        elif words[0] == "layout":
            out.append((fields, []))
        else:
            out[-1][1].append({a: int(b) for a, b in fields.items()})
    assert len(out) == len(cases)
    return out


def offsets_of(lengths):
    o = [0]
    for n in lengths:
        o.append(o[-1] + n)
    return o


def expected_pieces(lengths, k, stride, phase, piece):
    o, want, multi = offsets_of(lengths), [], []
    for r, n in enumerate(lengths):
        ph = phase if r == 0 else 0
        starts = tc.window_starts(n, k, stride, ph)
        chunks = [starts[i:i + piece] for i in range(0, len(starts), piece)] or [starts]
        if len(chunks) > 1:
            multi.append(r)
        for i, c in enumerate(chunks):
            want.append({"p": len(want), "rec": r, "first": i * piece, "count": len(c), "at": o[r] + ph + i * piece * stride})
    return want, multi


@pytest.mark.parametrize("k", [1, 3, 4, 6])
def test_layout_is_the_window_definition_cut_into_pieces(k):
    cases, wants = [], []
    for stride in range(1, k + 1):
        for phase in sorted({0, stride - 1}):
            wins = [PIECE - 1, PIECE, PIECE + 1, 2 * PIECE + 1, 1, 3 * PIECE]
            lengths = [0, k - 1, k] + [tc.length_for(w, k, stride) + (j % stride) for j, w in enumerate(wins)] + [0, k + 1]
            lengths[0:0] = [phase + tc.length_for(PIECE + 1, k, stride)] if phase else []           # (a phase is record 0's: give it windows)
            o = offsets_of(lengths)
            cases.append((k, stride, phase, PIECE, 1 << 31, o[-1], o))
            wants.append(expected_pieces(lengths, k, stride, phase, PIECE))
    for (header, pieces), (want, multi) in zip(run(cases), wants):
        assert pieces == want
        assert header["npieces"] == str(len(want)) and header["piece_rec"] == "1"
        assert [int(x) for x in header["multi"].split(",")] == multi and len(multi) >= 3


def test_single_piece_batches_have_no_piece_rec_and_short_records_are_rows_of_their_own():
    k, stride = 3, 3
    lengths = [0, 2, 3, 12, 1, 3 * PIECE + 2, 0]
    o = offsets_of(lengths)
    (header, pieces), = run([(k, stride, 0, PIECE, 1 << 31, o[-1], o)])
    assert header == {"npieces": str(len(lengths)), "multi": "", "piece_rec": "0"}
    assert [(p["rec"], p["count"]) for p in pieces] == [(0, 0), (1, 0), (2, 1), (3, 4), (4, 0), (5, PIECE), (6, 0)]
    # a phase moves record 0's windows alone, and can take its last one away
    (_, a), (_, b) = run([(k, stride, 0, PIECE, 1 << 31, 24, [0, 12, 24]), (k, stride, 2, PIECE, 1 << 31, 24, [0, 12, 24])])
    assert [(p["count"], p["at"]) for p in a] == [(4, 0), (4, 12)] and [(p["count"], p["at"]) for p in b] == [(3, 2), (4, 12)]


@pytest.mark.parametrize("stride", [1, 2, 3])
def test_layout_edges(stride):
    k = 3
    edges = tc.layout_edges(k, stride, PIECE)
    got = run([(k, stride, phase, PIECE, 1 << 31, sum(lens), offsets_of(lens)) for lens, phase, _ in edges])
    for (lens, phase, windows), (header, pieces) in zip(edges, got):
        want, multi = expected_pieces(lens, k, stride, phase, PIECE)
        assert pieces == want, (lens, phase)
        assert [sum(p["count"] for p in pieces if p["rec"] == r) for r in range(len(lens))] == windows, (lens, phase)
        assert multi == [r for r, n in enumerate(windows) if n > PIECE]
        assert header == {"npieces": str(len(lens) + len(multi)), "multi": ",".join(str(r) for r in multi), "piece_rec": "1" if multi else "0"}


def test_refusals():
    got = run([(3, 3, 0, PIECE, 1 << 31, 9, [1, 9]),                # does not start at 0
               (3, 3, 0, PIECE, 1 << 31, 9, [0, 8]),                # does not end at nbytes
               (3, 3, 0, PIECE, 1 << 31, 9, [0, 6, 5, 9]),          # falls
               (3, 3, 0, PIECE, 1 << 31, 9, [0, 12, 9]),            # passes nbytes on the way
               (6, 1, 0, PIECE, 1 << 13, 0, [0, 0, 0]),             # 2 x 4^6 entries, 2^13 allowed: the cap is met
               (6, 1, 0, PIECE, 1 << 13, 0, [0, 0, 0, 0]),          # ... and passed
               (1, 1, 0, PIECE, 7, 0, [0, 0]),
               (1, 1, 0, PIECE, 7, 0, [0, 0, 0]),
               (3, 3, 0, PIECE, 1 << 31, 9, [1, 12, 8]),            # starts past 0, ends before nbytes and falls: the ends are named
               (1, 1, 0, PIECE, 7, 0, [0, 1, 0, 0]),                # rises past nbytes, and too many entries: the offsets are named
               (1, 1, 0, PIECE, 7, 0, [0, 0, 0, 1])])
    assert [g if g[0] == "refused" else "ok" for g in got] == [("refused", "ends"), ("refused", "ends"), ("refused", "rise"), ("refused", "rise"), "ok",
                                                               ("refused", "entries"), "ok", ("refused", "entries"), ("refused", "ends"),
                                                               ("refused", "rise"), ("refused", "ends")]
