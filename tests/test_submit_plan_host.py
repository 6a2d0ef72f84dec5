"""CPU: kdbplan::SubmitCutter -- the cut of a submit into staging pieces, settled on the host between the engine's copies -- built alone
from tests/c/submit_plan_check.cpp with AddressSanitizer + UBSan and run as a program (never loaded into Python); its printed pieces
against the rule of tests/submit_cases.py.  Where this g++ has no sanitizer runtime the program is built plainly."""
import atexit
import functools
import os
import random
import shutil
import subprocess
import tempfile

import pytest

import submit_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]
CAP, MAX_RECS, K = 64, 3, 5                 # (arguments of the cut: the engine has the real ones, stage_bytes and stage_reads)


@functools.lru_cache(maxsize=None)
def program():
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    where = tempfile.mkdtemp(prefix="submit_plan_check_")
    atexit.register(shutil.rmtree, where, ignore_errors=True)
    exe = os.path.join(where, "submit_plan_check")
    src = os.path.join(ROOT, "tests", "c", "submit_plan_check.cpp")
    done = subprocess.run([gxx, "-std=c++17", "-O1", "-g"] + SANITIZE + ["-o", exe, src], capture_output=True, text=True)
    if done.returncode != 0 and "sanitize" in done.stderr:
        done = subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-o", exe, src], capture_output=True, text=True)
    assert done.returncode == 0, done.stderr
    return exe


def run(cases):
    """cases: (cap, max_recs, k, first_continues, nbytes, offsets) -> per case (pieces, refusal) as submit_cases.cut gives them, the
    refusal with the program's message behind it"""
    args = []
    for cap, max_recs, k, first_continues, nbytes, offsets in cases:
        args += ["submit", cap, max_recs, k, int(first_continues), nbytes, ",".join(str(o) for o in offsets)]
    done = subprocess.run([program()] + [str(a) for a in args], capture_output=True, text=True, timeout=120)
    assert done.returncode == 0, done.stdout[-2000:] + done.stderr[-2000:]
    assert "ERROR" not in done.stderr and "runtime error" not in done.stderr and "FAILED" not in done.stdout, done.stdout[-2000:] + done.stderr[-2000:]
    lines = done.stdout.splitlines()
    assert lines[-1] == "submit plan check ok"
    out = []
    for line in lines[:-1]:
        words = line.split(None, 1)
        if words[0] == "submit":
            out.append([[], None])
        elif words[0] == "refused":
            kind, at, text = words[1].split(None, 2)
            out[-1][1] = (kind, int(at.split("=")[1]), text.split("=", 1)[1])
        else:
            assert out[-1][1] is None                       # nothing is cut behind a refusal
            fields = dict(w.split("=", 1) for w in words[1].split())
            piece = {a: int(b) for a, b in fields.items() if a != "local"}
            piece["local"] = [int(x) for x in fields["local"].split(",")]
            out[-1][0].append(piece)
    assert len(out) == len(cases)
    return [(pieces, refusal) for pieces, refusal in out]


def test_edges_of_the_cut():
    edges = sc.edges(CAP, MAX_RECS, K)
    cases = []
    for _, lengths, first, cont, behind, _ in edges:
        offs = sc.offsets_of(lengths, first)
        cases.append((CAP, MAX_RECS, K, cont, offs[-1] + behind, offs))
    for (name, lengths, first, cont, _, want), (pieces, refusal) in zip(edges, run(cases)):
        offs = sc.offsets_of(lengths, first)
        assert refusal is None, name
        assert [(p["nbytes"], p["nrecs"], p["cont"], p["inside"]) for p in pieces] == want, name
        assert pieces == sc.cut(offs, cont, CAP, MAX_RECS, K)[0], name
        assert pieces[0]["start"] == first, name
        sc.check_pieces(offs, cont, pieces, CAP, MAX_RECS, K)
    # the rest of a tiled record carries the short records behind it: a piece that begins inside a record, which the engine never
    # appends to its accumulated batch
    joined = run([(CAP, MAX_RECS, K, 0, CAP + 1 + 2 * K, sc.offsets_of([CAP + 1, K, K]))])[0][0][1]
    assert (joined["cont"], joined["inside"], joined["nrecs"], joined["local"]) == (1, 0, 3, [0, K, 2 * K, 3 * K])


def test_refusals_and_what_was_cut_before_them():
    cases = sc.refusals(CAP, MAX_RECS, K)
    got = run([(CAP, MAX_RECS, K, 0, nbytes, offs) for offs, nbytes, _, _ in cases])
    for (offs, nbytes, before, (kind, at)), (pieces, refusal) in zip(cases, got):
        text = sc.ENDS_TEXT if kind == "ends" else sc.RISE_TEXT.format(at)
        assert refusal == (kind, at, text), offs
        assert len(pieces) == before and (pieces, (kind, at)) == sc.cut(offs, 0, CAP, MAX_RECS, K, nbytes), offs


@pytest.mark.parametrize("cap,max_recs,k", [(64, 3, 5), (64, 1, 5), (33, 4, 11), (16, 1000, 1), (24, 2, 24)])
def test_random_submits_are_cut_by_the_rule(cap, max_recs, k):
    rng = random.Random(cap * 1000 + max_recs * 10 + k)
    submits = []
    for _ in range(60):
        lengths = [rng.choice([0, 1, k - 1, k, k + 1, cap // 3, cap - 1, cap, cap + 1, 2 * cap - k + 1, 2 * cap - k + 2, 3 * cap + 2])
                   for _ in range(rng.randint(1, 9))]
        cont = rng.random() < 0.3
        submits.append((sc.offsets_of(lengths, rng.choice([0, 0, 7])), cont))
    got = run([(cap, max_recs, k, cont, offs[-1], offs) for offs, cont in submits])
    for (offs, cont), (pieces, refusal) in zip(submits, got):
        assert refusal is None and pieces == sc.cut(offs, cont, cap, max_recs, k)[0], (offs, cont)
        sc.check_pieces(offs, cont, pieces, cap, max_recs, k)
