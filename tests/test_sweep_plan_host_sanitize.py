"""The host plans of the analysis calls (kdb_sweep_plan.cpp.h: the rows and groups of kdb_gram, kdb_pairstats and kdb_pairfloat, the grid of
a sweep, the pieces of kdb_score_reads) under AddressSanitizer + UBSan on the CPU, driven by a stand-alone program that proves the plans'
own invariants and prints them; what it prints is compared with the model the GPU tests place their values by (tests/sweep_cases.py) and,
for the score layout, with the layout computed here."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import score_cases  # noqa: E402
import sweep_cases as sc  # noqa: E402
import sweep_plan_program as prog  # noqa: E402
import test_sweep_cases_cpu as cpu  # noqa: E402

PIECE = sc.header_constant("KDB_SCORE_PIECE")


@pytest.fixture(scope="module", autouse=True)
def _sanitized_program():
    try:
        prog.build(True)
    except prog.NoCompiler as e:
        pytest.skip(str(e))


def test_rows_and_groups_are_the_models_under_asan_ubsan():
    got = prog.rows(sc.B, sc.HALF)
    assert sorted(got) == list(range(1, 18)) + [64]
    for n, (gram, pair, flt) in got.items():
        assert gram == [tuple(r) for r in sc.gram_rows(n)], n
        assert pair == [tuple(r) for r in sc.pair_rows(n)], n
        assert flt == [(i, j) for i in range(n) for j in range(i + 1, n)], n


def _map_cases():
    marks = [m for m in cpu.test_the_map_is_the_kernels_loop.pytestmark if m.name == "parametrize"]
    return list(marks[0].args[1])


def test_grid_triples_are_the_layouts():
    cases = _map_cases()
    assert len(cases) == 10
    caps = (sc.GRID_MAX, sc.GRID_MAX_MANY, sc.FLOAT_GRID_MAX, sc.SF_GRID_MAX)
    cases += [(sc.deep_nbins(cap), cap, cap != sc.SF_GRID_MAX) for cap in caps]
    cases.append((sc.deep_nbins(sc.SF_GRID_MAX), sc.SF_GRID_MAX, True))
    commands = tuple(str(x) for nbins, cap, tail in cases for x in ("grid", nbins, sc.CHUNK, sc.WAVES, cap, int(tail)))
    lines = prog.run(commands)
    assert len(lines) == len(cases)
    for (nbins, cap, tail), line in zip(cases, lines):
        lay = sc.Layout(nbins, cap, tail)
        assert line == "grid nbins=%d cap=%d tail=%d: nchunks=%d gx=%d nparts=%d" % (nbins, cap, int(tail), lay.nchunks, lay.gx, lay.nparts)


def test_the_cap_is_chosen_by_the_rows():
    counts = (1, sc.MANY_ROWS - 1, sc.MANY_ROWS, sc.MANY_ROWS + 1, 2080)
    commands = tuple(str(x) for nrows in counts for x in ("cap", nrows, sc.MANY_ROWS, sc.GRID_MAX, sc.GRID_MAX_MANY))
    assert prog.run(commands) == ["cap nrows=%d: %d" % (nrows, sc.grid_cap(nrows)) for nrows in counts]


def _layout(offs, nbytes, k, continues):
    """the answer of kdb_score_reads' layout, computed directly"""
    nreads = len(offs) - 1
    if offs[0] != 0 or offs[-1] != nbytes:
        return " error=ends"
    if any(offs[r + 1] < offs[r] or offs[r + 1] > nbytes for r in range(nreads)):
        return " error=rise"
    lens = [offs[r + 1] - offs[r] for r in range(nreads)]
    nshort = sum(1 for r, n in enumerate(lens) if n < k and not (r == 0 and continues))
    pieces = [score_cases.pieces_of(max(0, n - k + 1), PIECE) for n in lens]
    rec_piece0 = [sum(pieces[:r]) for r in range(nreads + 1)]
    piece_rec = [] if nshort or sum(pieces) == nreads else [r for r, p in enumerate(pieces) for _ in range(p)]
    csv = lambda v: ",".join(str(x) for x in v)
    return " nshort=%d npieces=%d rec_piece0=%s piece_rec=%s" % (nshort, sum(pieces), csv(rec_piece0), csv(piece_rec))


def _offsets(lens):
    return [sum(lens[:r]) for r in range(len(lens) + 1)]


def _answers(cases):
    """the program's answers to (k, continues, nbytes, offsets), each the layout computed here"""
    commands = tuple(str(x) for k, cont, nbytes, offs in cases for x in ("score", k, PIECE, cont, nbytes, ",".join(str(o) for o in offs)))
    lines = prog.run(commands)
    assert len(lines) == len(cases)
    answers = []
    for (k, cont, nbytes, offs), line in zip(cases, lines):
        head, _, answer = line.partition(":")
        assert head == "score k=%d continues=%d nbytes=%d offs=%s" % (k, cont, nbytes, ",".join(str(o) for o in offs))
        assert answer == _layout(offs, nbytes, k, bool(cont)), head
        answers.append(answer)
    return answers


def test_score_layouts_and_refusals():
    cases = []                                         # (k, continues, nbytes, offsets)
    for k in (1, 3, 12):
        offs = _offsets(score_cases.length_ladder(k, PIECE))
        cases.append((k, 0, offs[-1], offs))
    cases.append((3, 0, 10, _offsets([5, 0, 5])))                          # an empty record
    cases.append((3, 0, 9, _offsets([2, 7])))                              # a first record shorter than k ...
    cases.append((3, 1, 9, _offsets([2, 7])))                              # ... that continues an earlier call's
    cases.append((3, 1, 9, _offsets([7, 2])))                              # (only the first may)
    cases.append((3, 0, 9, _offsets([3, 3, 3])))                           # every record one piece: no piece_rec
    cases.append((3, 0, 9, [0, 6, 4, 9]))                                  # offsets that fall
    cases.append((3, 0, 9, [0, 4, 12, 9]))                                 # ... that pass nbytes on the way
    cases.append((3, 0, 9, [0, 4, 8]))                                     # ... that do not end at nbytes
    cases.append((3, 0, 9, [1, 4, 9]))                                     # ... that do not start at 0
    # the cases are what they say
    answers = _answers(cases)
    assert all(" nshort=0 npieces=12 " in a and a.endswith("piece_rec=0,1,2,3,4,5,6,7,7,8,8,8") for a in answers[:3])
    assert answers[3] == " nshort=1 npieces=3 rec_piece0=0,1,2,3 piece_rec="
    assert " nshort=1 " in answers[4] and " nshort=0 " in answers[5] and " nshort=1 " in answers[6]
    assert answers[7] == " nshort=0 npieces=3 rec_piece0=0,1,2,3 piece_rec="
    assert answers[8:] == [" error=rise", " error=rise", " error=ends", " error=ends"]


def test_score_layout_edges():
    k = 3
    edges = score_cases.layout_edges(k, PIECE)
    cases = [(k, int(cont), sum(lens), _offsets(lens)) for lens, cont, _, _ in edges]
    cases.append((k, 0, 9, [1, 12, 8]))                                    # starts past 0, ends before nbytes and falls: the ends are named
    answers = _answers(cases)
    csv = lambda v: ",".join(str(x) for x in v)
    for (lens, cont, nshort, pieces), answer in zip(edges, answers):
        piece_rec = [r for r, n in enumerate(pieces) for _ in range(n)] if nshort == 0 and max(pieces) > 1 else []
        assert answer == " nshort=%d npieces=%d rec_piece0=%s piece_rec=%s" % (nshort, sum(pieces), csv(_offsets(pieces)), csv(piece_rec)), lens
    assert answers[-1] == " error=ends"
