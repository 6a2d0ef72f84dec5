"""tests/sweep_cases.py proven on the CPU: the layout model agrees with the kernels' loops written out, the row grouping with the
host code's (run on the CPU), every case is where it claims to be, and the expected integers agree between two formulations.  No GPU."""
import itertools
import os
import re
import shutil
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sweep_cases as sc  # noqa: E402
import sweep_plan_program as prog  # noqa: E402

ROOT = sc.ROOT
TOP = sc.TOP
WIDE = 2 ** 32


# the files that hold the host code of the analysis sweeps: the entry points, their plans, and the engine they left (with the headers its
# host code is split into)
HOST_FILES = ("kdb_analysis_host.hip.h", "kdb_sweep_plan.cpp.h", "kdb_hostutil.hip.h", "kdb_engine.hip", "kdb_io_abi.hip.h", "kdb_probe_host.hip.h",
              "kdb_engine_options.hip.h", "kdb_submit_plan.cpp.h")


def _host_rows():
    """{n: (gram rows, pair rows, float rows)} printed by tests/c/sweep_plan_check.cpp from the plan header the entry points use; under the
    sanitizers where this g++ has them (tests/test_sweep_plan_host_sanitize.py is about that), plainly where not"""
    try:
        return prog.rows(sc.B, sc.HALF)
    except prog.NoCompiler as e:
        if shutil.which("g++") is None:
            pytest.skip(str(e))
        return prog.rows(sc.B, sc.HALF, sanitize=False)


# ---- the constants, the map and the grouping ----

def test_the_grid_caps_are_the_headers_and_the_host_code_uses_them():
    from kmerdb_amd import _abi
    for name in ("KDB_GRAM_GRID_MAX", "KDB_GRAM_GRID_MAX_MANY_ROWS", "KDB_GRAM_GRID_MANY_ROWS", "KDB_PAIRFLOAT_GRID_MAX", "KDB_SIZEFACTORS_GRID_MAX"):
        assert getattr(_abi, name) == sc.header_constant(name)
    assert (sc.GRID_MAX, sc.GRID_MAX_MANY, sc.MANY_ROWS, sc.FLOAT_GRID_MAX, sc.SF_GRID_MAX) == (1024, 256, 4, 512, 1024)
    host = "".join(open(os.path.join(ROOT, "kmerdb_amd", "csrc", f)).read() for f in HOST_FILES)
    assert not re.search(r"1024u\s*:\s*256u|wg_chunks,\s*512u", host)
    for name in ("KDB_GRAM_GRID_MAX", "KDB_GRAM_GRID_MAX_MANY_ROWS", "KDB_GRAM_GRID_MANY_ROWS", "KDB_PAIRFLOAT_GRID_MAX"):
        assert re.search(r"\b%s\b" % name, host), name
    kernels = open(os.path.join(ROOT, "kmerdb_amd", "csrc", "kdb_sizefactors.hip.h")).read()
    assert re.search(r"static_assert\([^;]*MAX_GRID == KDB_SIZEFACTORS_GRID_MAX", kernels)
    assert (sc.deep_nbins(sc.GRID_MAX), sc.deep_nbins(sc.GRID_MAX_MANY), sc.deep_nbins(sc.FLOAT_GRID_MAX)) == (524877, 131661, 262733)


def _loops_written_out(nchunks, gx):
    """{chunk: (workgroup, wave, iteration)} by running every wave's loop as the kernels write it"""
    out = {}
    for wg in range(gx):
        for wave in range(sc.WAVES):
            chunk, it = wg * sc.WAVES + wave, 0
            while chunk < nchunks:
                assert chunk not in out
                out[chunk] = (wg, wave, it)
                chunk += gx * sc.WAVES
                it += 1
    return out


@pytest.mark.parametrize("nbins,cap,tail", [(1, 4, True), (127, 4, True), (128, 4, True), (77 + 128 * 9, 2, True), (77 + 128 * 9, 2, False), (128 * 23, 3, False),
                                            (sc.deep_nbins(5), 5, True), (sc.deep_nbins(5), 5, False), (sc.STRIDE_NBINS, sc.GRID_MAX_MANY, True),
                                            (sc.SF_NBINS, sc.SF_GRID_MAX, False)])
def test_the_map_is_the_kernels_loop(nbins, cap, tail):
    lay = sc.Layout(nbins, cap, tail)
    assert lay.gx == max(1, min(-(-lay.nchunks // 4), cap)) and lay.nparts == lay.gx + 1
    loops = _loops_written_out(lay.nchunks, lay.gx)
    assert sorted(loops) == list(range(lay.nchunks))                       # every chunk once
    assert lay.iterations == max([it for _, _, it in loops.values()] + [0]) + 1
    step = max(1, nbins // 4000)
    for b in itertools.chain(range(0, nbins, step), range(max(0, nbins - 300), nbins)):
        w = lay.where(b)
        if w is None:
            assert tail and b >= (nbins // 128) * 128
            continue
        assert (w.workgroup, w.wave, w.iteration) == loops[w.chunk] and w.chunk * 128 + 2 * w.lane + w.half == b
        assert lay.bin(w.iteration, w.workgroup, w.wave, w.lane, w.half) == b
        assert lay.iteration_of([b])[0] == w.iteration
    if not tail:
        assert lay.where(nbins - 1) is not None and lay.body == nbins
    assert all(lay.where(int(b)).iteration >= 1 for b in lay.second_stride()[:: 7])
    assert lay.second_stride().size == max(0, lay.body - 4 * lay.gx * 128)


@pytest.mark.parametrize("n", list(range(1, 18)) + [64])
def test_every_pair_has_one_row_and_its_instantiation(n):
    g, p = sc.gram_rows(n), sc.pair_rows(n)
    host_gram, host_pair, _ = _host_rows()[n]          # what the host code's own plan gives (kdb_sweep_plan.cpp.h, run on the CPU)
    assert [tuple(r) for r in g] == host_gram
    assert [tuple(r) for r in p] == host_pair
    nblk = -(-n // 4)
    assert len(g) == nblk * (nblk + 1) // 2
    assert len(p) == nblk + sum(bj * -(-min(4, n - 4 * bj) // 2) for bj in range(1, nblk))
    for rows, served in ((g, sc.gram_served), (p, sc.pair_served)):
        for row in rows:
            na, nb, diag = row.inst
            assert (len(row.a), len(row.b)) == (na, nb) and (row.a == row.b) == diag
            assert diag or (na == 4 and row.a[-1] < row.b[0])
        for i in range(n):
            for j in range(i + 1, n):
                s = served(n, i, j)
                assert rows[s.row].a[s.slot[0]] == i and rows[s.row].b[s.slot[1]] == j
                assert s.inst[2] == (i // 4 == j // 4)
    for row in p:
        assert row.inst[2] or row.inst[1] <= sc.HALF
    # off the diagonal kdb_gram takes the second block in passes of two, or of one where all four are there
    for i in range(min(n, 4)):
        for j in range(4, n):
            s = sc.gram_served(n, i, j)
            nb = s.inst[1]
            want = (s.slot[1], 1) if nb == 4 else ((0, min(nb, 2)) if s.slot[1] < 2 else (2, nb - 2))
            assert s.passes == want and s.passes[0] <= s.slot[1] < s.passes[0] + s.passes[1]


def test_the_row_counts_choose_the_caps_the_cases_rely_on():
    for n in sc.GUARD_NS:
        assert len(sc.gram_rows(n)) == 3 < sc.MANY_ROWS
    for n in sc.STRIDE_NS:
        assert len(sc.gram_rows(n)) >= sc.MANY_ROWS and len(sc.pair_rows(n)) >= sc.MANY_ROWS
    assert len(sc.pair_rows(7)) == 4 and len(sc.pair_rows(6)) == 3 and len(sc.pair_rows(2)) == len(sc.gram_rows(2)) == 1


# ---- two formulations of the expected integers ----

def _loops_gram(vs):
    ints = [[int(x) for x in v] for v in vs]
    return [sum(r) for r in ints], [[sum(p * q for p, q in zip(a, b)) for b in ints] for a in ints]


def _loops_pair(vs):
    ints = [[int(x) for x in v] for v in vs]
    n = len(vs)
    out = {"S": [sum(r) for r in ints], "nnz": [sum(1 for x in r if x) for r in ints]}
    for key in ("L1", "Linf", "ne", "both"):
        out[key] = [[0] * n for _ in range(n)]
    for i in range(n):
        for j in range(n):
            d = [abs(p - q) for p, q in zip(ints[i], ints[j])]
            out["L1"][i][j], out["Linf"][i][j], out["ne"][i][j] = sum(d), max(d), sum(1 for x in d if x)
            out["both"][i][j] = sum(1 for p, q in zip(ints[i], ints[j]) if p and q)
    return out


def test_the_limb_formulation_is_plain_python_on_edge_values():
    rng = np.random.default_rng(1)
    edge = np.array([0, 1, 2 ** 16 - 1, 2 ** 16, 2 ** 32 - 1, 2 ** 32, 2 ** 48 + 12345, 2 ** 63, TOP, TOP - 1], dtype=np.uint64)
    vs = [rng.choice(edge, 300) for _ in range(5)] + [np.full(300, TOP, dtype=np.uint64), np.zeros(300, dtype=np.uint64)]
    assert sc.gram_expected(vs) == _loops_gram(vs) == sc._tg._expected(vs)
    assert sc.pair_expected(vs) == _loops_pair(vs) == sc._tp._expected(vs)


# ---- a. the guard ----

@pytest.mark.parametrize("n", sc.GUARD_NS)
def test_guard_case_one_wide_value_per_wave_in_every_vector_and_half(n):
    vs, placed = sc.gram_guard_case(n)
    nbins = vs[0].size
    lay = sc.gram_layout(n, nbins)
    assert nbins == (2 * n + 4) * 128 + 77 and lay.nchunks == 2 * n + 4 and lay.iterations == 1 and lay.gx == -(-(2 * n + 4) // 4)
    assert sorted((v, h) for v, h, _ in placed) == [(v, h) for v in range(n) for h in (0, 1)]
    wide = np.stack([v >= WIDE for v in vs])                               # [vector, bin]
    per_chunk = wide[:, :lay.body].reshape(n, lay.nchunks, 128).sum(axis=(0, 2))
    assert not wide[:, lay.body:].any()                                    # the tail is small
    chunks = set()
    for v, half, b in placed:
        w = lay.where(b)
        assert w.half == half and w.lane != 0 and per_chunk[w.chunk] == 1 and wide[v, b] and int(vs[v][b]) == sc.GUARD_VALUE
        assert all(0 < int(vs[u][b]) < 16 for u in range(n) if u != v)     # the others: small and not zero, so 32 bits of the value change G
        chunks.add(w.chunk)
    assert len(chunks) == 2 * n and int(per_chunk.sum()) == 2 * n          # a wave each; the other four waves take the short multiply
    S, G = sc.gram_expected(vs)
    assert (S, G) == sc._tg._expected(vs) == _loops_gram(vs) and max(S) < 2 ** 64
    # what a wave that took the 32-bit multiply at one placed bin would have added differs in every pair with that vector
    for v, _, b in placed:
        for u in range(n):
            assert (int(vs[v][b]) % WIDE) * (int(vs[u][b]) % WIDE) != int(vs[v][b]) * int(vs[u][b])
    # the roles: every (vector, half) of both sides of <4,1..4,false>, and every diagonal block size
    insts = {r.inst for r in sc.gram_rows(n)}
    assert insts == {(4, 4, True), (n - 4, n - 4, True), (4, n - 4, False)}


def test_guard_cases_reach_every_instantiation():
    insts = set().union(*[{r.inst for r in sc.gram_rows(n)} for n in sc.GUARD_NS])
    assert insts == {(k, k, True) for k in (1, 2, 3, 4)} | {(4, k, False) for k in (1, 2, 3, 4)}


# ---- b. across the stride ----

@pytest.fixture(scope="module")
def stride_cases():
    return {n: sc.stride_case(n) for n in sc.STRIDE_NS}


def test_stride_cases_shape_and_values(stride_cases):
    for n, (vs, classes, (p0, p0b, p1)) in stride_cases.items():
        nbins = vs[0].size
        for lay in (sc.gram_layout(n, nbins), sc.pair_layout(n, nbins)):
            assert nbins == sc.GRID_MAX_MANY * 512 + 512 + 77 and lay.nparts == 257 and lay.iterations == 2 and lay.nbins - lay.body == 77
            w0, w0b, w1 = lay.where(p0), lay.where(p0b), lay.where(p1)
            assert (w0.iteration, w0b.iteration, w1.iteration) == (0, 0, 1) and w1.workgroup == 0 and 0 not in (w0.workgroup, w0b.workgroup)
            assert 0 not in (w0.lane, w0b.lane, w1.lane) and len({w0.workgroup, w0b.workgroup}) == 2
            second = lay.second_stride()
            assert second.size == 512 and all(lay.where(int(b)).workgroup == 0 for b in second[:: 128])       # some workgroups two iterations, the others one
        assert "late" in classes and "zeros" in classes and set(classes) <= set(sc.CLASSES)
        for v, cls in zip(vs, classes):
            s = int(v.astype(object).sum())
            assert s < 2 ** 63 and int(v.max()) < 2 ** 62
            nz = np.flatnonzero(v)
            if cls == "zeros":
                assert nz.size == 0
            elif cls == "late":
                assert nz.size == 512 and set(lay.iteration_of(nz).tolist()) == {1}         # its only non-zero bins: second-iteration bins
            else:
                assert set(lay.iteration_of(nz).tolist()) == {-1, 0, 1} and v[p0] >= WIDE and v[p0b] >= 2 ** 61 and v[p1] >= 2 ** 61
            if cls in ("big32", "big32b"):
                assert int(np.count_nonzero(v == WIDE - 1)) > nbins // 3 and int(np.count_nonzero(v >= WIDE)) == 3
    assert {c for _, classes, _ in stride_cases.values() for c in classes} == set(sc.CLASSES)


def test_stride_cases_every_off_diagonal_slot_meets_wide_operands_and_carries_in_both_iterations(stride_cases):
    """per (sweep, instantiation, slot): a row at some n whose pair meets, in one lane other than lane 0, a 64-bit operand against a
    non-zero one, a sum of 2^64 or more in the first iteration, and again from the second iteration's bins alone; and a non-zero
    contribution from workgroup 0's first iteration, which a reset inside the chunk loop would lose"""
    met = {}
    for n, (vs, classes, (p0, p0b, p1)) in stride_cases.items():
        lay = sc.gram_layout(n, vs[0].size)
        first_of_wg0 = slice(0, 512)
        for sweep, rows in (("gram", sc.gram_rows(n)), ("pairstats", sc.pair_rows(n))):
            for row in rows:
                if row.inst[2]:
                    continue
                for ia, i in enumerate(row.a):
                    for jb, j in enumerate(row.b):
                        x, y = vs[i], vs[j]
                        ok = (int(x[p0]) >= WIDE and int(y[p0]) >= WIDE                       # 64-bit operands on both sides
                              and int(x[p0b]) * int(y[p0b]) >= 2 ** 64 and lay.where(p0b).iteration == 0
                              and int(x[p1]) * int(y[p1]) >= 2 ** 64 and lay.where(p1).iteration == 1
                              and int(np.dot(x[first_of_wg0].astype(object), y[first_of_wg0].astype(object))) > 0
                              and bool(np.any(x[first_of_wg0] != y[first_of_wg0])))
                        key = (sweep, row.inst, ia, jb)
                        met[key] = met.get(key, False) or ok
    want = {("gram", (4, nb, False), i, j) for nb in (1, 2, 3, 4) for i in range(4) for j in range(nb)}
    want |= {("pairstats", (4, nb, False), i, j) for nb in (1, 2) for i in range(4) for j in range(nb)}
    assert set(met) == want
    assert all(met.values()), sorted(k for k, v in met.items() if not v)


def test_stride_cases_expected_integers_in_two_formulations(stride_cases):
    for n in (sc.STRIDE_NS[0], sc.STRIDE_NS[-1]):
        vs = stride_cases[n][0]
        S, G = sc.gram_expected(vs)
        assert (S, G) == sc._tg._expected(vs) and max(S) < 2 ** 64
        assert sc.pair_expected(vs) == sc._tp._expected(vs)
        late = stride_cases[n][1].index("late")
        assert max(max(r) for r in G) >= 2 ** 122 and G[late][late] >= 2 ** 122


# ---- c. the carry ladder ----

def _ladder_relation(placement, wa, wb):
    same = lambda *f: all(getattr(wa, k) == getattr(wb, k) for k in f)
    return {"lane": same("chunk", "lane") and (wa.half, wb.half) == (0, 1),
            "iterations": same("workgroup", "wave", "lane") and (wa.iteration, wb.iteration) == (0, 1),
            "lanes": same("chunk") and wa.lane != wb.lane,
            "waves": same("workgroup", "iteration") and wa.wave != wb.wave,
            "workgroups": wa.workgroup != wb.workgroup and wa.iteration == wb.iteration}[placement]


@pytest.mark.parametrize("placement", sc.PLACEMENTS)
@pytest.mark.parametrize("n", sc.LADDER_NS)
def test_ladder_case_meets_where_it_says_in_every_instantiation(n, placement):
    vs, a, b = sc.ladder_case(n, placement)
    nbins = vs[0].size
    lay = sc.pair_layout(n, nbins)
    assert lay.nparts == {7: 257, 6: 1025}[n] and lay.iterations == 2 and nbins == sc.deep_nbins({7: 256, 6: 1024}[n])
    wa, wb = lay.where(a), lay.where(b)
    assert _ladder_relation(placement, wa, wb) and wa.lane != 0 and wb.lane != 0
    assert [p for p in sc.PLACEMENTS if _ladder_relation(p, wa, wb)][0] == placement          # the lowest level at which the two meet
    holders_a, holders_b = [v for v in sc.LADDER_A if v < n], [v for v in sc.LADDER_B if v < n]
    for v in range(n):
        s = int(vs[v].astype(object).sum())
        assert s < 2 ** 64                                                 # no refusal here
        if v in holders_a or v in holders_b:
            assert s == TOP and np.flatnonzero(vs[v]).tolist() == [a if v in holders_a else b]
        else:
            assert 0 < int(vs[v].max()) < 64 and int(vs[v][a]) + int(vs[v][b]) < s
    roles = set()
    for i, j in ((min(p, q), max(p, q)) for p in holders_a for q in holders_b):
        s = sc.pair_served(n, i, j)
        roles.add((s.inst, None if s.inst[2] else s.slot[1]))
    if n == 7:
        assert roles == {((4, 4, True), None), ((3, 3, True), None), ((4, 2, False), 0), ((4, 2, False), 1), ((4, 1, False), 0)}
    else:
        assert roles == {((4, 4, True), None), ((2, 2, True), None), ((4, 2, False), 0), ((4, 2, False), 1)}
    # the expected integers, pair by pair, from the construction: plain Python and int64
    want = sc.pair_expected(vs)
    noise = [v for v in range(n) if v not in holders_a + holders_b]
    for i in range(n):
        for j in range(i + 1, n):
            hi, hj = i not in noise, j not in noise
            if hi and hj:
                apart = (i in holders_a) != (j in holders_a)
                l1, linf, ne, both = (2 ** 65 - 2, TOP, 2, 0) if apart else (0, 0, 0, 1)
            elif hi or hj:
                at = a if (i if hi else j) in holders_a else b
                x = vs[j if hi else i].astype(np.int64)
                l1 = TOP - int(x[at]) + int(x.sum()) - int(x[at])
                linf, ne, both = TOP - int(x[at]), int(np.count_nonzero(x)) + (0 if x[at] else 1), (1 if x[at] else 0)
            else:
                d = np.abs(vs[i].astype(np.int64) - vs[j].astype(np.int64))
                l1, linf, ne = int(d.sum()), int(d.max()), int(np.count_nonzero(d))
                both = int(np.count_nonzero((vs[i] > 0) & (vs[j] > 0)))
            assert (want["L1"][i][j], want["Linf"][i][j], want["ne"][i][j], want["both"][i][j]) == (l1, linf, ne, both), (i, j)
            assert want["L1"][j][i] == l1
    assert any(want["L1"][i][j] >= 2 ** 64 for i in noise for j in holders_a)              # (a noise pair's L1 carries too)
    if n == 7 and placement == "lane":
        assert want == sc._tp._expected(vs)


@pytest.mark.parametrize("placement", sc.REFUSALS)
def test_refusal_case_reaches_two_to_the_64_inside_one_lane(placement):
    vs, (a, b) = sc.refusal_case(placement)
    nbins = vs[0].size
    for lay in (sc.pair_layout(2, nbins), sc.gram_layout(2, nbins)):
        assert lay.nparts == 1025 and lay.iterations == 2
        wa, wb = lay.where(a), lay.where(b)
        assert (wa.workgroup, wa.wave, wa.lane) == (wb.workgroup, wb.wave, wb.lane) and wa.lane != 0
        assert (wa.chunk == wb.chunk) == (placement == "lane") and (wa.iteration, wb.iteration) == ((0, 0) if placement == "lane" else (0, 1))
    assert int(vs[1][a]) == int(vs[1][b]) == 2 ** 63 and int(np.count_nonzero(vs[1])) == 2         # S = 2^64 exactly: the least refused sum
    assert int(vs[0].astype(object).sum()) == nbins


# ---- d. the float sweep ----

@pytest.mark.parametrize("nbins", [sc.FLOAT_DEEP_NBINS, sc.FLOAT_MID_NBINS])
def test_float_case_lone_words_and_partials(nbins):
    vs, lone = sc.float_case(nbins)
    lay = sc.float_layout(nbins)
    if nbins == sc.FLOAT_DEEP_NBINS:
        assert nbins == sc.FLOAT_GRID_MAX * 512 + 512 + 77 and lay.nparts == 513 and lay.iterations == 2
    else:
        assert 64 < lay.nparts == 101 < 128 and lay.iterations == 1
    assert nbins - lay.body == 77 and sorted(lone) == [(v, h) for v in range(3) for h in (0, 1)]
    assert len({lay.where(b).chunk for b in lone.values()}) == 6
    words = ("x.x", "x.y", "y.x", "y.y")
    for i, j in ((0, 1), (0, 2), (1, 2)):
        seen, iterations = set(), []
        for (v, half), b in lone.items():
            if v not in (i, j):
                continue
            w = lay.where(b)
            x, y = vs[i][lay.chunk_bins(w.chunk)], vs[j][lay.chunk_bins(w.chunk)]
            nonzero = {"x.x": int(np.count_nonzero(x[0::2])), "x.y": int(np.count_nonzero(x[1::2])),
                       "y.x": int(np.count_nonzero(y[0::2])), "y.y": int(np.count_nonzero(y[1::2]))}
            word = ("x" if v == i else "y") + "." + "xy"[half]
            assert nonzero == {k: (1 if k == word else 0) for k in words}, (i, j, v, half)       # exactly one of the four words, in one lane
            assert w.half == half and w.lane != 0
            seen.add(word)
            iterations.append(w.iteration)
        assert seen == set(words)
        assert sorted(iterations) == ([0, 0, 0, 1] if (i, j) != (0, 2) else [0, 0, 1, 1]) if lay.iterations == 2 else set(iterations) == {0}
    # the recipe's properties hold at this length
    assert int(vs[0].max()) == 2 ** 40 and all(0.3 < np.count_nonzero(v) / nbins < 0.7 for v in vs)
    assert 0 < int(np.count_nonzero(vs[1] != vs[2])) <= nbins // 17 + 1
    assert all(int(v.astype(object).sum()) < 2 ** 64 for v in vs)
    assert len(set(zip(vs[0].tolist(), vs[1].tolist()))) < 400             # (the exact references group by distinct pairs)


# ---- e. size factors and scaling ----

@pytest.mark.parametrize("mode", sc.SF_MODES)
def test_grouped_case_deep_has_the_medians_group_beyond_the_first_stride(mode):
    x, y, ts, deep = sc.grouped_case_deep(mode, 2000 + sc.SF_MODES.index(mode))
    nbins = x.size
    lay = sc.sf_layout(nbins)
    assert nbins == sc.SF_GRID_MAX * 512 + 512 + 77 and lay.gx == 1024 and lay.iterations == 2 and lay.body == nbins and lay.nchunks == 4101
    last = lay.where(nbins - 1)
    assert (last.chunk, last.workgroup, last.wave, last.iteration) == (4100, 1, 0, 1)       # the partial chunk goes through the body, in a second iteration
    eligible = (x > 0) & (y > 0)
    m = int(eligible.sum())
    lo, hi = (m - 1) // 2, m // 2
    assert m == len(ts) and ts == sorted(ts) and not eligible[-1] and eligible[0]
    t_of = {8 * 2 ** t if t >= 0 else 8 >> -t: t for t in sc._ts.T_VALUES}
    t = np.array([t_of[int(v)] for v in y[eligible]])
    assert sorted(t.tolist()) == ts                                        # the vector holds the multiset it says
    bins = np.flatnonzero(eligible)
    median_groups = {ts[lo], ts[hi]}
    in_group = np.isin(t, list(median_groups))
    its = lay.iteration_of(bins)
    assert set(its[in_group].tolist()) == {1} and set(its[~in_group].tolist()) == {0}       # the median's group: all of it beyond the first stride, and nothing else there
    assert sorted(bins[in_group].tolist()) == deep.tolist() and deep.size > 300
    assert {lay.where(int(b)).workgroup for b in deep} == {0, 1}           # whole chunks of workgroup 0 and the partial chunk of workgroup 1
    if mode == "first":
        assert ts[lo - 1] < ts[lo] == ts[hi]
    elif mode == "last":
        assert ts[lo] == ts[hi] < ts[hi + 1]
    else:
        assert hi == lo + 1 and ts[lo] < ts[hi]
    assert len(set(ts)) == 4 and int(np.count_nonzero(x == 0)) > nbins // 16 and int(np.count_nonzero(y == 0)) > nbins // 16


def test_scale_case_deep_has_its_edge_values_in_two_second_iteration_chunks():
    v, second = sc.scale_case_deep(9)
    lay = sc.sf_layout(v.size)
    closing = range(v.size - len(sc.SCALE_EDGE), v.size)
    assert [int(v[b]) for b in closing] == list(sc.SCALE_EDGE) == [int(v[b]) for b in second]
    assert {lay.where(b).chunk for b in closing} == {4100} and {lay.where(b).iteration for b in closing} == {1}
    ws = [lay.where(b) for b in second]
    assert {w.iteration for w in ws} == {1} and {w.chunk for w in ws} == {4097} and {w.half for w in ws} == {0, 1} and len({w.lane for w in ws}) == len(ws)
    assert (4097 + 1) * 128 <= v.size                                      # a whole chunk
    assert np.rint(v.astype(np.float64) / 0.75).max() < 2.0 ** 63          # nothing here is refused
    where = sc.overflow_bins()
    assert where["bin 0"] == 0 and where["last bin of the partial chunk"] == v.size - 1
    w = lay.where(where["second iteration"])
    assert w.iteration == 1 and (w.chunk + 1) * 128 <= v.size and w.chunk not in (4097, 4100)
