"""CPU: what the seeded cases of tests/test_gpu_fuzz_records.py are, checked without a device -- for exactly its (call, seed, cases)
triples: the draws are deterministic and legal under the Python wrappers' own validation, the restatements agree with their independent
twins on them, they reach the conditions listed per call below (computed from the restatements alone: where a seed misses one, the
generator or the seed changes, never the condition), and a wrong tie rule in a copy of a restatement shows on them."""
import functools
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import alignment_cases as ac  # noqa: E402
import fuzz_records as fr  # noqa: E402
import minimizer_cases as mc  # noqa: E402
import tables_cases as tb  # noqa: E402
import traceback_cases as tc  # noqa: E402
from test_gpu_fuzz_records import SEEDED, _tiny_tasks, SCAN_TOP, TINY_BAND  # noqa: E402

PLAIN_CELLS = 200000                           # positions x run length up to which select_runs_plain walks a record
MUTATED = 5                                    # the wrong E rule is run on the first MUTATED cases of every (call, seed)


def _of(call):
    return [(seed, index) for c, seed, n in SEEDED if c == call for index in range(n)]


def _equal(a, b):
    if isinstance(a, dict):
        return isinstance(b, dict) and a.keys() == b.keys() and all(_equal(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(_equal(x, y) for x, y in zip(a, b))
    if isinstance(a, np.ndarray):
        return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
    return a == b


@functools.lru_cache(maxsize=None)
def _report(call, seed, index):
    """one case drawn and restated once, and what the tests below ask of it -> a dict of small values (the arrays are let go)"""
    desc, arrays = fr.draw(seed, index, call)
    again = fr.draw(seed, index, call)
    rep = dict(desc=desc, deterministic=_equal((json.loads(json.dumps(desc)), arrays), again), legal=fr.legal(desc, arrays))
    want = fr.want_case(desc, arrays)
    if call == "minimizers":
        k, w, canonical, order = desc["k"], desc["w"], desc["canonical"], desc["order"]
        rep.update(want["stats"])
        rep["twin"], rep["rightmost_differs"], walked = True, False, 0
        for rec, keys in zip(arrays["records"], want["keys"]):
            if keys.size * min(w, keys.size) <= PLAIN_CELLS:
                walked += 1
                rep["twin"] &= mc.select_runs(keys, w).tolist() == mc.select_runs_plain(keys, w)
            # the wrong rule: of every run the RIGHTMOST position holding the smallest key (the leftmost of the reversed keys)
            right = keys.size - 1 - mc.select_runs(keys[::-1], w)[::-1] if keys.size else np.zeros(0, dtype=np.int64)
            rep["rightmost_differs"] |= right.tolist() != mc.select_runs(keys, w).tolist()
        rep["walked"] = walked
    elif call == "tables":
        rep["twin"] = True
        if desc["split"]:
            a, b = want["outs"][1], want["outs"][2]
            rep["twin"] = fr._same_row(fr.join_tables(fr._row(a, len(a[1]) - 1), fr._row(b, 0)), want["whole"])      # the cut and the phase are right
        lens = sorted(set(desc["lens"]))
        block = [r for r in arrays["records"] if len(r) == lens[-1]]          # uniform_tables: written on its own, for records of one length
        uni = tb.uniform_tables(np.array([np.frombuffer(r, dtype=np.uint8) for r in block]).reshape(len(block), lens[-1]), desc["k"], desc["stride"], desc["canonical"])
        rows = [i for i, r in enumerate(arrays["records"]) if len(r) == lens[-1]]
        rep["twin"] &= all(np.array_equal(u, o[rows]) for u, o in zip(uni, want["outs"][0]))
    elif call == "score":
        rep.update(want["stats"])
        rep["twin"] = True
        if desc["split"]:
            a, b, whole = want["outs"][1][-1], want["outs"][2][0], want["whole"]
            rep["twin"] = (a.windows + b.windows, a.zero_windows + b.zero_windows, min(a.min_count, b.min_count)) == (whole.windows, whole.zero_windows, whole.min_count)
        for s in want["outs"][0]:                                             # plain float64 numpy is inside the bound the device is held to
            if s.log10_p is not None and s.log10_p != float("-inf"):
                rep["twin"] &= fr.sc.error(fr.sc.float64_log10_p(s), s) <= fr.sc.bound(s, fr.SCORE_PIECE, fr.SCORE_LANES)
    else:
        band, scores, tasks = desc["band"], desc["scores"], desc["tasks"]
        queries, refs = arrays["queries"], arrays["refs"]
        args = fr.align_args(desc, arrays)
        five, tie_best, decided = fr.banded_batch_ties(*args, band, **scores)
        wrong = fr.banded_batch_ties(*args, band, e_tie_opens=False, **scores)[0] if index < MUTATED else want["five"]
        one = lambda t: (queries[tasks[t][0]], refs[tasks[t][1]], tasks[t][2], band, tasks[t][3])
        rng = np.random.Generator(np.random.PCG64([seed, index, 7]))
        some = sorted(set(rng.integers(0, len(tasks), size=12).tolist()) | set(want["covered"][:12]))
        rep.update(ntasks=len(tasks), zero=int(np.count_nonzero(want["five"][0] == 0)), ties=int(np.count_nonzero(tie_best | decided)),
                   covered=len(want["covered"]), multi_stage=sum(1 for q, _, _, _ in tasks if len(queries[q]) > fr.ALIGN_STAGE), rel=(scores["gap_open"] > scores["gap_extend"]) - (scores["gap_open"] < scores["gap_extend"]),
                   e_rule_differs=fr._five_differ(wrong, want["five"]) is not None,
                   twin=fr._five_differ(five, want["five"]) is None and                                     # the copy that counts the ties is banded_batch
                   all(tuple(int(g[t]) for g in want["five"]) == ac.banded(*one(t), **scores) for t in some) and
                   all(ac.banded(*one(t), **scores) == full for t, full in zip(want["covered"], want["full"])))
        if call == "traceback":
            positive = [t for t in desc["sample"] if want["paths"][t][0][0] > 0]
            rep.update(sampled=len(desc["sample"]), positive=len(positive),
                       gapped=sum(1 for t in positive if any(x & 15 in (tc.OP_I, tc.OP_D) for x in want["paths"][t][1])))
            rep["twin"] &= all(fr.trace_e_rule(*one(t), **scores) == want["paths"][t] for t in desc["sample"])
            rep["twin"] &= all(tc.trace_full(ac.orient(one(t)[0], one(t)[4]), one(t)[1], **scores) == want["paths"][t] for t in desc["sample"] if t in want["covered"])
            if index < MUTATED:
                rep["e_rule_differs"] |= any(fr.trace_e_rule(*one(t), e_tie_opens=False, **scores) != want["paths"][t] for t in desc["sample"])
            rep["limits"] = (desc["scratch_limit"], desc["other_limit"])
    return rep


def _reports(call):
    return [_report(call, seed, index) for seed, index in _of(call)]


def _share(reports, key):
    return sum(1 for r in reports if r[key]) / len(reports)


@pytest.mark.parametrize("call", fr.CALLS)
def test_the_draws_are_deterministic_legal_and_the_restatements_agree_with_their_twins(call):
    for rep in _reports(call):
        where = {k: v for k, v in rep["desc"].items() if k in ("call", "seed", "index")}
        assert rep["deterministic"], where
        assert rep["legal"], where
        assert rep["twin"], where


def test_an_illegal_case_is_not_legal():
    desc, arrays = fr.draw(101, 0, "align")
    with pytest.raises(ValueError):
        fr.legal(dict(desc, band=fr.MAX_BAND + 1), arrays)
    desc, arrays = fr.draw(101, 0, "minimizers")
    with pytest.raises(ValueError):
        fr.legal(dict(desc, w=fr.MIN_MAX_W + 1), arrays)


def test_minimizer_cases_reach_the_pieces_the_wide_windows_and_the_ties():
    reps = _reports("minimizers")
    assert _share(reps, "multi_piece") >= 0.25
    assert sum(1 for r in reps if r["desc"]["w"] > 64) / len(reps) >= 0.25
    assert sum(1 for r in reps if r["desc"]["k"] > 16) / len(reps) >= 0.25
    assert _share(reps, "tied_run") >= 0.25
    for seed in {s for _, s, _ in SEEDED}:
        mine = [r for r in reps if r["desc"]["seed"] == seed]
        assert any(r["one_run"] for r in mine) and any(r["no_key"] for r in mine) and any(r["empty"] for r in mine), seed
    assert sum(r["walked"] for r in reps) >= 100


def test_tables_cases_reach_every_k_the_strides_between_and_the_splits():
    reps = _reports("tables")
    assert {r["desc"]["k"] for r in reps} == set(range(1, 7))
    assert any(1 < r["desc"]["stride"] < r["desc"]["k"] for r in reps)
    assert {r["desc"]["canonical"] for r in reps} == {False, True}
    split = [r["desc"]["split"] for r in reps if r["desc"]["split"]]
    assert len(split) / len(reps) >= 0.2 and any(s["phase"] for s in split)


def test_score_cases_reach_minus_infinity_nan_the_splits_and_the_pieces():
    reps = _reports("score")
    assert _share(reps, "minus_inf") >= 0.2
    assert any(r["nan"] for r in reps)
    assert sum(1 for r in reps if r["desc"]["split"]) / len(reps) >= 0.2
    assert any(r["desc"]["split"] and r["desc"]["split"]["none_scored"] for r in reps)       # a first piece without a scored window
    assert _share(reps, "multi_piece") >= 0.25
    assert {0, 1} < {r["desc"]["pseudocount"] for r in reps}                  # 0, 1 and a large one


@pytest.mark.parametrize("call", ["align", "traceback"])
def test_alignment_cases_reach_the_bands_the_scores_and_the_ties(call):
    reps = _reports(call)
    ntasks = sum(r["ntasks"] for r in reps)
    assert sum(r["zero"] for r in reps) / ntasks <= 1 / 3
    assert sum(r["ties"] for r in reps) / ntasks >= 0.1
    bands = {r["desc"]["band"] for r in reps}
    assert {b & 1 for b in bands} == {0, 1}
    assert {1, fr.MAX_BAND} <= bands and len(bands - {1, fr.MAX_BAND}) >= 20
    assert sum(r["multi_stage"] for r in reps) / ntasks >= 0.01               # queries of more than one KDB_ALIGN_STAGE (they come at bands up to 7 only)
    assert {r["rel"] for r in reps} == {-1, 0, 1}
    assert sum(r["covered"] for r in reps) >= 20
    if call == "traceback":
        assert sum(r["gapped"] for r in reps) / sum(r["positive"] for r in reps) >= 0.2
        assert {x for r in reps for x in r["limits"]} >= {0, 1}


def test_a_wrong_tie_rule_shows_on_the_drawn_cases():
    assert any(r["rightmost_differs"] for r in _reports("minimizers"))
    for call in ("align", "traceback"):
        assert any(r["e_rule_differs"] for r in _reports(call) if r["desc"]["index"] < MUTATED), call


def test_the_tiled_tasks_are_tiny_and_fit_one_chunk():
    queries, refs, tasks = _tiny_tasks()
    sizes = [fr.trace_bytes(len(queries[q]), len(refs[r]), d, TINY_BAND) for q, r, d, _ in tasks]
    assert max(sizes) <= 3 * 256 and min(sizes) == 0
    assert 100 << 20 < sum(sizes) * (SCAN_TOP + 1) // 37 and sum(sizes) * (2 * SCAN_TOP + 3) // 37 + max(sizes) * 37 < 2 ** 31
