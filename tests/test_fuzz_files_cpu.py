"""CPU: the randomised run over the file layers (tests/fuzz_files.py) without a device.  The draws are deterministic and legal; the reader
row of the table holds for every seeded draw of every layer, at the overlap that layer reads with; tables_file, codon_tables,
minimizers_file and score_file run the very cases of tests/test_gpu_fuzz_files.py with the restatements in the device calls' places
(fuzz_files.stand_ins: score_cases.score_reads_stub expresses none_scored as score_record's plain form, so score_file's join is here
too; parsefile has no stand-in and is left to the device); the seeded cases reach what they are there for; no minimizer case is refused
at its refusal bound; and readers that are wrong in the three ways a reader of pieces can be wrong fail the reader row."""
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fuzz_files as ff  # noqa: E402

SEEDED = ff.SEEDED


def _overlap(desc):
    """the overlap the layer of a case reads the file with"""
    if desc["layer"] == "reader":
        return desc["overlap"]
    return desc["k"] + desc["w"] - 2 if desc["layer"] == "minimizers" else desc["k"] - 1


@pytest.fixture(scope="module")
def seeded(oracle, tmp_path_factory):
    """every seeded case, drawn once: [(desc, arrays, want, path of the file)]"""
    folder = tmp_path_factory.mktemp("fuzz_files")
    cases = []
    for layer, seed, n in SEEDED:
        for i in range(n):
            desc, arrays = ff.draw(seed, i, layer)
            sub = folder / ("%s_%d_%d" % (layer, seed, i))
            sub.mkdir()
            path = str(sub / ff.file_name(desc))
            with open(path, "wb") as f:
                f.write(arrays["data"])
            cases.append((desc, arrays, ff.want_case(desc, arrays, oracle), path))
    return cases


@pytest.fixture(scope="module")
def reader_rows(seeded):
    """the reader row of every seeded case -> [(failure or None, pieces per record)]"""
    return [ff.check_reader(path, dict(desc, overlap=_overlap(desc)), want) for desc, _, want, path in seeded]


def test_the_text_tools_on_a_text_written_by_hand():
    text = b"junk\n>a one\r\nAC\r\nG\r\n\r\n>b\nTT\n>c"
    assert ff.plain_parse(text) == [("a", b"ACG"), ("b", b"TT"), ("c", b"")]
    lay = ff.layout(text)
    assert [(s, h, at.tolist()) for s, h, at in lay] == [(5, 13, [13, 14, 17]), (22, 25, [25, 26]), (28, 30, [])]
    assert ff.aim_positions(text) == {"header_gt": [5, 22, 28], "in_header": [6, 7, 8, 9, 10, 11, 12, 23, 24, 29], "line_last_residue": [14, 17, 26],
                                      "line_cr": [15, 18], "line_lf": [16, 19, 27], "record_first_residue": [13, 25]}
    assert ff.edge_kinds(text, 5) == {"header_gt", "in_header", "line_cr", "record_first_residue", "size"} and ff.edge_kinds(text, 30) == {"size"} and ff.edge_kinds(text, 31) == {"size_plus_1"}
    assert ff.edge_kinds(text, 13) == {"record_first_residue", "line_last_residue"} and ff.edge_kinds(text, 29) == {"size_minus_1", "in_header"}
    assert ff.chunks_spanned(text, 8) == [3, 2, 1] and ff.chunks_spanned(text, 64) == [1, 1, 1]
    # the first m residues of a record end within H + g m bytes of its '>': H = 8 (">a one\r\n"), g = 3 (C -> G over "\r\n")
    assert ff.refusal_bound(text, 2, 2) == 8 + 3 * 3 and [ff.first_piece_need(text, m) for m in (1, 2, 3, 4)] == [9, 10, 13, 13]
    assert ff.plain_parse(b"@q d\nACGT\n+\n@+I#\n\n@r\nA\n+r\nI", fastq=True) == [("q", b"ACGT"), ("r", b"A")]
    stats = ff.text_stats(b">r\nNNNNNNNN\nNNNNAC\n\n\n\n", 4, False)
    assert stats["n_run_fills_a_chunk"] and stats["last_chunk_line_ends_only"] and not stats["empty_record"] and stats["most_chunks"] == 5
    stats = ff.text_stats(b">r\nNNNNNNNN\nANNNAC\n>e\n", 8, False)
    assert not stats["n_run_fills_a_chunk"] and not stats["last_chunk_line_ends_only"] and stats["empty_record"]


def test_draws_are_deterministic_and_legal(seeded):
    seen = set()
    for desc, arrays, _, _ in seeded:
        again, arrays2 = ff.draw(desc["seed"], desc["index"], desc["layer"])
        assert json.dumps(again) == json.dumps(desc) and arrays2["data"] == arrays["data"] and arrays2["text"] == arrays["text"]
        assert ff.legal(desc, arrays), desc
        seen.add(arrays["text"])
    assert len(seen) == len(seeded)
    assert {(d["layer"], d["seed"]) for d, _, _, _ in seeded} == {(layer, seed) for layer, seed, _ in SEEDED}


def test_every_draws_reader_row_holds(seeded, reader_rows):
    for (desc, _, _, _), (failed, _) in zip(seeded, reader_rows):
        assert failed is None, (failed, desc)


@pytest.mark.parametrize("layer,seed,ncases", [s for s in SEEDED if s[0] == "reader"])
def test_seeded_reader_cases(layer, seed, ncases, tmp_path):
    n, bad, _, _ = ff.run_cases(seed, max_cases=ncases, layers=[layer], verbose=False, directory=str(tmp_path))
    assert bad is None and n == ncases, bad


@pytest.mark.parametrize("layer,seed,ncases", [s for s in SEEDED if s[0] in ("tables", "codons", "minimizers", "score")])
def test_seeded_cases_through_the_stand_ins(layer, seed, ncases, tmp_path, capfd):
    with ff.stand_ins():
        n, bad, refused, nmin = ff.run_cases(seed, max_cases=ncases, layers=[layer], verbose=False, directory=str(tmp_path))
    assert bad is None and n == ncases, bad
    assert refused <= ff.MAX_REFUSED * ncases, (refused, ncases)
    capfd.readouterr()                                                        # (codon_tables warns of every record it leaves out)


def test_no_minimizer_case_is_refused_at_its_bound(seeded, tmp_path):
    """refusal_bound: from the text alone, and enough -- at it no seeded minimizer case is refused, and it does bound what it says it
    bounds in every seeded text."""
    from kmerdb_amd import minimizer
    ran = 0
    with ff.stand_ins():
        for desc, arrays, want, path in seeded:
            if desc["fastq"] or desc["layer"] not in ("parse", "score", "minimizers"):
                continue
            k, w = desc["k"], desc.get("w", 1)
            assert ff.refusal_bound(arrays["text"], k, w) >= ff.first_piece_need(arrays["text"], k + w - 1), desc
            if desc["layer"] != "minimizers" or "raises" in want:
                continue
            B = max(ff.refusal_bound(arrays["text"], k, w), 4 * (k + w))
            rows = list(minimizer.minimizers_file(path, k, w, canonical=desc["canonical"], order=ff.fuzz_records.ORDER_NAMES[desc["order"]], block_bytes=B))
            assert all(np.array_equal(got[2], pos) for got, (pos, _, _) in zip(rows, want["lists"])) and len(rows) == len(want["lists"]), desc
            ran += 1
    assert ran >= 40


def test_the_seeded_cases_reach_what_they_are_for(seeded, reader_rows):
    edges, per_layer = set(), {layer: dict(pieces=0, edges=set(), n_run=0, empty=0, line_ends=0, containers=set(), aimed=0) for layer in ff.LAYERS}
    for (desc, _, want, _), (_, pieces) in zip(seeded, reader_rows):
        stats, mine = want["stats"], per_layer[desc["layer"]]
        mine["pieces"] = max([mine["pieces"]] + pieces)
        mine["edges"] |= set(stats["edges"])
        mine["n_run"] += stats["n_run_fills_a_chunk"]
        mine["empty"] += stats["empty_record"]
        mine["line_ends"] += stats["last_chunk_line_ends_only"]
        mine["containers"].add(desc["container"])
        mine["aimed"] += desc["aim"] != "free"
        if desc["aim"] != "free":                                             # an aimed block size does put an edge where it aims
            assert desc["aim"] in stats["edges"], desc
    for layer, mine in per_layer.items():
        assert mine["pieces"] >= 3, layer                                     # a record in three pieces and more
        assert mine["containers"] == {"plain", "gzip", "bgzf"}, layer
        assert mine["line_ends"] >= 1, layer                                  # a last chunk of line ends only
        assert mine["aimed"] >= 10 and len(mine["edges"]) >= 8, (layer, mine["edges"])
        assert mine["empty"] >= 1 or layer in ("parse", "score"), layer       # (those two refuse a record below k)
        assert mine["n_run"] >= 1 or layer == "codons", layer                 # an N run longer than a block (codon_tables refuses three triplets with N)
        edges |= mine["edges"]
    assert edges == set(ff.AIMS)                                              # every aimed edge position


# ---- bite: readers that are wrong must fail the reader row ----

class _Bite:
    """reader.BlockReader with one fault; .bit counts how often the fault changed something"""

    def __init__(self, path, want_ids=False, block_bytes=None, overlap=None):
        from kmerdb_amd import reader
        self.rd, self.ov, self.bit = reader.BlockReader(path, want_ids=want_ids, block_bytes=block_bytes, overlap=overlap), int(overlap or 0), 0

    total_reads, min_len, max_len = (property(lambda self, name=name: getattr(self.rd, name)) for name in ("total_reads", "min_len", "max_len"))
    sum_len = property(lambda self: self.rd.sum_len)

    def pieces(self):
        """-> (block, the residues of its first record's record so far, before this block) per block"""
        so_far = b""
        for blk in self.rd:
            bases, offsets, _ = blk
            o = offsets.astype(np.int64)
            yield blk, so_far
            if len(o) > 1:
                last = bytes(bases[o[-2]:o[-1]])
                so_far = so_far + last[min(self.ov, len(so_far)):] if blk.cont and len(o) == 2 else last


class DropsTheOverlap(_Bite):
    def __iter__(self):
        from kmerdb_amd import reader
        for blk, so_far in self.pieces():
            p = min(self.ov, len(so_far)) if blk.cont else 0
            if p:
                self.bit += 1
                bases, offsets, ids = blk
                offsets = offsets.copy()
                offsets[1:] -= np.uint64(p)
                blk = reader.Block(bases[p:], offsets, ids, True)
            yield blk


class EmitsTheEmptyPiece(_Bite):
    def __iter__(self):
        from kmerdb_amd import reader
        for blk, so_far in self.pieces():
            yield blk
            bases, offsets, ids = blk
            if blk.cont and len(offsets) == 2:                                # the piece again, as the overlap alone
                self.bit += 1
                whole = so_far + bytes(bases)[min(self.ov, len(so_far)):]
                tail = np.frombuffer(whole[len(whole) - min(self.ov, len(whole)):], dtype=np.uint8)
                yield reader.Block(tail, np.array([0, tail.size], dtype=np.uint64), [None], True)


class MiscountsThePrefix(_Bite):
    """the statistics take every repeated prefix for one residue shorter than it is"""
    sum_len = property(lambda self: self.rd.sum_len + self.bit)

    def __iter__(self):
        for blk, so_far in self.pieces():
            self.bit += bool(blk.cont and min(self.ov, len(so_far)))
            yield blk


@pytest.mark.parametrize("bite", [DropsTheOverlap, EmitsTheEmptyPiece, MiscountsThePrefix])
def test_wrong_readers_fail_the_reader_row(seeded, reader_rows, bite):
    bitten = 0
    for (desc, _, want, path), (_, pieces) in zip(seeded, reader_rows):
        if max(pieces) == 1:                                                  # (no continuation piece: nothing for the fault to change)
            continue
        made = []

        def make(*args, **kwargs):
            made.append(bite(*args, **kwargs))
            return made[-1]
        failed, _ = ff.check_reader(path, dict(desc, overlap=_overlap(desc)), want, reader_cls=make, whole=False)
        assert (failed is not None) == bool(made[0].bit), (bite.__name__, failed, made[0].bit, desc)
        bitten += failed is not None
    assert bitten >= 40, bitten
