"""The randomised differential run of the file layers (tests/fuzz_files.py) on the device: seeded cases of reader.BlockReader,
parse.parsefile, composition.tables_file, codons.codon_tables, minimizer.minimizers_file and probability.score_file, each file read at
a drawn or aimed block size and at block_bytes=None and compared with the whole-record answer of the CPU restatements; and the four
layers on the file whose last chunk is its last line end alone, where the reader used to emit a continuation piece that repeated the
overlap and brought no residue.  tests/test_fuzz_files_cpu.py shows, without a device, what the very cases of SEEDED cover.

TIMES, wall, measured on one MI355X (DESIGN.md section 20 has the table):
    the module alone, 16 tests                    32.7 s (14.1 s of it the first score test: the process's first use of the device and of torch)
    seeded, per (layer, seed) of 20 or 30 cases   1.0 - 2.4 s; inside the whole suite none of the 16 tests is among the 40 slowest (>= 3.4 s)
    the four end-of-file tests                    0.11, 0.01, 0.15, 0.23 s
    the whole -m gpu suite                        686 s before this module (1382 tests), 702 s with it (1398 tests)
The module's budget is a tenth of the suite's time before it, 68 s.  python tests/fuzz_files.py 60 777, once: 723 cases, all equal; 4 of
120 minimizer cases refused at their block size and equal at the refusal bound."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fuzz_files  # noqa: E402
import minimizer_cases as mc  # noqa: E402
import score_cases as sc  # noqa: E402
import tables_cases as tb  # noqa: E402

pytestmark = pytest.mark.gpu

SEEDED = fuzz_files.SEEDED


@pytest.mark.parametrize("layer,seed,ncases", SEEDED)
def test_seeded_fuzz_cases_equal_the_whole_record_answers(gpu_engine_cls, monkeypatch, tmp_path, capfd, layer, seed, ncases):
    from kmerdb_amd import reader
    default = reader.BLOCK_BYTES
    set_block = lambda b: monkeypatch.setattr(reader, "BLOCK_BYTES", default if b is None else int(b))      # (parsefile has no block_bytes argument)
    n, bad, refused, _ = fuzz_files.run_cases(seed, max_cases=ncases, layers=[layer], verbose=False, directory=str(tmp_path), set_block=set_block)
    capfd.readouterr()                                                        # (codon_tables warns of every record it leaves out)
    assert bad is None, f"case {n - 1} of seed {seed} differs from the whole-record answer of {layer}: {bad}"
    assert n == ncases and refused <= fuzz_files.MAX_REFUSED * ncases


# ---- the file whose last chunk is its last line end alone ----

BLOCK, K, W = 4096, 15, 10
RESIDUES = 2 * BLOCK - 3                      # ">r\n" + 8189 residues + "\n": two full chunks and one byte


def _one_record_file(folder, seed, p_n=0.0):
    rng = np.random.Generator(np.random.PCG64(seed))
    seq = mc.random_record(rng, RESIDUES, p_n)
    path = str(folder / ("end_%d.fa" % seed))
    with open(path, "wb") as f:
        f.write(b">r\n" + seq + b"\n")
    assert os.path.getsize(path) == 2 * BLOCK + 1
    return path, seq


def test_minimizers_file_when_the_last_chunk_is_the_last_line_end(gpu_engine_cls, tmp_path):
    """40 random records: a last piece of k + w - 2 residues, the overlap alone, has w - 1 start positions, and kdb_minimizers takes a
    record of fewer than w for one run -- its minimum is no minimizer of the record unless the run before agrees."""
    from kmerdb_amd import minimizer
    wrong = []
    for seed in range(40):
        path, seq = _one_record_file(tmp_path, seed)
        pos, ids, strand = mc.record_minimizers(seq, K, W, True, mc.LEX)
        for block_bytes in (BLOCK, None):
            (row,) = list(minimizer.minimizers_file(path, K, W, block_bytes=block_bytes))
            assert row[:2] == ("r", RESIDUES)
            if not (np.array_equal(row[2], pos) and np.array_equal(row[3], ids) and np.array_equal(row[4], strand)):
                wrong.append((seed, block_bytes, row[2][-3:].tolist(), pos[-3:].tolist()))
    assert not wrong, wrong


def test_tables_file_when_the_last_chunk_is_the_last_line_end(gpu_engine_cls, tmp_path):
    from kmerdb_amd import composition
    for seed, (k, stride) in enumerate([(4, 1), (3, 3), (6, 4), (1, 1)]):
        path, seq = _one_record_file(tmp_path, seed, p_n=0.001)
        row, windows, skipped, first, last = tb.record_table(seq, k, stride, True)
        for block_bytes in (BLOCK, None):
            (got,) = list(composition.tables_file(path, k, stride=stride, canonical=True, block_bytes=block_bytes))
            assert got[:6] == ("r", RESIDUES, windows, skipped, first, last) and np.array_equal(got[6], row.astype(np.uint64)), (k, stride, block_bytes)


def test_parsefile_when_the_last_chunk_is_the_last_line_end(gpu_engine_cls, oracle, monkeypatch, tmp_path):
    from kmerdb_amd import parse, reader
    for seed, (k, canonicalize, drop) in enumerate([(9, True, True), (5, False, False), (1, False, True)]):
        path, seq = _one_record_file(tmp_path, seed, p_n=0.001)
        want, total = oracle.c_count(*oracle.pack_records([seq]), k, canonicalize, oracle.N_DROP if drop else oracle.N_EXPAND)
        for block_bytes in (BLOCK, None):
            with monkeypatch.context() as m:
                if block_bytes:
                    m.setattr(reader, "BLOCK_BYTES", block_bytes)
                counts, md, _ = parse.parsefile(path, k, replace_with_none=drop, canonicalize=canonicalize)
            assert np.array_equal(counts, want), (k, block_bytes)
            assert (md["total_reads"], md["total_kmers"], md["min_read_length"], md["max_read_length"], md["avg_read_length"]) == (1, total, RESIDUES, RESIDUES, RESIDUES)


def test_score_file_when_the_last_chunk_is_the_last_line_end(gpu_engine_cls, tmp_path):
    from kmerdb_amd import probability
    for seed, (k, canonical) in enumerate([(6, False), (9, True), (1, False)]):
        path, seq = _one_record_file(tmp_path, seed, p_n=0.001)
        v, total = fuzz_files.profile(k, canonical)
        ref = sc.score_record(seq, v, k, canonical, total, 1)
        assert ref.windows > 0 and ref.log10_p not in (None, float("-inf"))
        for block_bytes in (BLOCK, None):
            (row,) = list(probability.score_file(path, fuzz_files.profile_file(k, canonical), pseudocount=1, block_bytes=block_bytes))
            assert row[:5] == ("r", RESIDUES, ref.windows, ref.zero_windows, ref.min_count), (k, block_bytes)
            assert sc.error(row[5], ref) <= sc.bound(ref, fuzz_files.fuzz_records.SCORE_PIECE, fuzz_files.fuzz_records.SCORE_LANES, joins=3 if block_bytes else 0)
