#!/usr/bin/env python3
"""Randomised differential test of the FILE LAYERS: the code that turns reader.BlockReader's blocks and continuation pieces into
per-record answers -- the reader itself, parse.parsefile, composition.tables_file, codons.codon_tables, minimizer.minimizers_file and
probability.score_file.  A sibling of tests/fuzz_records.py, which fuzzes the calls those layers sit on.
Usage: python tests/fuzz_files.py [seconds] [seed] [layer,layer,...]    prints one line per case and a summary; exit 1 on a mismatch.
Also collected by pytest -m gpu through tests/test_gpu_fuzz_files.py; tests/test_fuzz_files_cpu.py runs the very same cases without a
device, with the CPU restatements of the device calls in their place, and shows what the seeded cases cover.

A case is (seed, index, layer): its generator is seeded with exactly those three (draw(seed, index, layer)).  draw_case gives the
description (JSON) and the file's bytes; want_case the answer on the CPU -- the text parsed by plain_parse, a parser written here from
the formats' definition and from no project code, then the restatements under tests/ applied to WHOLE records --; check_case writes the
file, runs the layer at the case's block_bytes and at block_bytes=None, and compares both with that answer.

The file.  Records from fuzz_records.draw_records (lengths around one and two reader blocks, empty and short ones, N in runs and at three
densities), written as FASTA (wrap 0, 1, 7, 60, 80 or a free length per line; LF or CRLF; blank lines inside and behind records, also a
run of them as long as a block; headers with and without a description of up to 200 bytes; text before the first header; a file that
ends with one line end, with none or with several) or as four-line FASTQ (which the reader never cuts into pieces: it is here for the
containers and the carry between blocks), plain, as one gzip stream or as BGZF members.  At most 64 KiB of text, and at most CHUNKS
reader blocks of it.

block_bytes.  Free values from the layer's smallest one upward, and values AIMED at the text, so that a chunk edge falls in front of a
header's '>', inside a header, in front of a line's last residue, its CR, its LF, a record's first residue, the file's last one or two
bytes, at the file's size and one past it (AIMS; edge_kinds says, from the text alone, what the edges of a block size hit).
The smallest block size: 1 for the reader, tables_file and codon_tables; 4 (k + w), what minimizers_file itself asks, for the
minimizers; refusal_bound(text, k, 1) for parsefile and score_file, because the engine and kdb_score_reads refuse a record's FIRST
piece if it is shorter than k, as they refuse a record: below that bound a long record whose header ends a chunk is a ValueError,
loudly, and the fuzz does not go there.

The refusal bound.  minimizers_file refuses a file (ValueError "... block_bytes is too small for this file") when a piece that is
followed by another holds fewer than k + w - 1 residues.  A continuation piece repeats k + w - 2 and brings at least one, so only a
record's first piece can be that short.  A first piece spans at least block_bytes bytes from the record's '>' (the reader holds a record
that begins in a chunk back to the next chunk, or the chunk begins with it), or the whole record.  With H the longest header line, line
end included, and g the largest distance in bytes from one residue of a record to the next (from the header's end to one past the first
residue, too: blank lines count), the first m residues of every record end within H + g m bytes of its '>':
    refusal_bound(text, k, w) = H + g (k + w - 1)
and at a block size of at least that no file is refused.  A refused case must pass there (check_case runs it again at
max(bound, 4 (k + w))); tests/test_fuzz_files_cpu.py runs every seeded minimizer case at its bound and sees none refused.

Lower case and IUPAC letters, per layer.  reader: both, at any density -- it passes residues through and keeps their case (the module
docstring of kmerdb_amd/reader.py).  tables_file, codon_tables, minimizers_file: include/kdbhip.h says of kdb_record_tables and
kdb_minimizers that a byte outside upper-case ACGTN anywhere in a batch refuses the call, so one case in 25 holds such a letter and the
layer must raise ValueError at every block size.  parsefile, score_file: left out.  DESIGN.md section 1 makes the outcome depend, window
by window, on whether an N shields the letter, tests/golden/iupac_next_to_n.json holds those cases, and neither the oracle's c_count nor
score_cases.score_record restates them.
"""
import gzip
import io
import json
import os
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (ROOT, HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import numpy as np  # noqa: E402

import fuzz_records  # noqa: E402
import minimizer_cases as mc  # noqa: E402
import score_cases as sc  # noqa: E402
import tables_cases as tb  # noqa: E402

LAYERS = ("reader", "parse", "tables", "codons", "minimizers", "score")
AIMS = ("header_gt", "in_header", "line_last_residue", "line_cr", "line_lf", "record_first_residue", "size_minus_2", "size_minus_1", "size",
        "size_plus_1")
MAX_TEXT = 64 << 10                            # bytes of (uncompressed) text in a file
TEXT_CAP = {"score": 8 << 10, "parse": 32 << 10}      # (score_cases.score_record and the oracle's N expansion walk every window in turn)
CHUNKS = 1000                                  # reader blocks in a file, at most: a block is a device call
MAX_OVERLAP = 70
PARSE_MAX_K, EXPAND_MAX_K, TABLES_MAX_K, MIN_MAX_K, MIN_MAX_W, SCORE_MAX_K = 9, 5, 6, 31, 64, 9     # (N expansion: 4^m k-mers for a window of m Ns)
REFUSED = "block_bytes is too small for this file"
MAX_REFUSED = 0.10                             # the share of a run's minimizer cases that may be refused at their block size
# (layer, seed, cases) of the seeded runs: tests/test_gpu_fuzz_files.py runs them on the device, tests/test_fuzz_files_cpu.py with the stand-ins
SEEDED = [(layer, seed, 30 if layer == "minimizers" else 20) for layer in LAYERS for seed in (101, 202)]
IUPAC = b"RYSWKMBDHV"
EOL = (10, 13)


def case_rng(seed, index, layer):
    return np.random.Generator(np.random.PCG64([int(seed), int(index), 1000 + LAYERS.index(layer)]))


# ---------------------------------------------------------------------------------------------------------------
# the text: written, parsed plainly, and measured
# ---------------------------------------------------------------------------------------------------------------

def plain_parse(text, fastq=False):
    """The records of a FASTA / FASTQ text -> [(id: str, residues: bytes)].  FASTA: a line that begins with '>' opens a record, its id
    is the first whitespace-separated word behind the '>'; every other line, its line end and blanks taken off, is appended to the open
    record; lines before the first header are dropped.  FASTQ in four lines: title, residues, '+', qualities; blank lines between
    records are dropped."""
    lines = [line.rstrip(b"\r") for line in bytes(text).split(b"\n")]
    name = lambda line: (line[1:].split() or [b""])[0].decode("utf-8", "replace")
    recs = []
    if fastq:
        at = 0
        while at < len(lines):
            if not lines[at]:
                at += 1
                continue
            assert lines[at][:1] == b"@" and lines[at + 2][:1] == b"+" and len(lines[at + 3]) == len(lines[at + 1])
            recs.append((name(lines[at]), lines[at + 1]))
            at += 4
        return recs
    for line in lines:
        if line[:1] == b">":
            recs.append((name(line), b""))
        elif recs:
            recs[-1] = (recs[-1][0], recs[-1][1] + line.replace(b" ", b"").replace(b"\t", b""))
    return recs


def layout(text):
    """Where a FASTA text keeps its records -> [(s, h, at)] per record: s the byte of the '>', h the byte behind the header line (its
    line end included), at: int64[] the bytes of the record's residues.  A walk over the lines, like plain_parse."""
    t = np.frombuffer(bytes(text), dtype=np.uint8)
    out, pos = [], 0
    for line in bytes(text).split(b"\n"):
        end = pos + len(line) + 1                                             # (one past the text for a last line without LF)
        if line[:1] == b">":
            out.append([pos, min(end, t.size), []])
        elif out and line.strip():
            body = np.arange(pos, pos + len(line))
            out[-1][2].append(body[~np.isin(t[pos:pos + len(line)], (13, 32, 9))])
        pos = end
    return [(s, h, np.concatenate(at) if at else np.zeros(0, dtype=np.int64)) for s, h, at in out]


def refusal_bound(text, k, w):
    """H + g (k + w - 1) of the module docstring, from the text alone"""
    H, g = 1, 1
    for s, h, at in layout(text):
        H = max(H, h - s)
        if at.size:
            g = max(g, int(at[0]) - h + 1, int(np.diff(at).max()) if at.size > 1 else 1)
    return H + g * (k + w - 1)


def first_piece_need(text, m):
    """the bytes from a record's '>' through its m-th residue (its last, if it has fewer; its header line, if none), largest over the
    records: what refusal_bound bounds"""
    need = 1
    for s, h, at in layout(text):
        need = max(need, (int(at[min(m, at.size) - 1]) + 1 if at.size else h) - s)
    return need


def aim_positions(text):
    """-> {aim: sorted bytes p}: a chunk edge in front of byte p is an edge of that kind (FASTA)"""
    t = np.frombuffer(bytes(text), dtype=np.uint8)
    pos = {a: [] for a in AIMS[:6]}
    for s, h, at in layout(text):
        pos["header_gt"].append(s)
        pos["in_header"] += list(range(s + 1, h))                             # (behind the '>', the header's line end included: without it the header waits)
        if at.size:
            pos["record_first_residue"].append(int(at[0]))
            last = at[np.append(np.diff(at) > 1, True)]                       # a residue that is not followed by one at once
            pos["line_last_residue"] += last.tolist()
            for p in (last + 1).tolist():
                if p < t.size and t[p] == 13:
                    pos["line_cr"].append(p)
                    p += 1
                if p < t.size and t[p] == 10:
                    pos["line_lf"].append(p)
    return {a: sorted(set(p)) for a, p in pos.items()}


def edge_kinds(text, block_bytes):
    """the kinds of AIMS that the chunk edges of block_bytes hit in this text, counted from the text and the block size alone"""
    size, B = len(text), int(block_bytes)
    hit = {a for a, d in (("size_minus_2", -2), ("size_minus_1", -1), ("size", 0), ("size_plus_1", 1)) if size + d >= B and (size + d) % B == 0}
    edges = np.arange(B, size, B, dtype=np.int64)
    if edges.size:
        for a, p in aim_positions(text).items():
            if np.isin(edges, np.array(p, dtype=np.int64)).any():
                hit.add(a)
    return hit


def chunks_spanned(text, block_bytes):
    """per FASTA record: the number of chunks its bytes, from the '>' through its last residue, lie in"""
    B = int(block_bytes)
    return [int((int(at[-1]) if at.size else h - 1) // B - s // B + 1) for s, h, at in layout(text)]


def text_stats(text, block_bytes, fastq):
    """what a case reaches, from the text and the block size (tests/test_fuzz_files_cpu.py adds what the reader's pieces show)"""
    t = np.frombuffer(bytes(text), dtype=np.uint8)
    B, size = int(block_bytes), len(text)
    stats = dict(edges=sorted(edge_kinds(text, B)) if not fastq else [], n_run_fills_a_chunk=False, empty_record=False, last_chunk_line_ends_only=False,
                 most_chunks=1)
    if fastq:
        return stats
    lay = layout(text)
    stats["empty_record"] = any(at.size == 0 for _, _, at in lay)
    stats["most_chunks"] = max(chunks_spanned(text, B), default=1)
    last = t[(size - 1) // B * B:] if size else t
    stats["last_chunk_line_ends_only"] = bool(size > B and lay and lay[-1][2].size and np.isin(last, EOL).all())
    for s, h, at in lay:
        if at.size:
            for j in range(-(-h // B), (int(at[-1]) + 1) // B):               # the chunks that lie whole between the header and the last residue
                inside = at[(at >= j * B) & (at < (j + 1) * B)]
                if inside.size and (t[inside] == fuzz_records.N).all():
                    stats["n_run_fills_a_chunk"] = True
    return stats


def _wrapped(rng, seq, wrap):
    if wrap == 0:
        return [seq] if seq else []
    lines, at = [], 0
    while at < len(seq):
        n = int(rng.integers(1, 101)) if wrap == "free" else wrap
        lines.append(seq[at:at + n])
        at += n
    return lines


def _description(rng):
    n = int(rng.choice([1, int(rng.integers(1, 30)), int(rng.integers(30, 201))]))
    return bytes(rng.choice(np.frombuffer(b"abcdefgXYZ 0123456789_|=:>@+;,.-\t", dtype=np.uint8), size=n).tolist()).replace(b"\t\t", b"\t ")


def render(rng, ids, records, shape):
    """the text of the records in the shape drawn for the file"""
    eol = b"\r\n" if shape["crlf"] else b"\n"
    out = []
    if shape["fastq"]:
        for rid, seq in zip(ids, records):
            desc = b" " + _description(rng) if rng.random() < shape["p_desc"] else b""
            qual = bytes(rng.choice(np.frombuffer(b"@+I#5", dtype=np.uint8), size=len(seq)).tolist())
            out.append(b"@" + rid + desc + eol + seq + eol + b"+" + (rid + desc if rng.random() < 0.2 else b"") + eol + qual + eol)   # (the title again, or nothing)
            if rng.random() < shape["p_blank"]:
                out.append(eol * int(rng.integers(1, 4)))
    else:
        if shape["junk"]:
            out.append(b"".join(b"text before the first header %d" % i + eol for i in range(shape["junk"])))
        for r, (rid, seq) in enumerate(zip(ids, records)):
            desc = b" " + _description(rng) if rng.random() < shape["p_desc"] else b""
            out.append(b">" + rid + desc + eol)
            lines = _wrapped(rng, seq, shape["wrap"])
            gap_at = int(rng.integers(0, len(lines))) if lines and r == shape["gap_record"] else -1
            if shape["p_blank"] and rng.random() < shape["p_blank"]:           # (blank lines between the header and the first residue)
                out.append(eol * int(rng.integers(1, 4)))
            for i, line in enumerate(lines):
                out.append(line + eol)
                if i == gap_at:
                    out.append(eol * shape["gap_lines"])                      # a run of blank lines as long as a block, in mid-record
                elif shape["p_blank"] and rng.random() < shape["p_blank"]:
                    out.append(eol * int(rng.integers(1, 4)))
    text = b"".join(out)
    if shape["ending"] == "none":
        text = text.rstrip(b"\r\n")
    elif shape["ending"] == "several":
        text = text.rstrip(b"\r\n") + eol * shape["ending_lines"]
    return text


def contain(rng, text, container):
    """the file's bytes: the text as it is, as one gzip stream, or as BGZF members and the empty member that ends them"""
    if container == "plain":
        return text
    if container == "gzip":
        buf = io.BytesIO()
        with gzip.GzipFile(fileobj=buf, mode="wb", mtime=0) as f:
            f.write(text)
        return buf.getvalue()
    from kmerdb_amd import fileutil
    member = int(rng.choice([int(rng.integers(1, 200)), int(rng.integers(200, 65281)), 65280]))
    member = max(member, len(text) // 400 + 1)
    return b"".join(fileutil._bgzf_member(text[i:i + member]) for i in range(0, len(text), member)) + fileutil._bgzf_member(b"")


def file_name(desc):
    return "case" + (".fq" if desc["fastq"] else ".fa") + ("" if desc["container"] == "plain" else ".gz")


# ---------------------------------------------------------------------------------------------------------------
# the draw
# ---------------------------------------------------------------------------------------------------------------

def _draw_params(rng, layer):
    if layer == "reader":
        return dict(overlap=int(rng.choice([0, 1, int(rng.integers(0, MAX_OVERLAP + 1))])))
    if layer == "parse":
        drop = bool(rng.integers(0, 2))
        return dict(k=int(rng.integers(1, (PARSE_MAX_K if drop else EXPAND_MAX_K) + 1)), canonicalize=bool(rng.integers(0, 2)), replace_with_none=drop)
    if layer == "tables":
        k = int(rng.integers(1, TABLES_MAX_K + 1))
        return dict(k=k, stride=int(rng.integers(1, k + 1)), canonical=bool(rng.integers(0, 2)))
    if layer == "codons":
        return dict(k=3, stride=3, as_reference=bool(rng.integers(0, 2)), include_start_codons=bool(rng.integers(0, 2)), include_stop_codons=bool(rng.integers(0, 2)))
    if layer == "minimizers":
        k = int(rng.integers(1, MIN_MAX_K + 1))
        w = int(rng.choice([1, int(rng.integers(2, 17)), int(rng.integers(17, MIN_MAX_W + 1))]))
        return dict(k=k, w=w, canonical=bool(rng.integers(0, 2)), order=int(rng.integers(0, 2)))
    return dict(k=int(rng.integers(1, SCORE_MAX_K + 1)), canonical=bool(rng.integers(0, 2)), pseudocount=int(rng.choice([0, 1, 1, 7])))


def _window_k(layer, params):
    return params["overlap"] + 1 if layer == "reader" else params["k"]


def smallest_block(layer, params, text):
    """the smallest block_bytes the fuzz gives the layer (module docstring)"""
    if layer == "minimizers":
        return 4 * (params["k"] + params["w"])
    if layer in ("parse", "score"):
        return refusal_bound(text, params["k"], 1)
    return 1


def draw_case(rng, layer):
    """One random case of `layer` -> (description dict, JSON-serialisable; dict(text: the file's text, data: the file's bytes))."""
    params = _draw_params(rng, layer)
    k = _window_k(layer, params)
    fastq = layer != "codons" and rng.random() < 0.15
    floor = 4 * (params["k"] + params["w"]) if layer == "minimizers" else 1
    x = rng.random()
    nominal = floor + int(rng.integers(0, 24)) if x < 0.3 else int(np.exp(rng.uniform(np.log(floor), np.log(max(4096, 2 * floor)))))
    cap = min(TEXT_CAP.get(layer, MAX_TEXT), CHUNKS * nominal)
    if layer in ("parse", "score"):                                           # (their smallest block is a header and k residues: the text takes its measure from there)
        nominal = max(nominal, int(rng.choice([20, 100, 300])))
    # the records: lengths around one and two blocks' residues, as fuzz_records draws them around a call's piece
    shortest = k if layer in ("parse", "score") else 1 if fastq else 0
    top = max(k + 1, min(3000, cap))
    nrec = int(rng.integers(1, 13))
    length_for = (lambda n: 3 * (n // 3)) if layer == "codons" and rng.random() < 0.8 else (lambda n: n)
    records = fuzz_records.draw_records(rng, nrec, k, max(1, min(nominal, top)), length_for, top, shortest=shortest, long=rng.random() < 0.5)
    records = [r if len(r) >= shortest else fuzz_records.draw_content(rng, shortest, records) for r in records]      # (the long one, at a tiny block)
    if layer != "codons" and rng.random() < 0.2 and any(len(r) > 1 for r in records):       # an N run of a block's length and more
        i = int(rng.choice([i for i, r in enumerate(records) if len(r) > 1]))
        at = int(rng.integers(0, len(records[i]) - 1))
        g = max(1, int(nominal * rng.uniform(1.0, 2.5)))
        records[i] = records[i][:at] + b"N" * len(records[i][at:at + g]) + records[i][at + g:]
    if layer == "codons":                                                     # (more than two triplets with an N refuse the whole file: few records keep theirs)
        records = [r if rng.random() < 0.15 else r.replace(b"N", b"A") for r in records]
    letters = None
    if layer == "reader" and rng.random() < 0.4:                              # lower case and IUPAC letters pass through the reader
        p = float(rng.choice([0.01, 0.5]))
        alphabet = np.frombuffer(b"acgtn" + IUPAC + IUPAC.lower(), dtype=np.uint8)
        for i, r in enumerate(records):
            s = np.frombuffer(r, dtype=np.uint8).copy()
            change = rng.random(s.size) < p
            s[change] = alphabet[rng.integers(0, alphabet.size, size=int(change.sum()))]
            records[i] = s.tobytes()
        letters = "any"
    elif layer in ("tables", "codons", "minimizers") and rng.random() < 0.04 and any(len(r) for r in records):
        i = int(rng.choice([i for i, r in enumerate(records) if len(r)]))
        at = int(rng.integers(0, len(records[i])))
        records[i] = records[i][:at] + bytes([int(rng.choice(np.frombuffer(b"acgtn" + IUPAC, dtype=np.uint8)))]) + records[i][at + 1:]
        letters = "refused"
    ids = [b"r%d" % i if rng.random() < 0.8 else b"rec%d|" % i + b"x" * int(rng.integers(1, 60)) for i in range(nrec)]
    shape = dict(fastq=bool(fastq), crlf=bool(rng.random() < 0.3), wrap=[0, 1, 7, 60, 80, "free"][int(rng.integers(0, 6))],
                 p_blank=float(rng.choice([0.0, 0.0, 0.05, 0.3])), p_desc=float(rng.choice([0.0, 0.5, 1.0])),
                 junk=int(rng.integers(1, 4)) if rng.random() < 0.2 else 0, gap_record=int(rng.integers(0, nrec)) if rng.random() < 0.2 else -1,
                 gap_lines=max(1, min(3000, int(nominal * rng.uniform(0.5, 2.5)))), ending=str(rng.choice(["one", "one", "none", "several"])),
                 ending_lines=int(rng.choice([2, 3, max(2, min(3000, nominal + 2))])))
    if shape["wrap"] == 1 and sum(len(r) for r in records) > 6000:            # (a line per residue: keep the walk over the lines short)
        shape["wrap"] = 7
    render_seed = int(rng.integers(0, 2 ** 62))
    while True:
        text = render(np.random.Generator(np.random.PCG64(render_seed)), ids, records, shape)
        if len(text) <= cap:
            break
        if len(records) > 1:
            records.pop()
            ids.pop()
            shape["gap_record"] = min(shape["gap_record"], len(records) - 1)
        else:
            shape["gap_lines"], shape["ending_lines"] = min(shape["gap_lines"], cap // 8), min(shape["ending_lines"], cap // 8)
            keep = max(shortest, min(len(records[0]) // 2, cap // 4))
            records[0] = records[0][:keep - keep % 3] if layer == "codons" and keep >= 3 else records[0][:keep]
            shape["p_desc"] = 0.0 if keep <= shortest else shape["p_desc"]
            if keep <= shortest:
                cap = max(cap, len(render(np.random.Generator(np.random.PCG64(render_seed)), ids, records, shape)))
    # block_bytes: aimed at the text, or free
    low = max(smallest_block(layer, params, text) if not fastq else floor, -(-len(text) // CHUNKS), 1)
    block_bytes, aim = max(nominal, low), "free"
    if not fastq and rng.random() < 0.55:
        aim = AIMS[int(rng.integers(0, len(AIMS)))]
        if aim in AIMS[:6]:
            p = [x for x in aim_positions(text)[aim] if x >= low]
            target = int(p[int(rng.integers(0, len(p)))]) if p else 0
        else:
            target = len(text) + {"size_minus_2": -2, "size_minus_1": -1, "size": 0, "size_plus_1": 1}[aim]
        part = [j for j in (1, 2, 3, 4, 5, 7) if target % j == 0 and target // j >= low]      # the edge may be the first one, or a later one
        if target >= low and part:
            block_bytes = target // int(rng.choice(part))
        else:
            aim = "free"
    container = str(rng.choice(["plain", "plain", "plain", "gzip", "bgzf"]))
    desc = dict(layer=layer, **params, fastq=bool(fastq), container=container, block_bytes=int(block_bytes), aim=aim, letters=letters, size=len(text),
                lens=[len(r) for r in records], shape=shape, smallest_block=int(low))
    return desc, dict(text=text, data=contain(rng, text, container))


def draw(seed, index, layer):
    """the case (seed, index, layer), from nothing else"""
    desc, arrays = draw_case(case_rng(seed, index, layer), layer)
    return dict(seed=int(seed), index=int(index), **desc), arrays


def legal(desc, arrays):
    """the draw keeps to what the module docstring promises and to what the layer's own argument checks ask -> bool"""
    from kmerdb_amd import composition, minimizer
    text, layer, B = arrays["text"], desc["layer"], desc["block_bytes"]
    recs = plain_parse(text, desc["fastq"])
    ok = len(text) <= MAX_TEXT and [len(s) for _, s in recs] == desc["lens"] and len(recs) >= 1 and -(-len(text) // B) <= CHUNKS and B >= 1
    if layer == "reader":
        ok &= 0 <= desc["overlap"] <= MAX_OVERLAP
    elif layer == "parse":
        ok &= 1 <= desc["k"] <= PARSE_MAX_K and all(len(s) >= desc["k"] for _, s in recs) and (desc["replace_with_none"] or desc["k"] <= EXPAND_MAX_K)
    elif layer in ("tables", "codons"):
        ok &= 1 <= desc["k"] <= min(TABLES_MAX_K, composition.MAX_K) and 1 <= desc["stride"] <= desc["k"] and (layer == "tables" or not desc["fastq"])
    elif layer == "minimizers":
        ok &= 1 <= desc["k"] <= min(MIN_MAX_K, minimizer.MAX_K) and 1 <= desc["w"] <= min(MIN_MAX_W, minimizer.MAX_W) and B >= 4 * (desc["k"] + desc["w"])
    else:
        ok &= 1 <= desc["k"] <= SCORE_MAX_K and all(len(s) >= desc["k"] for _, s in recs)
    if layer in ("parse", "score") and not desc["fastq"]:
        ok &= B >= refusal_bound(text, desc["k"], 1) >= first_piece_need(text, desc["k"])
    alphabet = set(b"ACGTN")
    if desc["letters"] is None:
        ok &= all(set(s) <= alphabet for _, s in recs)
    elif desc["letters"] == "refused":
        ok &= sum(len(set(s) - alphabet) for _, s in recs) == 1
    return bool(ok)


# ---------------------------------------------------------------------------------------------------------------
# the answers, from whole records
# ---------------------------------------------------------------------------------------------------------------

_PROFILES = {}
_PROFILE_DIR = []


def _profile_dir():
    """a folder of this process's own for the .kdb profiles, removed when it ends"""
    if not _PROFILE_DIR:
        import atexit
        import shutil
        _PROFILE_DIR.append(tempfile.mkdtemp(prefix="fuzz_files_"))
        atexit.register(shutil.rmtree, _PROFILE_DIR[0], True)
    return _PROFILE_DIR[0]


def profile(k, canonical):
    """the count vector the score cases of this k and strand mode are scored against: score_cases.spread_vector -- zeros, small counts, a
    few near 2^40 --, folded onto the smaller of both strands' ids where canonical -> (v: uint64[4^k], total)"""
    if (k, canonical) not in _PROFILES:
        v = sc.spread_vector(k, 900 + k)
        if canonical:
            ids = np.arange(4 ** k, dtype=np.int64)
            folded = np.zeros_like(v)
            np.add.at(folded, np.minimum(ids, tb.rc_ids(ids, k)), v)
            v = folded
        _PROFILES[(k, canonical)] = (v, int(v.sum(dtype=np.uint64)))
    return _PROFILES[(k, canonical)]


def profile_file(k, canonical):
    """the .kdb of profile(k, canonical), written once"""
    from kmerdb_amd import fileutil
    path = os.path.join(_profile_dir(), "fuzz_%s.%d.kdb" % ("canonical" if canonical else "forward", k))
    if not os.path.exists(path):
        v, total = profile(k, canonical)
        md = {"version": fileutil.VERSION, "metadata_blocks": 1, "k": k, "total_kmers": total, "unique_kmers": int(np.count_nonzero(v)), "unique_nullomers": 0,
              "sorted": False, "tags": [], "files": []}
        fileutil.write_kdb(path, md, v)
    return path


def want_case(desc, arrays, oracle=None):
    """the part of a case that runs on the CPU: the plain parse of the text, and the layer's answer for the WHOLE records (a dict).
    oracle: oracle.kmer_oracle, for the parse layer."""
    layer = desc["layer"]
    recs = plain_parse(arrays["text"], desc["fastq"])
    lens = [len(s) for _, s in recs]
    want = dict(records=recs, stats=dict(text_stats(arrays["text"], desc["block_bytes"], desc["fastq"]), container=desc["container"]),
                statistics=(len(lens), min(lens), max(lens), sum(lens)))
    if desc["letters"] == "refused":
        want["raises"] = ValueError
        return want
    if layer == "parse":
        counts, total = oracle.c_count(*oracle.pack_records([s for _, s in recs]), desc["k"], desc["canonicalize"],
                                       oracle.N_DROP if desc["replace_with_none"] else oracle.N_EXPAND)
        unique = int(np.count_nonzero(counts))
        want["counts"] = counts
        want["metadata"] = dict(total_reads=len(lens), total_kmers=int(total), unique_kmers=unique, nullomers=4 ** desc["k"] - unique, min_read_length=min(lens),
                                max_read_length=max(lens), avg_read_length=int(sum(lens) / len(lens)))
    elif layer == "tables":
        want["rows"] = [tb.record_table(s, desc["k"], desc["stride"], desc["canonical"]) for _, s in recs]
    elif layer == "codons":
        from kmerdb_amd import codons
        ids, rows, flags = [], [], []
        for rid, s in recs:                                                   # codon_tables' host rules on whole-record tables: the join is what is tested
            row, windows, skipped, first, last = tb.record_table(s, 3, 3, desc["as_reference"])
            if len(s) % 3:
                continue
            if skipped > 2:
                want["raises"] = ValueError
                break
            ids.append(rid)
            rows.append(codons.counts_from_row(row, windows, first, last, desc["include_start_codons"], desc["include_stop_codons"]))
            flags.append(codons.is_non_canonical(windows, skipped, first, last))
        want["codons"] = (ids, rows, flags)
    elif layer == "minimizers":
        want["lists"] = [mc.record_minimizers(s, desc["k"], desc["w"], desc["canonical"], desc["order"]) for _, s in recs]
    elif layer == "score":
        v, total = profile(desc["k"], desc["canonical"])
        want["scores"] = [sc.score_record(s, v, desc["k"], desc["canonical"], total, desc["pseudocount"]) for _, s in recs]
        # the chunks a record's bytes can span, from the text: every chunk edge inside it may cut a piece, and a piece is a join
        want["joins"] = [1] * len(recs) if desc["fastq"] else chunks_spanned(arrays["text"], desc["block_bytes"])
    return want


# ---------------------------------------------------------------------------------------------------------------
# the layers, run and compared
# ---------------------------------------------------------------------------------------------------------------

def read_pieces(rd, overlap):
    """Join the blocks of a streamed file -> (failure or None, [(id, residues)], pieces per record).  Every continuation piece must begin
    with the last min(overlap, so far) residues of its record and bring at least one more."""
    recs, pieces = [], []
    for blk in rd:
        bases, offsets, ids = blk
        o = np.asarray(offsets).astype(np.int64)
        cont = bool(getattr(blk, "cont", False))
        if o.size < 2 or o[0] != 0 or np.any(np.diff(o) < 0) or o[-1] != len(bases):
            return "a block's offsets", recs, pieces
        for r in range(o.size - 1):
            seq = bytes(bases[o[r]:o[r + 1]])
            if r == 0 and cont:
                if not recs:
                    return "a continuation piece before any record", recs, pieces
                if ids is not None and ids[0] is not None:
                    return "a continuation piece with an id", recs, pieces
                p = min(int(overlap), len(recs[-1][1]))
                if seq[:p] != recs[-1][1][len(recs[-1][1]) - p:]:
                    return "a piece's prefix is not the record's last %d residues" % p, recs, pieces
                if len(seq) <= p:
                    return "a continuation piece without a new residue", recs, pieces
                recs[-1] = (recs[-1][0], recs[-1][1] + seq[p:])
                pieces[-1] += 1
            else:
                recs.append((ids[r], seq))
                pieces.append(1)
    return None, recs, pieces


def check_reader(path, desc, want, reader_cls=None, whole=True):
    """the reader row of the table -> (failure or None, pieces per record at the case's block size).  whole=False: at the case's block
    size only, not at block_bytes=None and not read whole."""
    from kmerdb_amd import reader
    reader_cls = reader_cls or reader.BlockReader
    shown = None
    for B in (desc["block_bytes"], None) if whole else (desc["block_bytes"],):
        rd = reader_cls(path, want_ids=True, block_bytes=B, overlap=desc["overlap"])
        failed, recs, pieces = read_pieces(rd, desc["overlap"])
        shown = pieces if shown is None else shown
        where = " at block_bytes=%s" % B
        if failed:
            return failed + where, shown
        if recs != want["records"]:
            return "records" + where, shown
        if (rd.total_reads, rd.min_len, rd.max_len, rd.sum_len) != want["statistics"]:
            return "statistics" + where, shown
    if not whole:
        return None, shown
    rd = reader.BlockReader(path, want_ids=True)                               # (one block per FASTA file: no overlap given)
    failed, recs, _ = read_pieces(rd, 0)
    if failed or recs != want["records"] or (rd.total_reads, rd.min_len, rd.max_len, rd.sum_len) != want["statistics"]:
        return "the file read whole", shown
    return None, shown


def _raises(run, error):
    try:
        run()
    except error:
        return True
    return False


def _check_parse(path, desc, want, set_block):
    from kmerdb_amd import parse
    for B in (desc["block_bytes"], None):
        set_block(B)
        counts, md, nullomers = parse.parsefile(path, desc["k"], replace_with_none=desc["replace_with_none"], canonicalize=desc["canonicalize"])
        where = " at block_bytes=%s" % B
        if counts.dtype != np.uint64 or not np.array_equal(counts, want["counts"]):
            return "counts" + where
        if {x: md[x] for x in want["metadata"]} != want["metadata"]:
            return "metadata" + where
        if not np.array_equal(np.sort(np.asarray(nullomers, dtype=np.int64)), np.flatnonzero(want["counts"] == 0)):
            return "nullomers" + where
    return None


def _check_tables(path, desc, want, set_block):
    from kmerdb_amd import composition
    for B in (desc["block_bytes"], None):
        run = lambda: list(composition.tables_file(path, desc["k"], stride=desc["stride"], canonical=desc["canonical"], block_bytes=B))
        where = " at block_bytes=%s" % B
        if "raises" in want:
            if not _raises(run, want["raises"]):
                return "no refusal" + where
            continue
        rows = run()
        if [(r[0], r[1]) for r in rows] != [(rid, len(s)) for rid, s in want["records"]]:
            return "ids and lengths" + where
        for got, (row, windows, skipped, first, last) in zip(rows, want["rows"]):
            if got[2:6] != (windows, skipped, first, last) or got[6].dtype != np.uint64 or not np.array_equal(got[6], row.astype(np.uint64)):
                return "record %r%s" % (got[0], where)
    return None


def _check_codons(path, desc, want, set_block):
    from kmerdb_amd import codons
    for B in (desc["block_bytes"], None):
        run = lambda: codons.codon_tables(path, include_start_codons=desc["include_start_codons"], include_stop_codons=desc["include_stop_codons"],
                                          include_noncanonicals=True, ignore_invalid_cds=True, as_reference=desc["as_reference"], block_bytes=B)
        where = " at block_bytes=%s" % B
        if "raises" in want:
            if not _raises(run, want["raises"]):
                return "no refusal" + where
            continue
        ids, rows, flags = run()
        wids, wrows, wflags = want["codons"]
        if list(ids) != wids or flags.tolist() != wflags or rows.shape != (len(wids), 64):
            return "ids and flags" + where
        if any(not np.array_equal(a, b) for a, b in zip(rows, wrows)):
            return "rows" + where
    return None


def _check_minimizers(path, desc, want, set_block):
    from kmerdb_amd import minimizer
    k, w = desc["k"], desc["w"]
    run = lambda B: list(minimizer.minimizers_file(path, k, w, canonical=desc["canonical"], order=fuzz_records.ORDER_NAMES[desc["order"]], block_bytes=B))
    sizes = [desc["block_bytes"], None]
    while sizes:
        B = sizes.pop(0)
        where = " at block_bytes=%s" % B
        if "raises" in want:
            if not _raises(lambda: run(B), want["raises"]):
                return "no refusal" + where
            continue
        try:
            rows = run(B)
        except ValueError as e:
            if REFUSED not in str(e) or B is None or desc.get("refused"):
                raise
            desc["refused"] = True                                            # documented; the case must pass at the bound
            sizes.insert(0, max(refusal_bound(desc["_text"], k, w), 4 * (k + w)))
            continue
        if [(r[0], r[1]) for r in rows] != [(rid, len(s)) for rid, s in want["records"]]:
            return "ids and lengths" + where
        for got, (pos, ids, strand) in zip(rows, want["lists"]):
            if got[2].dtype != np.int64 or not np.array_equal(got[2], pos) or not np.array_equal(got[3], ids) or not np.array_equal(got[4], strand):
                return "record %r%s" % (got[0], where)
    return None


def _check_score(path, desc, want, set_block):
    import math
    from kmerdb_amd import probability
    kdb = profile_file(desc["k"], desc["canonical"])
    for B in (desc["block_bytes"], None):
        rows = list(probability.score_file(path, kdb, pseudocount=desc["pseudocount"], block_bytes=B))
        where = " at block_bytes=%s" % B
        if [(r[0], r[1]) for r in rows] != [(rid, len(s)) for rid, s in want["records"]]:
            return "ids and lengths" + where
        for got, s, joins in zip(rows, want["scores"], want["joins"]):
            if got[2:5] != (s.windows, s.zero_windows, s.min_count):
                return "integers of record %r%s" % (got[0], where)
            lp = got[5]
            if s.log10_p is None or s.log10_p == float("-inf"):
                ok = math.isnan(lp) if s.log10_p is None else lp == float("-inf")
            else:
                ok = math.isfinite(lp) and sc.error(lp, s) <= sc.bound(s, fuzz_records.SCORE_PIECE, fuzz_records.SCORE_LANES, joins if B else 0)
            if not ok or not (got[6] == probability.log_odds_ratio(lp, desc["k"]) or math.isnan(lp)):
                return "log10_p of record %r%s" % (got[0], where)
    return None


class stand_ins:
    """with stand_ins(): the CPU restatements stand in the device calls' places -- composition.record_tables, minimizer.minimizers,
    probability.score_reads (and the upload of the profile) --, so that tables_file, codon_tables, minimizers_file and score_file run
    without a device: the reader, the joins and the host rules are the project's, the per-record answers the restatements'."""

    def __enter__(self):
        from kmerdb_amd import composition, minimizer, probability
        self.saved = [(composition, "record_tables", tb.record_tables_stub), (minimizer, "minimizers", mc.minimizers_stub),
                      (probability, "score_reads", sc.score_reads_stub), (probability, "_upload", lambda counts, device: counts)]
        self.saved = [(mod, name, getattr(mod, name), new) for mod, name, new in self.saved]
        for mod, name, _, new in self.saved:
            setattr(mod, name, new)
        return self

    def __exit__(self, *exc):
        for mod, name, old, _ in self.saved:
            setattr(mod, name, old)


_CHECK = {"parse": _check_parse, "tables": _check_tables, "codons": _check_codons, "minimizers": _check_minimizers, "score": _check_score}


def _set_block_bytes(value):
    """parsefile has no block_bytes argument: the reader's default is what it reads with"""
    from kmerdb_amd import reader
    reader.BLOCK_BYTES = _set_block_bytes.default if value is None else int(value)


def check_case(desc, arrays, want=None, directory=None, oracle=None, set_block=None):
    """Write the file, run the layer and compare -> bool; desc["failed"] then names the first comparison that did not hold.  directory:
    where the files go (one folder per case under it); set_block(block_bytes or None):
    what sets the block size parsefile reads with (default: reader.BLOCK_BYTES, put back afterwards)."""
    from kmerdb_amd import reader
    if oracle is None and desc["layer"] == "parse":
        from oracle import kmer_oracle as oracle
        oracle.build()
    want = want_case(desc, arrays, oracle) if want is None else want
    with tempfile.TemporaryDirectory(dir=directory) as folder:
        path = os.path.join(folder, file_name(desc))
        with open(path, "wb") as f:
            f.write(arrays["data"])
        if desc["layer"] == "reader":
            failed, _ = check_reader(path, desc, want)
        else:
            _set_block_bytes.default = reader.BLOCK_BYTES
            desc["_text"] = arrays["text"]
            try:
                failed = _CHECK[desc["layer"]](path, desc, want, set_block or _set_block_bytes)
            finally:
                del desc["_text"]
                if set_block is None:
                    reader.BLOCK_BYTES = _set_block_bytes.default
    if failed:
        desc["failed"] = failed
    return failed is None


def run_cases(seed, budget_s=None, max_cases=None, layers=None, verbose=True, directory=None, set_block=None, first=0):
    """-> (cases run, description of the first failing case or None, minimizer cases refused at their block size, minimizer cases).
    Case `index` is of layer layers[index % len(layers)]; first: the index of the first case."""
    layers = list(layers) if layers else list(LAYERS)
    t_end = time.time() + budget_s if budget_s else None
    ncase, refused, nmin = 0, 0, 0
    with tempfile.TemporaryDirectory(dir=directory) as folder:
        while (t_end is None or time.time() < t_end) and (max_cases is None or ncase < max_cases):
            desc, arrays = draw(seed, first + ncase, layers[(first + ncase) % len(layers)])
            try:
                ok = check_case(desc, arrays, directory=folder, set_block=set_block)
            except Exception as e:  # noqa: BLE001 - an error of the layer is a failing case too: name the case before it goes up
                print("FAIL " + json.dumps(desc) + "  raised %s: %s" % (type(e).__name__, e), flush=True)
                raise
            ncase += 1
            nmin += desc["layer"] == "minimizers"
            refused += bool(desc.get("refused"))
            if verbose:
                print(("ok   " if ok else "FAIL ") + json.dumps(desc), flush=True)
            if not ok:
                return ncase, desc, refused, nmin
    return ncase, None, refused, nmin


if __name__ == "__main__":
    budget = float(sys.argv[1]) if len(sys.argv) > 1 else 120.0
    seed = int(sys.argv[2]) if len(sys.argv) > 2 else 12345
    only = [c for c in sys.argv[3].split(",") if c] if len(sys.argv) > 3 else None
    if only and any(c not in LAYERS for c in only):
        sys.exit("layers: " + ",".join(LAYERS))
    n, bad, refused, nmin = run_cases(seed, budget_s=budget, layers=only)
    if bad is not None:
        sys.exit(1)
    if refused > MAX_REFUSED * max(nmin, 1):
        sys.exit(f"{refused} of {nmin} minimizer cases were refused at their block size: more than {MAX_REFUSED:.0%}")
    print(f"{n} cases, all equal to the whole-record answers; {refused} of {nmin} minimizer cases refused at their block size and equal at the bound (seed {seed})")
