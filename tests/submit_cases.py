"""The cut of one submit into staging pieces, restated from its rule (test infrastructure: the product never imports this; the product's
cut is kdbplan::SubmitCutter of kmerdb_amd/csrc/kdb_submit_plan.cpp.h).

The caller's record i lies at bytes [offs[i], offs[i + 1]) of its buffer.  A staging buffer takes `cap` bytes and `max_recs` records.
With start = where the piece before left a record it could not finish (or, for the first piece of a call that continues an earlier
one, offs[0]), else offs[r]: the piece is the records r .. r1 - 1 for the largest r1 in (r, min(nreads, r + max_recs)] with
offs[r1] <= start + cap; where there is none it is `cap` bytes of record r alone, and the next piece starts k - 1 bytes before this
one ends and continues the record.  Offsets that fall are refused, by index, when the piece they lie in is cut: the pieces before stay.
(For offsets that do not rise the rule settles r1 only where every offset in reach fits or none does: the refusal cases here are such.)
"""

ENDS_TEXT = "read_offsets exceed nbytes"
RISE_TEXT = "read_offsets not monotone at {0}"


def offsets_of(lengths, first=0):
    o = [first]
    for n in lengths:
        o.append(o[-1] + n)
    return o


def cut(offs, first_continues, cap, max_recs, k, nbytes=None):
    """-> (pieces, refusal): pieces are dicts start, nbytes, rec0, nrecs, cont, inside, local; refusal None, ("ends", 0) or ("rise", index)"""
    n = len(offs) - 1
    if offs[n] < offs[0] or offs[n] > (offs[n] if nbytes is None else nbytes):
        return [], ("ends", 0)
    pieces, r, cont, carry = [], 0, bool(first_continues), offs[0]
    while r < n:
        start = carry if cont else offs[r]
        fits = [j for j in range(r + 1, min(n, r + max_recs) + 1) if offs[j] <= start + cap]
        if not fits:
            pieces.append(dict(start=start, nbytes=cap, rec0=r, nrecs=1, cont=int(cont), inside=1, local=[0, cap]))
            carry, cont = start + cap - (k - 1), True
            continue
        r1, prev = max(fits), start
        for i in range(r + 1, r1 + 1):
            if offs[i] < prev:
                return pieces, ("rise", i)
            prev = offs[i]
        pieces.append(dict(start=start, nbytes=offs[r1] - start, rec0=r, nrecs=r1 - r, cont=int(cont), inside=0,
                           local=[0] + [offs[i] - start for i in range(r + 1, r1 + 1)]))
        r, cont = r1, False
    return pieces, None


def check_pieces(offs, first_continues, pieces, cap, max_recs, k):
    """what must hold of the pieces of offsets that rise, whoever cut them"""
    n = len(offs) - 1
    spans = {r: [] for r in range(n)}                       # per record: the byte ranges of it that the pieces hold, in order
    for i, p in enumerate(pieces):
        assert 1 <= p["nrecs"] <= max_recs and p["nbytes"] <= cap, p
        assert p["local"][0] == 0 and p["local"][-1] == p["nbytes"] and len(p["local"]) == p["nrecs"] + 1, p
        assert p["cont"] == (pieces[i - 1]["inside"] if i else int(bool(first_continues))), p
        for j in range(p["nrecs"]):
            spans[p["rec0"] + j].append((p["start"] + p["local"][j], p["start"] + p["local"][j + 1]))
        if p["cont"] and i:                                 # the rest of a record this call has tiled: a window at least
            assert p["local"][1] >= k, p
        if not p["inside"]:                                 # a run of whole records is maximal
            r1 = p["rec0"] + p["nrecs"]
            assert r1 == n or p["nrecs"] == max_recs or offs[r1 + 1] > p["start"] + cap, p
    for r in range(n):
        s = spans[r]
        assert s and s[0][0] == offs[r] and s[-1][1] == offs[r + 1], (r, s)
        for (a0, a1), (b0, b1) in zip(s, s[1:]):
            assert b0 == a1 - (k - 1) and a1 - a0 == cap, (r, s)
        for w in range(offs[r], offs[r + 1] - k + 1):       # every k-byte window of the record lies whole in exactly one piece
            assert sum(1 for a, b in s if a <= w and w + k <= b) == 1, (r, w, s)


def edges(cap, max_recs, k):
    """the submits at the edges of the cut -> (name, record lengths, offs[0], first_continues, bytes behind the last record,
    [(nbytes, nrecs, cont, inside) of every piece])"""
    m, v = max_recs, k - 1
    assert m >= 3 and (m + 1) * k <= cap and cap > 3 * k
    return [
        ("a record of one buffer is a whole piece", [cap], 0, 0, 0, [(cap, 1, 0, 0)]),
        ("one byte more: a tile and a window", [cap + 1], 0, 0, 0, [(cap, 1, 0, 1), (k, 1, 1, 0)]),
        ("a tile and a remainder of one buffer", [2 * cap - v], 0, 0, 0, [(cap, 1, 0, 1), (cap, 1, 1, 0)]),
        ("one byte more: two tiles and a window", [2 * cap - v + 1], 0, 0, 0, [(cap, 1, 0, 1), (cap, 1, 1, 1), (k, 1, 1, 0)]),
        ("one record more than a buffer lists", [k] * (m + 1), 0, 0, 0, [(m * k, m, 0, 0), (k, 1, 0, 0)]),
        ("the same with empty records among them", [k if i % 2 == 0 else 0 for i in range(m + 1)], 0, 0, 0,
         [(k * ((m + 1) // 2), m, 0, 0), (k if m % 2 == 0 else 0, 1, 0, 0)]),
        ("a full list that fills the buffer to the byte", [cap - (m - 1) * k] + [k] * (m - 1), 0, 0, 0, [(cap, m, 0, 0)]),
        ("a record that fits where the one behind it does not", [k, cap - 2 * k, 2 * k], 0, 0, 0, [(cap - k, 2, 0, 0), (2 * k, 1, 0, 0)]),
        ("short records join the rest of a tiled one", [cap + 1, k, k], 0, 0, 0, [(cap, 1, 0, 1), (3 * k, 3, 1, 0)]),
        ("a call that continues, its first record longer than a buffer", [cap + 1], 7, 1, 0, [(cap, 1, 1, 1), (k, 1, 1, 0)]),
        ("bytes in front of the first record are skipped", [k, k], 7, 0, 0, [(2 * k, 2, 0, 0)]),
        ("bytes behind the last record are accepted", [k, k], 0, 0, 9, [(2 * k, 2, 0, 0)]),
    ]


def refusals(cap, max_recs, k):
    """-> (offsets, nbytes, pieces cut before the refusal, (kind, index))"""
    m = max_recs
    falls = offsets_of([k] * m) + [m * k + 10, m * k + 5, m * k + 20]       # the second piece's offsets all fit the buffer; its second falls
    assert falls[-1] <= m * k + cap
    return [([5, 3], 9, 0, ("ends", 0)), ([0, 10], 9, 0, ("ends", 0)), ([0, 4, 2], 1, 0, ("ends", 0)),
            (falls, falls[-1], 1, ("rise", m + 2)), ([0, 4, 2, 9], 9, 0, ("rise", 2))]
