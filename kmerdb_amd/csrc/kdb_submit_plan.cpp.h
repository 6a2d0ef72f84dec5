// kdb_submit_plan.cpp.h -- the cut of one kdb_submit / kdb_submit_pinned / kdb_submit_ex call into staging pieces (plain C++, no HIP and
// nothing of the engine's: tests/c/submit_plan_check.cpp compiles it alone, runs it under the sanitizers and prints the pieces for
// tests/submit_cases.py to be compared with).  The caller's records lie one behind the other in its buffer, record i at bytes
// [offs[i], offs[i + 1]).  A piece is what one staging buffer takes: the longest run of whole records that fits `cap` bytes and
// `max_recs` records, or -- where one record alone is longer than a buffer -- `cap` bytes of it, the next piece beginning k - 1 bytes
// before this one ends, so that every k-byte window of the record lies whole in exactly one piece.  The buffer size, the record count
// and k are arguments: the engine has the real ones (stage_bytes, stage_reads).
#pragma once
#include <cstddef>
#include <cstdint>

#include <algorithm>

namespace kdbplan {

enum SubmitError { SUBMIT_OK = 0, SUBMIT_ENDS /* offs[nreads] < offs[0] or > nbytes */, SUBMIT_RISE /* a record ends before it begins */ };

// what the engine says of the two (SUBMIT_RISE with the index of the offset that falls)
constexpr const char *SUBMIT_ENDS_TEXT = "read_offsets exceed nbytes";
constexpr const char *SUBMIT_RISE_FORMAT = "read_offsets not monotone at %zu";

// Bytes [start, start + nbytes) of the caller's buffer hold the records rec0 .. rec0 + nrecs, the first from where an earlier piece (or
// an earlier call) left it if first_is_continuation, the last -- then the only one -- up to somewhere inside it if ends_inside_record.
struct SubmitPiece {
    uint64_t start = 0, nbytes = 0;
    size_t rec0 = 0, nrecs = 0;
    bool first_is_continuation = false, ends_inside_record = false;
};

struct SubmitCutter {
    const uint64_t *offs;
    size_t nreads, max_recs;
    uint64_t cap, overlap;
    size_t r = 0;                    // the record the next piece begins with (or goes on with)
    bool cont;                       // the next piece continues a record split across buffers (or across calls)
    uint64_t carry;                  // where that piece starts
    size_t bad = 0;                  // SUBMIT_RISE: the index of the offset that falls

    // first_continues: record 0 goes on where an earlier call ended, its bytes here begin at offs[0].  nreads >= 1, cap >= k, max_recs >= 1.
    SubmitCutter(const uint64_t *offs_, size_t nreads_, bool first_continues, uint64_t cap_, size_t max_recs_, int k)
        : offs(offs_), nreads(nreads_), max_recs(max_recs_), cap(cap_), overlap((uint64_t)(k - 1)), cont(first_continues), carry(first_continues ? offs_[0] : 0) {}

    // before anything is cut; offs[nreads] < nbytes is accepted (the bytes behind are no record's), and so is offs[0] > 0
    static SubmitError check_ends(const uint64_t *offs, size_t nreads, uint64_t nbytes)
    {
        return offs[nreads] < offs[0] || offs[nreads] > nbytes ? SUBMIT_ENDS : SUBMIT_OK;
    }

    bool done() const { return r >= nreads; }

    // The next piece, its offsets relative to p.start in local[0 .. p.nrecs] (0 first, p.nbytes last; an array of max_recs + 1).  Only the
    // offsets of a piece of whole records are read one by one, and these are checked to rise on the way: what was cut before a refusal
    // stays cut.  (The search reads offsets that are not yet checked.  It stays inside (r, rmax] whatever they hold, and whichever of
    // them it settles on, every offset up to there is then compared with the one before.)
    SubmitError next(uint64_t *local, SubmitPiece &p)
    {
        p.first_is_continuation = cont;
        p.start = cont ? carry : offs[r];
        p.rec0 = r;
        const size_t rmax = nreads - r < max_recs ? nreads : r + max_recs;
        const uint64_t *ub = std::upper_bound(offs + r + 1, offs + rmax + 1, p.start + cap);
        const size_t r1 = (size_t)(ub - offs) - 1;      // offs[r1] <= start + cap
        local[0] = 0;
        if (r1 <= r) {                                   // the record at r alone exceeds a buffer: tile it with k - 1 overlap
            p.nbytes = cap; p.nrecs = 1; local[1] = cap;
            carry = p.start + cap - overlap; cont = true;
        } else {
            p.nbytes = offs[r1] - p.start; p.nrecs = r1 - r;
            uint64_t prev = p.start;
            for (size_t i = 1; i <= p.nrecs; i++) {
                const uint64_t o = offs[r + i];
                if (o < prev) { bad = r + i; return SUBMIT_RISE; }
                prev = o;
                local[i] = o - p.start;
            }
            r = r1; cont = false;
        }
        p.ends_inside_record = cont;
        return SUBMIT_OK;
    }
};

}  // namespace kdbplan
