// kdb_score.hip.h -- reads scored against a finished profile: the log-probability of every record under the (k-1)-order Markov chain
// that the 4^k count vector defines (the reference's markov_probability, kmerdb/probability.py:36-151).
//
// With v the vector, a the pseudocount and total' = total + a 4^k, a window w whose k residues are all ACGT and lie inside its record
// ("scored": exactly the windows kdb_window_ids of a forward engine emits an id for) has
//     c(w) = v[id(w)] + a                      (canonical profile: v[min(id, rc(id))] + a)
//     D(w) = Sum over x in ACGT of c(prefix_{k-1}(w) x): the four bins 4 (id >> 2) .. + 3, 32 aligned bytes of a forward profile
// and contributes  ln c(w) - ln total'  if it is the first scored window of its record and  ln c(w) - ln D(w)  otherwise
// (probability.py:75 and :91-99, :130-133); -inf where c(w) is 0.  log10_p is the sum of the terms divided by ln 10, once per record.
//
// Shape.  A record's windows are cut into pieces of PIECE.  One wave scores one piece: lane l takes windows l, l + 64, ... of the piece in
// that order, forms each id from the residues directly (k <= 17 bytes in three aligned 8-byte words, neighbouring lanes read the same words), fetches the four bins
// of the transition and adds the term to its own float64 sum.  Every lane works through WINDOWS_IN_FLIGHT windows at a time: all their
// ids first, then all their loads, then the logarithms -- the kernel waits on random 32-byte reads of a table of up to 128 GiB and wants
// many of them outstanding.  The 64 lane sums go through the fixed butterfly of wave_sum_fixed (kdb_pairstats.hip.h).  The first scored
// window of a PIECE is kept out of the lane sums: the piece hands c and D of it on, as float64, and record_kernel -- one thread per
// record, pieces in order -- knows whether it is the first of the record (term against total') or not (term against D).  So the order of
// the additions is: per lane PIECE / 64 terms in window order, six butterfly levels, then per piece its first term and its sum.  It
// depends on the record's length (and on which of its windows hold an N) and on these constants alone: not on the grid, the batch or the
// record's place in it.  No atomics.  The integer outputs (windows, windows whose bin is 0, smallest bin) take the same route in integers.
// D reaches 2^66: it is formed in 128 bits and rounded to float64 once, to nearest even (to_double).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>

#include "../../include/kdbhip.h"
#include "kdb_gram.hip.h"
#include "kdb_pairstats.hip.h"
#include "kdb_strands.hip.h"

namespace kdbscore {

using kdbgram::u128;
typedef unsigned long long u64;

constexpr int TPB = 256;                           // four waves: four pieces per workgroup
constexpr int PIECE = KDB_SCORE_PIECE;             // windows one wave scores
constexpr int WINDOWS_IN_FLIGHT = 4;               // per lane: 4 x 32 bytes of the vector asked for before the first is used
static_assert(KDB_SCORE_LANES == 64, "one wave of gfx950");
static_assert(PIECE % (64 * WINDOWS_IN_FLIGHT) == 0, "a piece is whole rounds of the wave");

struct PieceOut {
    double sum;            // the terms of the piece's scored windows but the first, all taken as transitions
    double first_c;        // c of the piece's first scored window (0.0: the count is 0, the term is -inf)
    double first_d;        // D of it
    u64 min_count;         // over the piece's scored windows; ~0 if none
    uint32_t windows;      // scored windows of the piece, the first one included
    uint32_t zero_windows; // those whose bin is 0 (before the pseudocount)
};

// round to nearest even, once: the top 64 bits with a sticky last bit go through the hardware's u64 -> f64 conversion (64 > 53 + 2 bits,
// so the sticky bit decides ties as the dropped bits would), the power of two is exact
__device__ __forceinline__ double to_double(u128 v)
{
    const u64 hi = (u64)(v >> 64), lo = (u64)v;
    if (hi == 0) return (double)lo;
    const int s = 64 - __builtin_clzll(hi);                                   // 1..64 bits above the low word
    const u64 dropped = s == 64 ? lo : (lo & ((1ull << s) - 1ull));
    const u64 top = (s == 64 ? hi : ((hi << (64 - s)) | (lo >> s))) | (dropped != 0 ? 1ull : 0ull);
    return ldexp((double)top, s);
}

// ln c - ln d, -inf for a count of zero (also where d is 0: then c is)
__device__ __forceinline__ double term(double c, double d) { return c > 0.0 ? log(c) - log(d) : -INFINITY; }

// Which bytes of the five 32-bit words a window's residues arrive in belong to it (k <= 17 residues; byte 0 of a word is the first residue)
struct IdMasks {
    uint32_t m[5];
    __device__ __forceinline__ explicit IdMasks(int k)
    {
#pragma unroll
        for (int i = 0; i < 5; i++) {
            const int n = k - 4 * i;
            m[i] = n >= 4 ? 0xFFFFFFFFu : n <= 0 ? 0u : ((1u << (8 * n)) - 1u);
        }
    }
};

// the id of a window, or false if one of its residues is not ACGT (upper case: what the engine counts).  The residues come as the three
// aligned 8-byte words that hold them, loaded by the caller for all its windows before the first is decoded (byte loads would be k loads
// in a row per window, each waiting for the one before); the words reach up to 23 bytes past the window's start, into the padding behind
// the buffer at its very end (never used: IdMasks).  Four residues become one byte of id with the dot product of encode16 (kdb_kernels.hip.h).
__device__ __forceinline__ bool window_id(const u64 (&w)[3], uint32_t s /* 8 x the window's offset in w[0] */, int k, const IdMasks &masks, uint64_t *id_out)
{
    const u64 lo = s ? (w[0] >> s) | (w[1] << (64u - s)) : w[0];
    const u64 mid = s ? (w[1] >> s) | (w[2] << (64u - s)) : w[1];
    const uint32_t x[5] = {(uint32_t)lo, (uint32_t)(lo >> 32), (uint32_t)mid, (uint32_t)(mid >> 32), (uint32_t)(w[2] >> s)};
    uint64_t id = 0;
    uint32_t bad = 0;
#pragma unroll
    for (int i = 0; i < 5; i++) {
        const uint32_t t = ((x[i] >> 1) ^ (x[i] >> 2)) & 0x03030303u;         // A0 C1 G2 T3 (kmer.py:44-49)
        bad |= (x[i] ^ __builtin_amdgcn_perm(0u, 0x54474341u /* "ACGT" */, t)) & masks.m[i];      // the letter of that code, looked up again
        id = (id << 8) | __builtin_amdgcn_udot4(t, 0x01041040u, 0u, false);   // byte0 * 64 + byte1 * 16 + byte2 * 4 + byte3
    }
    *id_out = id >> (40 - 2 * k);
    return bad == 0;
}

struct Bins { u64 x[4]; };

// grid: ceil(npieces / 4) workgroups.  piece_rec: the record of every piece, or null where every record is one piece (piece p = record p);
// rec_piece0: nreads + 1 entries, the first piece of every record.
__global__ void __launch_bounds__(TPB, 2)
piece_kernel(const uint8_t *__restrict__ bases, const uint64_t *__restrict__ offs, const uint32_t *__restrict__ piece_rec,
             const uint32_t *__restrict__ rec_piece0, uint32_t npieces, const u64 *__restrict__ v, int k, int canonical, u64 pseudocount,
             PieceOut *__restrict__ out)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t piece = __builtin_amdgcn_readfirstlane(blockIdx.x * (TPB / 64) + (threadIdx.x >> 6));
    if (piece >= npieces) return;
    const uint32_t rec = piece_rec ? piece_rec[piece] : piece;
    const uint64_t s = offs[rec], e = offs[rec + 1];
    const uint64_t len = e - s, nwin = len >= (uint64_t)k ? len - (uint64_t)k + 1 : 0;   // (a continuation piece may be shorter than k)
    const uint64_t w0 = (uint64_t)(piece - rec_piece0[rec]) * PIECE;
    const uint32_t nw = (uint32_t)(nwin - w0 < (uint64_t)PIECE ? nwin - w0 : (uint64_t)PIECE);
    const u64 *words = reinterpret_cast<const u64 *>(bases);                  // (the buffer is the call's own allocation: aligned, padded)
    const uint64_t at0 = s + w0;                                              // the piece's first window starts at this residue
    const IdMasks masks(k);

    double sum = 0.0, first_c = 0.0, first_d = 0.0;
    u64 mn = ~0ull;
    uint32_t windows = 0, zeros = 0;
    bool found = false;                                                       // (wave-uniform) the piece's first scored window is behind us
    for (uint32_t j0 = 0; j0 < nw; j0 += 64 * WINDOWS_IN_FLIGHT) {
        uint64_t id[WINDOWS_IN_FLIGHT];
        bool ok[WINDOWS_IN_FLIGHT], is_first[WINDOWS_IN_FLIGHT];
        Bins b[WINDOWS_IN_FLIGHT];
        u64 w[WINDOWS_IN_FLIGHT][3];
        uint32_t sh[WINDOWS_IN_FLIGHT];
#pragma unroll
        for (int u = 0; u < WINDOWS_IN_FLIGHT; u++) {
            const uint32_t j = j0 + 64u * u + lane;
            const uint64_t at = at0 + j;
            ok[u] = j < nw;
            sh[u] = ((uint32_t)at & 7u) * 8u;
            w[u][0] = w[u][1] = w[u][2] = 0;
            if (ok[u]) {
                const u64 *q = words + (at >> 3);
                w[u][0] = q[0]; w[u][1] = q[1]; w[u][2] = q[2];
            }
        }
#pragma unroll
        for (int u = 0; u < WINDOWS_IN_FLIGHT; u++) {
            id[u] = 0;
            ok[u] = ok[u] && window_id(w[u], sh[u], k, masks, &id[u]);
            is_first[u] = false;
            if (!found) {
                const u64 m = __ballot(ok[u]);
                if (m) { found = true; is_first[u] = lane == (uint32_t)__builtin_ctzll(m); }
            }
        }
#pragma unroll
        for (int u = 0; u < WINDOWS_IN_FLIGHT; u++) {
            b[u].x[0] = b[u].x[1] = b[u].x[2] = b[u].x[3] = 0;
            if (!ok[u]) continue;
            const uint64_t base = id[u] & ~3ull;
            if (!canonical) {
                const ulonglong2 *q = reinterpret_cast<const ulonglong2 *>(v + base);       // 32 aligned bytes (k = 1: the whole vector)
                const ulonglong2 lo = q[0], hi = q[1];
                b[u].x[0] = lo.x; b[u].x[1] = lo.y; b[u].x[2] = hi.x; b[u].x[3] = hi.y;
            } else {
#pragma unroll
                for (int x = 0; x < 4; x++) {
                    const uint64_t f = base + (uint64_t)x, r = kdbstrands::rc_id(f, k);
                    b[u].x[x] = v[f < r ? f : r];
                }
            }
        }
#pragma unroll
        for (int u = 0; u < WINDOWS_IN_FLIGHT; u++) {
            if (!ok[u]) continue;
            const uint32_t sel = (uint32_t)id[u] & 3u;
            const u64 cv = sel == 0 ? b[u].x[0] : sel == 1 ? b[u].x[1] : sel == 2 ? b[u].x[2] : b[u].x[3];
            windows++;
            zeros += cv == 0 ? 1u : 0u;
            mn = cv < mn ? cv : mn;
            const u128 c = (u128)cv + pseudocount;
            const u128 d = (u128)b[u].x[0] + b[u].x[1] + b[u].x[2] + b[u].x[3] + (u128)pseudocount * 4u;
            const double cd = to_double(c), dd = to_double(d);
            if (is_first[u]) { first_c = cd; first_d = dd; }
            else sum += term(cd, dd);
        }
    }
    // the lane that holds the first scored window is the only one with non-zero first_c / first_d: the same butterfly hands them on exactly
    sum = kdbpair::wave_sum_fixed(sum);
    first_c = kdbpair::wave_sum_fixed(first_c);
    first_d = kdbpair::wave_sum_fixed(first_d);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        windows += __shfl_down(windows, off);
        zeros += __shfl_down(zeros, off);
        const u64 m2 = __shfl_down(mn, off);
        mn = m2 < mn ? m2 : mn;
    }
    if (lane == 0) {
        PieceOut o;
        o.sum = sum; o.first_c = first_c; o.first_d = first_d; o.min_count = mn; o.windows = windows; o.zero_windows = zeros;
        out[piece] = o;
    }
}

// one thread per record: its pieces in order
__global__ void __launch_bounds__(256)
record_kernel(const PieceOut *__restrict__ pieces, const uint32_t *__restrict__ rec_piece0, uint64_t nreads, double total, int first_continues,
              double *__restrict__ log10_p, u64 *__restrict__ windows_out, u64 *__restrict__ zero_out, u64 *__restrict__ min_out)
{
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= nreads) return;
    double acc = 0.0;
    u64 windows = 0, zeros = 0, mn = ~0ull;
    bool seen = r == 0 && first_continues;                                    // a scored window of this record lies before: no initial term
    for (uint32_t p = rec_piece0[r]; p < rec_piece0[r + 1]; p++) {
        const PieceOut o = pieces[p];
        if (o.windows == 0) continue;
        acc += term(o.first_c, seen ? o.first_d : total);
        acc += o.sum;
        seen = true;
        windows += o.windows;
        zeros += o.zero_windows;
        mn = o.min_count < mn ? o.min_count : mn;
    }
    log10_p[r] = windows ? acc / 2.302585092994045684 : (double)NAN;
    windows_out[r] = windows;
    zero_out[r] = zeros;
    min_out[r] = mn;
}

}  // namespace kdbscore
