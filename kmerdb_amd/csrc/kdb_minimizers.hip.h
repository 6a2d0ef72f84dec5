// kdb_minimizers.hip.h -- the (w,k)-minimizers of every record (kdb_minimizers of include/kdbhip.h): per start
// position a key (the window's id, or the id mixed by an invertible hash), per run of w positions the leftmost smallest key, and the
// selected positions of every record packed into one list, ordered by (record, position).
//
// A record's start positions are cut into pieces of PIECE; one wave owns one piece (kdbplan::minimizer_piece has the ranges).
//
// select_kernel.  KEYS: the wave copies the residues behind its piece -- its own positions and w - 1 more on either side, cut at the
// record's ends -- into LDS as aligned 4-byte words; lane l then takes the l-th run of ceil(keys / 64) positions and rolls through it,
// one residue per step: the forward id shifts the new 2-bit code in at the bottom, the reverse complement's shifts its complement in
// at the top, and a counter of the residues since the last N says whether the window has an id (the code is formed and the letter
// checked again as window_id of kdb_tables.hip.h does).  The first k - 1 steps of a lane fill its window and emit nothing.  Keys go to
// LDS, 8 bytes each, +infinity = ~0 (a key is below 4^31).  SELECT: lane l takes position l, l + 64, ... of the piece's own and
// decides it alone, by the per-position form of the definition: L = the positions to its left, in a row, with a larger key, R = those
// to its right with a key at least as large, both inside the record and at most we - 1; it is selected iff its key is finite and
// L + R + 1 >= we.  Strictly larger on the left, at least as large on the right: of equal keys the leftmost wins.  The lanes step
// outwards together (step j reads the keys at distance j on both sides: consecutive lanes, consecutive 8-byte words) and the wave
// stops as soon as every lane is settled; a step costs two LDS reads, and there are at most w - 1 of them (poly-A takes them all).
// A position has one owner, so its flag has one writer: a byte per residue of the batch, written 64 in a row.  The piece's number of
// selected positions comes from ballots.
//
// LDS: 8 bytes x (PIECE + 2 (w - 1)) of keys and PIECE + 2 (w - 1) + k + 6 of residues per wave at the most: 22.5 KiB at w = 256,
// 18.2 KiB at w = 10; two waves to a workgroup, so three workgroups share the 160 KiB of a CU even at the largest w.  The launch asks
// for what the batch's widest piece needs (kdbplan::MinimizersLayout::lds_wave): 1.3 KiB per wave for reads of 150 bp.
//
// scan_*_kernel: the exclusive prefix sums of the pieces' counts in three launches (sums of blocks of SCAN_BLOCK, one workgroup over
// those sums, the blocks again) -- no workgroup waits for another.  A record's pieces are consecutive, so its count is a difference
// of two of the sums (record_counts_kernel).  The host reads the total, and where the caller's arrays hold it:
//
// emit_kernel: a wave per piece again: 64 flags at a time, a ballot, every selected lane's place from the popcount of the lanes below
// it, and the id, position and strand stored there -- the wave's selected lanes write one packed run.  The id is formed again from the
// window's k residues, read as five aligned 8-byte words (selected positions alone: about 2 / (w + 1) of all on random sequence).
// No scalar memory writes, no spinning, no waiting between workgroups, and a workgroup barrier only where every wave of the workgroup arrives.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/kdbhip.h"
#include "kdb_strands.hip.h"
#include "kdb_sweep_plan.cpp.h"

namespace kdbminimizers {

typedef unsigned long long u64;

constexpr int TPB = 128;                           // two waves: two pieces per workgroup
constexpr int WAVES = TPB / 64;
constexpr uint32_t PIECE = KDB_MINIMIZER_PIECE;    // start positions one wave owns
constexpr int MAX_K = KDB_MINIMIZER_MAX_K;
constexpr int MAX_W = KDB_MINIMIZER_MAX_W;
constexpr u64 NO_KEY = ~0ull;
constexpr int SCAN_TPB = 256, SCAN_ITEMS = 8;
constexpr uint32_t SCAN_BLOCK = SCAN_TPB * SCAN_ITEMS;
static_assert(MAX_K <= 31, "a key is below 2^62: ~0 is free for +infinity");
static_assert((size_t)WAVES * (8u * (PIECE + 2u * (MAX_W - 1)) + PIECE + 2u * (MAX_W - 1) + MAX_K + 13u) <= 64u * 1024u, "a workgroup's LDS stays below 64 KiB");

// the invertible mix of KDB_MINIMIZER_HASHED on [0, m], m = 4^k - 1
__host__ __device__ __forceinline__ u64 mix(u64 x, u64 m)
{
    x = (~x + (x << 21)) & m;
    x ^= x >> 24;
    x = (x + (x << 3) + (x << 8)) & m;
    x ^= x >> 14;
    x = (x + (x << 2) + (x << 4)) & m;
    x ^= x >> 28;
    x = (x + (x << 31)) & m;
    return x;
}

// the 2-bit code of a residue (A0 C1 G2 T3, kmer.py:44-49), and whether the letter is the one of that code
__device__ __forceinline__ bool residue_code(uint32_t c, uint32_t *t)
{
    *t = ((c >> 1) ^ (c >> 2)) & 3u;
    return c == ((0x54474341u /* "ACGT" */ >> (8u * *t)) & 0xFFu);
}

// grid: ceil(npieces / WAVES) workgroups, WAVES * lds_wave bytes of dynamic LDS.  piece_rec: the record of every piece, or null where
// every record is one piece; rec_piece0: nreads + 1 entries.  flags: a byte per residue of the batch; the byte of start position p of a
// record at offset s is flags[s + p].  count_out[piece] = the selected positions among the piece's own.
__global__ void __launch_bounds__(TPB)
select_kernel(const uint8_t *__restrict__ bases, const uint64_t *__restrict__ offs, const uint32_t *__restrict__ piece_rec,
              const uint32_t *__restrict__ rec_piece0, uint32_t npieces, int k, uint32_t w, int canonical, int order, uint32_t max_keys,
              uint32_t lds_wave, uint8_t *__restrict__ flags, uint32_t *__restrict__ count_out)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t piece = __builtin_amdgcn_readfirstlane(blockIdx.x * WAVES + wave);
    if (piece >= npieces) return;                                            // (no workgroup barrier anywhere below)
    u64 *keys = reinterpret_cast<u64 *>(lds + (size_t)wave * lds_wave);
    uint8_t *res = reinterpret_cast<uint8_t *>(keys + max_keys);

    const uint32_t rec = piece_rec ? piece_rec[piece] : piece;
    const uint64_t s = offs[rec];
    const uint64_t nwin = kdbplan::minimizer_positions(offs[rec + 1] - s, k);
    const kdbplan::MinimizerPiece pc = kdbplan::minimizer_piece(nwin, piece - rec_piece0[rec], PIECE, w);
    if (pc.count == 0) {                                                     // (wave-uniform: a record without a start position)
        if (lane == 0) count_out[piece] = 0;
        return;
    }
    const uint32_t we = (uint32_t)(nwin < (uint64_t)w ? nwin : (uint64_t)w);
    const uint32_t nkeys = (uint32_t)(pc.hi - pc.lo);                        // <= max_keys
    const uint32_t own0 = (uint32_t)(pc.first - pc.lo);                      // the piece's first own position among its keys

    // the residues [lo, hi + k - 1) of the record, as the aligned words that hold them (the buffer is the call's own allocation: aligned, padded)
    const uint64_t r0 = s + pc.lo, a0 = r0 & ~(uint64_t)3;
    const uint32_t sh = (uint32_t)(r0 - a0);
    const uint32_t nwords = (sh + nkeys + (uint32_t)k - 1u + 3u) / 4u;
    {
        const uint32_t *src = reinterpret_cast<const uint32_t *>(bases + a0);
        uint32_t *dst = reinterpret_cast<uint32_t *>(res);
        for (uint32_t i = lane; i < nwords; i += 64) dst[i] = src[i];
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");                    // the residues before the lanes read each other's
    __builtin_amdgcn_wave_barrier();

    // keys: lane l rolls through the positions [a, b) of the piece's keys
    {
        const uint32_t per = (nkeys + 63u) / 64u;
        const uint32_t a = lane * per, b = a + per < nkeys ? a + per : nkeys;
        const u64 mask = (1ull << (2 * k)) - 1ull;
        const int top = 2 * (k - 1);
        u64 fwd = 0, rcv = 0;
        uint32_t run = 0;
        if (a < b) {
#pragma unroll 4
            for (uint32_t j = a; j < b + (uint32_t)k - 1u; j++) {
                uint32_t t;
                const bool ok = residue_code(res[sh + j], &t);
                fwd = ((fwd << 2) | t) & mask;
                rcv = (rcv >> 2) | ((u64)(3u - t) << top);
                run = ok ? run + 1u : 0u;
                if (j >= a + (uint32_t)k - 1u) {
                    const u64 id = canonical && rcv < fwd ? rcv : fwd;
                    keys[j - ((uint32_t)k - 1u)] = run >= (uint32_t)k ? (order == KDB_MINIMIZER_HASHED ? mix(id, mask) : id) : NO_KEY;
                }
            }
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");                    // the keys before the lanes read each other's
    __builtin_amdgcn_wave_barrier();

    uint32_t selected = 0;
    for (uint32_t i0 = 0; i0 < pc.count; i0 += 64) {
        const uint32_t i = i0 + lane;
        const bool in = i < pc.count;
        const uint32_t at = own0 + (in ? i : 0u);                             // among the keys
        const uint64_t p = pc.first + i;                                      // in the record
        const u64 key = in ? keys[at] : NO_KEY;
        const bool finite = key != NO_KEY;
        uint32_t L = 0, R = 0;
        bool lrun = finite, rrun = finite;
        // j <= we - 1 <= w - 1: at - j >= 0 where p - j >= 0, and at + j < nkeys where p + j < nwin (the halo)
        for (uint32_t j = 1; j < we; j++) {
            if (lrun) {
                if (p >= (uint64_t)j && keys[at - j] > key) L++; else lrun = false;
            }
            if (rrun) {
                if (p + j < nwin && keys[at + j] >= key) R++; else rrun = false;
            }
            if (__ballot((lrun || rrun) && L + R + 1u < we) == 0) break;      // (wave-uniform)
        }
        const bool sel = finite && L + R + 1u >= we;
        if (in) flags[s + p] = sel ? 1 : 0;
        selected += (uint32_t)__builtin_popcountll(__ballot(sel));
    }
    if (lane == 0) count_out[piece] = selected;
}

// the exclusive prefix sum of v over the workgroup's SCAN_TPB threads and, in *total, the sum; every thread of the workgroup calls it
__device__ __forceinline__ uint32_t block_exclusive(uint32_t v, uint32_t *wave_sums, uint32_t *total)
{
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t inc = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t t = __shfl_up(inc, off);
        if (lane >= (uint32_t)off) inc += t;
    }
    if (lane == 63) wave_sums[wave] = inc;
    __syncthreads();
    uint32_t base = 0, tot = 0;
#pragma unroll
    for (uint32_t i = 0; i < SCAN_TPB / 64; i++) {
        const uint32_t x = wave_sums[i];
        base += i < wave ? x : 0u;
        tot += x;
    }
    __syncthreads();                                                          // (wave_sums may be written again)
    *total = tot;
    return base + inc - v;
}

// sums[b] = the sum of counts[b SCAN_BLOCK .. (b + 1) SCAN_BLOCK); grid: one workgroup per block
__global__ void __launch_bounds__(SCAN_TPB)
scan_sums_kernel(const uint32_t *__restrict__ counts, uint32_t n, uint32_t *__restrict__ sums)
{
    __shared__ uint32_t wave_sums[SCAN_TPB / 64];
    const uint64_t at = (uint64_t)blockIdx.x * SCAN_BLOCK + threadIdx.x * SCAN_ITEMS;
    uint32_t v = 0;
#pragma unroll
    for (int j = 0; j < SCAN_ITEMS; j++) v += at + j < n ? counts[at + j] : 0u;
    uint32_t total;
    (void)block_exclusive(v, wave_sums, &total);
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

// one workgroup: sums[0 .. nblocks) <- their exclusive prefix sums, *total_out <- the sum of all
__global__ void __launch_bounds__(SCAN_TPB)
scan_top_kernel(uint32_t *__restrict__ sums, uint32_t nblocks, uint32_t *__restrict__ total_out)
{
    __shared__ uint32_t wave_sums[SCAN_TPB / 64];
    uint32_t carry = 0;
    for (uint32_t i0 = 0; i0 < nblocks; i0 += SCAN_TPB) {                     // (the same trips for every thread)
        const uint32_t i = i0 + threadIdx.x;
        const uint32_t v = i < nblocks ? sums[i] : 0u;
        uint32_t total;
        const uint32_t ex = block_exclusive(v, wave_sums, &total);
        if (i < nblocks) sums[i] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0) *total_out = carry;
}

// out[i] = the sum of counts[0 .. i), i < n, with the blocks' own sums from scan_top_kernel
__global__ void __launch_bounds__(SCAN_TPB)
scan_apply_kernel(const uint32_t *__restrict__ counts, uint32_t n, const uint32_t *__restrict__ sums, uint32_t *__restrict__ out)
{
    __shared__ uint32_t wave_sums[SCAN_TPB / 64];
    const uint64_t at = (uint64_t)blockIdx.x * SCAN_BLOCK + threadIdx.x * SCAN_ITEMS;
    uint32_t c[SCAN_ITEMS], v = 0;
#pragma unroll
    for (int j = 0; j < SCAN_ITEMS; j++) { c[j] = at + j < n ? counts[at + j] : 0u; v += c[j]; }
    uint32_t total;
    uint32_t run = block_exclusive(v, wave_sums, &total) + sums[blockIdx.x];
#pragma unroll
    for (int j = 0; j < SCAN_ITEMS; j++) {
        if (at + j < n) out[at + j] = run;
        run += c[j];
    }
}

// one thread per record: piece_off has npieces + 1 entries
__global__ void __launch_bounds__(256)
record_counts_kernel(const uint32_t *__restrict__ piece_off, const uint32_t *__restrict__ rec_piece0, uint64_t nreads, u64 *__restrict__ counts_out)
{
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= nreads) return;
    counts_out[r] = (u64)(piece_off[rec_piece0[r + 1]] - piece_off[rec_piece0[r]]);
}

// grid: ceil(npieces / WAVES) workgroups.  The piece's selected positions go to [piece_off[piece], piece_off[piece + 1]) of the three lists
// (strand_out may be null), which hold piece_off[npieces] entries.
__global__ void __launch_bounds__(TPB)
emit_kernel(const uint8_t *__restrict__ bases, const uint64_t *__restrict__ offs, const uint32_t *__restrict__ piece_rec,
            const uint32_t *__restrict__ rec_piece0, uint32_t npieces, int k, int canonical, const uint8_t *__restrict__ flags,
            const uint32_t *__restrict__ piece_off, u64 *__restrict__ ids_out, uint32_t *__restrict__ pos_out, uint8_t *__restrict__ strand_out)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t piece = __builtin_amdgcn_readfirstlane(blockIdx.x * WAVES + (threadIdx.x >> 6));
    if (piece >= npieces) return;
    uint32_t out = piece_off[piece];
    const uint32_t end = piece_off[piece + 1];
    if (out == end) return;                                                   // (wave-uniform)
    const uint32_t rec = piece_rec ? piece_rec[piece] : piece;
    const uint64_t s = offs[rec];
    const uint64_t nwin = kdbplan::minimizer_positions(offs[rec + 1] - s, k);
    const kdbplan::MinimizerPiece pc = kdbplan::minimizer_piece(nwin, piece - rec_piece0[rec], PIECE, 1);
    for (uint32_t i0 = 0; i0 < pc.count && out < end; i0 += 64) {
        const uint32_t i = i0 + lane;
        const uint64_t p = pc.first + i;
        const bool sel = i < pc.count && flags[s + p] != 0;
        const u64 m = __ballot(sel);
        if (m == 0) continue;                                                 // (wave-uniform)
        const uint32_t to = out + (uint32_t)__builtin_popcountll(m & ((1ull << lane) - 1ull));
        out += (uint32_t)__builtin_popcountll(m);
        if (sel && to < end) {                                                // (to < end always: the counts are these flags')
            // the five aligned 8-byte words that hold the window's k <= 31 residues, all asked for before the first is used (the buffer
            // is padded for them), shifted so that the window begins at byte 0
            const uint64_t at = s + p;
            const u64 *q = reinterpret_cast<const u64 *>(bases) + (at >> 3);
            const uint32_t sh = ((uint32_t)at & 7u) * 8u;
            u64 x[5], y[4];
#pragma unroll
            for (int j = 0; j < 5; j++) x[j] = q[j];
#pragma unroll
            for (int j = 0; j < 4; j++) y[j] = sh ? (x[j] >> sh) | (x[j + 1] << (64u - sh)) : x[j];
            u64 fwd = 0;
#pragma unroll
            for (int j = 0; j < MAX_K; j++) {
                if (j < k) {
                    uint32_t t;
                    (void)residue_code((uint32_t)(y[j >> 3] >> (8 * (j & 7))) & 0xFFu, &t);   // (selected: every residue of the window is ACGT)
                    fwd = (fwd << 2) | t;
                }
            }
            const u64 rcv = kdbstrands::rc_id(fwd, k);
            const bool minus = canonical && rcv < fwd;
            ids_out[to] = minus ? rcv : fwd;
            pos_out[to] = (uint32_t)p;
            if (strand_out) strand_out[to] = minus ? 1 : 0;
        }
    }
}

}  // namespace kdbminimizers
