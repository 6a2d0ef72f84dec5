// kdb_tables.hip.h -- one small k-mer table per record (kdb_record_tables of include/kdbhip.h): the frame-0 codon
// counts of every CDS (the reference's get_codons_in_order / count_codons, kmerdb/codons.py:175-273, at k = 3, stride 3) and, at stride 1,
// the composition vector of every contig.
//
// A record's windows start at phase + i stride and are cut into pieces of PIECE.  One wave counts one piece into 4^k uint32 of LDS that
// are its own (k <= 6: 16 KiB, four waves to a workgroup, 64 KiB at most; the LDS a launch asks for follows k): it zeroes them, lane l
// takes windows l, l + 64, ... of the piece, WINDOWS_IN_FLIGHT at a time -- the two aligned 8-byte words that hold a window's k <= 6
// residues are loaded for all of them before the first id is formed, as piece_kernel of kdb_score.hip.h reads its three -- and adds 1 at
// the id with a non-returning LDS add.  Where all counted windows of a round of 64 lanes have one id (poly-A, and every round at k = 1
// on a run of one letter), one lane adds their number instead: 64 adds to one word would go through the LDS one after the other.  At
// k <= 3 the 64 lanes of a round meet on 4^k <= 64 words whatever the layout; the adds that share a word are serialised by the LDS, and
// a round is still one instruction.  Nothing but this wave touches its words, so the three phases (zero, add, read) are ordered by the
// wave's own program order; the fences between them only keep the compiler from moving LDS accesses across.
//
// Then the wave writes its row.  The only piece of its record stores all 4^k entries, zeros included, 16 bytes per lane and coalesced:
// such rows need no memset.  A piece of a longer record adds its non-zero bins to a row that tables_zero_kernel has zeroed, with
// ordinary global atomic adds: integers add in any order, so nothing depends on the grid.  The piece's four numbers (counted, skipped,
// the ids at its smallest and largest counted position) come from wave reductions and go to tables_record_kernel, one thread per record,
// which joins them in piece order.  No scalar memory writes, no spinning, no waiting between workgroups.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/kdbhip.h"
#include "kdb_strands.hip.h"
#include "kdb_sweep_plan.cpp.h"

namespace kdbtables {

typedef unsigned long long u64;

constexpr int TPB = 256;                           // four waves: four pieces per workgroup
constexpr int WAVES = TPB / 64;
constexpr uint32_t PIECE = KDB_TABLES_PIECE;       // windows one wave counts
constexpr int MAX_K = KDB_TABLES_MAX_K;
constexpr int WINDOWS_IN_FLIGHT = 4;               // per lane: 4 x 16 bytes of residues asked for before the first is used
constexpr uint32_t NO_FIRST = 0xFFFFFFFFu;
static_assert(PIECE % (64 * WINDOWS_IN_FLIGHT) == 0, "a piece is whole rounds of the wave");
static_assert((uint64_t)PIECE << (2 * MAX_K) <= (1ull << 31), "(window of the piece, id) is one 32-bit key");

struct PieceOut {
    uint32_t counted, skipped;
    int32_t first_id, last_id;         // of the piece's counted windows with the smallest / largest position; -1 without one
};

// the LDS of a launch: a table per wave
constexpr size_t lds_bytes(int k) { return (size_t)WAVES * sizeof(uint32_t) << (2 * k); }

// the id of the window whose k <= 6 residues begin `s` / 8 bytes into w0 (w1: the next 8 bytes), or false if one of them is not ACGT.
// Four residues become one byte of id with the dot product of encode16 (kdb_kernels.hip.h); the bytes behind the k-th are masked out of
// the check and shifted out of the id (at the very end of the buffer they are its padding).
__device__ __forceinline__ bool window_id(u64 w0, u64 w1, uint32_t s, int k, uint32_t mask0, uint32_t mask1, uint32_t *id_out)
{
    const u64 lo = s ? (w0 >> s) | (w1 << (64u - s)) : w0;
    const uint32_t x[2] = {(uint32_t)lo, (uint32_t)(lo >> 32)};
    const uint32_t m[2] = {mask0, mask1};
    uint32_t id = 0, bad = 0;
#pragma unroll
    for (int i = 0; i < 2; i++) {
        const uint32_t t = ((x[i] >> 1) ^ (x[i] >> 2)) & 0x03030303u;         // A0 C1 G2 T3 (kmer.py:44-49)
        bad |= (x[i] ^ __builtin_amdgcn_perm(0u, 0x54474341u /* "ACGT" */, t)) & m[i];      // the letter of that code, looked up again
        id = (id << 8) | __builtin_amdgcn_udot4(t, 0x01041040u, 0u, false);   // byte0 * 64 + byte1 * 16 + byte2 * 4 + byte3
    }
    *id_out = id >> (16 - 2 * k);
    return bad == 0;
}

// rows of the records in `multi` <- 0 (16 bytes per thread; a row is 4^k >= 4 entries and starts 16-byte aligned)
__global__ void __launch_bounds__(256)
tables_zero_kernel(const uint32_t *__restrict__ multi, uint32_t nmulti, int k, uint32_t *__restrict__ tables)
{
    const uint32_t quads = 1u << (2 * k - 2);
    for (uint32_t m = blockIdx.x; m < nmulti; m += gridDim.x) {
        uint4 *row = reinterpret_cast<uint4 *>(tables + ((uint64_t)multi[m] << (2 * k)));
        for (uint32_t i = threadIdx.x; i < quads; i += blockDim.x) row[i] = make_uint4(0u, 0u, 0u, 0u);
    }
}

// grid: ceil(npieces / 4) workgroups, lds_bytes(k) of dynamic LDS.  piece_rec: the record of every piece, or null where every record is
// one piece (piece p = record p); rec_piece0: nreads + 1 entries, the first piece of every record.  phase: of record 0.
__global__ void __launch_bounds__(TPB)
tables_piece_kernel(const uint8_t *__restrict__ bases, const uint64_t *__restrict__ offs, const uint32_t *__restrict__ piece_rec,
                    const uint32_t *__restrict__ rec_piece0, uint32_t npieces, int k, int stride, int canonical, uint32_t phase,
                    uint32_t *__restrict__ tables, PieceOut *__restrict__ out)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t piece = __builtin_amdgcn_readfirstlane(blockIdx.x * WAVES + wave);
    if (piece >= npieces) return;                                            // (no workgroup barrier anywhere below)
    const uint32_t nbins = 1u << (2 * k);
    uint32_t *tab = lds + wave * nbins;
    for (uint32_t i = lane; i < nbins; i += 64) tab[i] = 0;

    const uint32_t rec = piece_rec ? piece_rec[piece] : piece;
    const uint32_t p0 = rec_piece0[rec], p1 = rec_piece0[rec + 1];
    const uint64_t s = offs[rec], len = offs[rec + 1] - s;
    const uint64_t ph = rec == 0 ? (uint64_t)phase : 0;
    const uint64_t nwin = kdbplan::tables_windows(len, k, stride, ph);
    const uint64_t w0 = (uint64_t)(piece - p0) * PIECE;
    const uint32_t nw = (uint32_t)(nwin > w0 ? (nwin - w0 < (uint64_t)PIECE ? nwin - w0 : (uint64_t)PIECE) : 0);
    const u64 *words = reinterpret_cast<const u64 *>(bases);                  // (the buffer is the call's own allocation: aligned, padded)
    const uint64_t at0 = s + ph + w0 * (uint64_t)stride;                      // the piece's first window starts at this residue
    const uint32_t mask0 = k >= 4 ? 0xFFFFFFFFu : (1u << (8 * k)) - 1u, mask1 = k <= 4 ? 0u : (1u << (8 * (k - 4))) - 1u;

    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");                    // the zeros before the adds
    __builtin_amdgcn_wave_barrier();

    uint32_t counted = 0, skipped = 0, first = NO_FIRST, last = 0;            // first: (j << 2k) | id of the lane's first counted window; last: 1 + that of its last
    for (uint32_t j0 = 0; j0 < nw; j0 += 64 * WINDOWS_IN_FLIGHT) {
        u64 w[WINDOWS_IN_FLIGHT][2];
        uint32_t sh[WINDOWS_IN_FLIGHT];
        bool in[WINDOWS_IN_FLIGHT];
#pragma unroll
        for (int u = 0; u < WINDOWS_IN_FLIGHT; u++) {
            const uint32_t j = j0 + 64u * u + lane;
            const uint64_t at = at0 + (uint64_t)j * (uint64_t)stride;
            in[u] = j < nw;
            sh[u] = ((uint32_t)at & 7u) * 8u;
            w[u][0] = w[u][1] = 0;
            if (in[u]) {
                const u64 *q = words + (at >> 3);
                w[u][0] = q[0]; w[u][1] = q[1];
            }
        }
#pragma unroll
        for (int u = 0; u < WINDOWS_IN_FLIGHT; u++) {
            const uint32_t j = j0 + 64u * u + lane;
            uint32_t id = 0;
            const bool ok = window_id(w[u][0], w[u][1], sh[u], k, mask0, mask1, &id) && in[u];
            if (canonical) {
                const uint32_t r = (uint32_t)kdbstrands::rc_id(id, k);
                id = r < id ? r : id;
            }
            counted += ok ? 1u : 0u;
            skipped += in[u] && !ok ? 1u : 0u;
            if (ok) {
                const uint32_t key = (j << (2 * k)) | id;
                first = first == NO_FIRST ? key : first;
                last = key + 1u;
            }
            const u64 m = __ballot(ok);
            if (m == 0) continue;                                             // (wave-uniform)
            const uint32_t lead = (uint32_t)__builtin_ctzll(m);
            const uint32_t id_lead = (uint32_t)__shfl((int)id, (int)lead);
            if (__ballot(ok && id == id_lead) == m) {                         // one id in the whole round: one add of their number
                if (lane == lead) __hip_atomic_fetch_add(&tab[id], (uint32_t)__builtin_popcountll(m), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            } else if (ok) {
                __hip_atomic_fetch_add(&tab[id], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            }
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        counted += __shfl_down(counted, off);
        skipped += __shfl_down(skipped, off);
        const uint32_t f2 = __shfl_down(first, off), l2 = __shfl_down(last, off);
        first = f2 < first ? f2 : first;
        last = l2 > last ? l2 : last;
    }
    if (lane == 0) {
        PieceOut o;
        o.counted = counted; o.skipped = skipped;
        o.first_id = first == NO_FIRST ? -1 : (int32_t)(first & (nbins - 1u));
        o.last_id = last == 0 ? -1 : (int32_t)((last - 1u) & (nbins - 1u));
        out[piece] = o;
    }

    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");                    // the adds before the row is read
    __builtin_amdgcn_wave_barrier();

    uint32_t *row = tables + ((uint64_t)rec << (2 * k));
    if (p1 - p0 == 1) {
        const uint4 *t4 = reinterpret_cast<const uint4 *>(tab);
        uint4 *r4 = reinterpret_cast<uint4 *>(row);
        for (uint32_t i = lane; i < nbins / 4; i += 64) r4[i] = t4[i];
    } else {
        for (uint32_t i = lane; i < nbins; i += 64) {
            const uint32_t v = tab[i];
            if (v) __hip_atomic_fetch_add(&row[i], v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

// one thread per record: its pieces in order
__global__ void __launch_bounds__(256)
tables_record_kernel(const PieceOut *__restrict__ pieces, const uint32_t *__restrict__ rec_piece0, uint64_t nreads, u64 *__restrict__ windows_out,
                     u64 *__restrict__ skipped_out, int32_t *__restrict__ first_out, int32_t *__restrict__ last_out)
{
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= nreads) return;
    u64 windows = 0, skipped = 0;
    int32_t first = -1, last = -1;
    for (uint32_t p = rec_piece0[r]; p < rec_piece0[r + 1]; p++) {
        const PieceOut o = pieces[p];
        windows += o.counted;
        skipped += o.skipped;
        if (first < 0) first = o.first_id;
        if (o.last_id >= 0) last = o.last_id;
    }
    windows_out[r] = windows;
    skipped_out[r] = skipped;
    first_out[r] = first;
    last_out[r] = last;
}

}  // namespace kdbtables
