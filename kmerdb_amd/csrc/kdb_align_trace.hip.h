// kdb_align_trace.hip.h -- the traceback of kdb_align_banded's alignments (kdb_align_traceback of include/kdbhip.h):
// per task the run-length encoded path from the origin to the best cell, one uint32 (len << 4) | op per run, BAM's op codes.
//
// Per chunk of tasks (kdbplan::align_trace_chunks) four steps, each its own launch on one stream:
//   trace_forward_kernel   kdb_align.hip.h's forward pass with the direction stores on: 4 bits per cell, one dword per lane and group
//   walk_kernel<false>     a wave per task walks the stored directions from the best cell to the origin and counts the runs
//   scan_*_kernel          the exclusive prefix sums of the counts, on top of the carry the chunks before left (64 bits)
//   walk_kernel<true>      the same walk again, which now writes run k of the n it meets (it meets them last to first) to place n - 1 - k
// VISIBILITY: the walk reads dwords that other lanes of the forward pass stored.  It is a second launch on the same stream, so the
// stores are complete and visible when it begins -- no fence inside a kernel, and the forward kernel keeps its registers for the
// recurrence alone.  The price is that the count walk reads the directions from memory, not from the cache the forward pass left warm.
//
// THE WALK is wave-uniform: the state -- row i, band diagonal c, which of H, E, F -- is the same in every lane (scalar registers).  With
// lane l = c / 2 and step T = i + l every move lowers T by 0 or 1, so the groups are visited in descending order and each is loaded once:
// one coalesced 256-byte read, a dword per lane, and beside it every lane works out which of its eight cells of the group hold equal
// residues (the `=` or X of a diagonal move) from the aligned words around its rows and columns.  The nibble and the equal-bit of the
// cell the walk stands on are then lane reads at a uniform index; no lane chases a chain of dependent loads cell by cell.
// State H at (i, c) reads the nibble of (i, c); state E at (i, c) reads the E-opens bit of (i, c - 1), the cell that handed the E on;
// state F at (i, c) the F-opens bit of (i - 1, c + 1).  A cell the definition's walk can never ask for (outside the band or the task's
// steps) ends the walk: no address outside the task's bytes is ever formed.
// No scalar memory writes, no atomics, no spinning, no workgroup barrier in the forward pass and the walks (the scan uses __syncthreads).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kdb_align.hip.h"

namespace kdbalign {

constexpr uint32_t OP_I = 1, OP_D = 2, OP_EQ = 7, OP_X = 8;                  // BAM's op codes
constexpr int SCAN_TPB = 256, SCAN_ITEMS = 8;
constexpr uint32_t SCAN_BLOCK = SCAN_TPB * SCAN_ITEMS;

// grid, block and LDS as align_kernel
__global__ void __launch_bounds__(TPB)
trace_forward_kernel(const uint32_t *__restrict__ q_words, int64_t q_nwords, const uint64_t *__restrict__ q_offs, const uint32_t *__restrict__ r_words, int64_t r_nwords,
                     const uint64_t *__restrict__ r_offs, const uint32_t *__restrict__ task_q, const uint32_t *__restrict__ task_r, const int64_t *__restrict__ task_diag,
                     const uint8_t *__restrict__ task_strand, uint32_t task_lo, uint32_t task_hi, int band, int match, int mismatch, int gap_open, int gap_extend,
                     int32_t *__restrict__ score_out, uint32_t *__restrict__ qstart_out, uint32_t *__restrict__ qend_out, uint32_t *__restrict__ rstart_out,
                     uint32_t *__restrict__ rend_out, uint32_t *__restrict__ dirs, const uint64_t *__restrict__ dir_offs)
{
    align_tasks<true>(q_words, q_nwords, q_offs, r_words, r_nwords, r_offs, task_q, task_r, task_diag, task_strand, task_lo, task_hi, band, match, mismatch, gap_open,
                      gap_extend, score_out, qstart_out, qend_out, rstart_out, rend_out, dirs, dir_offs);
}

// grid: workgroups of WAVES waves that stride through the tasks [task_lo, task_hi); no LDS.  score, qend, rend: the forward pass's.
// WRITE false: nruns[task] <- the number of runs.  WRITE true: the runs go to runs[run_offs[task] .. + nruns[task]) where that lies
// inside the cap entries of runs.
template <bool WRITE>
__global__ void __launch_bounds__(TPB)
walk_kernel(const uint32_t *__restrict__ q_words, int64_t q_nwords, const uint64_t *__restrict__ q_offs, const uint32_t *__restrict__ r_words, int64_t r_nwords,
            const uint64_t *__restrict__ r_offs, const uint32_t *__restrict__ task_q, const uint32_t *__restrict__ task_r, const int64_t *__restrict__ task_diag,
            const uint8_t *__restrict__ task_strand, uint32_t task_lo, uint32_t task_hi, int band, const int32_t *__restrict__ score, const uint32_t *__restrict__ qend,
            const uint32_t *__restrict__ rend, const uint32_t *__restrict__ dirs, const uint64_t *__restrict__ dir_offs, uint32_t *__restrict__ nruns,
            const u64 *__restrict__ run_offs, uint32_t *__restrict__ runs, u64 cap)
{
    const int lane = (int)(threadIdx.x & 63u);
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    for (uint32_t task = __builtin_amdgcn_readfirstlane(task_lo + blockIdx.x * WAVES + wave); task < task_hi; task += gridDim.x * WAVES) {   // (wave-uniform)
        uint32_t want = 0;
        u64 at = 0;
        if (WRITE) {
            want = nruns[task];
            at = run_offs[task];
            if (want == 0 || at + want > cap) continue;
        }
        if (score[task] <= 0) {
            if (!WRITE && lane == 0) nruns[task] = 0;
            continue;
        }
        const uint32_t tq = task_q[task], tr = task_r[task];
        const bool minus = task_strand[task] != 0;
        const int64_t q0 = (int64_t)q_offs[tq], r0 = (int64_t)r_offs[tr];
        const int64_t m = (int64_t)q_offs[tq + 1] - q0, n = (int64_t)r_offs[tr + 1] - r0;
        const kdbplan::AlignWindow win = kdbplan::align_window((uint64_t)m, (uint64_t)n, task_diag[task], (uint32_t)band);
        const int jb = win.jb, t_lo = (int)kdbplan::align_t_lo(win);
        const int ngroups = (int)kdbplan::align_trace_groups(win, (uint32_t)band);
        const uint32_t *const task_dirs = dirs + dir_offs[task] / 4;

        // the best cell, in state H
        int i = (int)qend[task] - 1, c = (int)((int64_t)rend[task] - 1 - i - jb), state = 0;
        int loaded = -1;
        uint32_t d = 0, eq = 0;                                               // the lane's dword of the loaded group, and its cells' equal-bits
        uint32_t op = 0, len = 0, k = 0;                                      // the run under way; the runs behind it
        bool done = false;
        while (!done) {
            // the cell whose nibble this move asks for
            const int ri = state == 2 ? i - 1 : i, rc = state == 0 ? c : (state == 1 ? c - 1 : c + 1);
            const int T = ri + (rc >> 1), g = (T - t_lo) >> 2;
            if (rc < 0 || rc > 2 * band || T < t_lo || g >= ngroups) break;   // (no path of the definition: see above)
            if (g != loaded) {
                loaded = g;
                d = task_dirs[kdbplan::align_trace_dword((uint32_t)g, (uint32_t)lane)];
                // the lane's rows x .. x + 3 and the columns y .. y + 4 of its two diagonals there, as align_tasks stages them
                const int64_t x = (int64_t)t_lo + 4 * g - lane, y = x + 2 * lane + jb;
                uint32_t v;
                if (!minus) v = bytes4(q_words, q_nwords, q0 + x);
                else v = __builtin_bswap32(bytes4(q_words, q_nwords, q0 + m - 4 - x));
                const uint32_t qw = inside4(codes4(v, minus, Q_NONE), x, m, Q_NONE);
                const uint32_t r_lo = inside4(codes4(bytes4(r_words, r_nwords, r0 + y), false, R_NONE), y, n, R_NONE);
                const uint32_t r_hi = inside4(codes4(bytes4(r_words, r_nwords, r0 + y + 4), false, R_NONE), y + 4, n, R_NONE);
                const u64 rw = ((u64)r_hi << 32) | r_lo;
                eq = 0;
#pragma unroll
                for (int r = 0; r < (int)kdbplan::ALIGN_GROUP; r++) {
                    const uint32_t q = (qw >> (8 * r)) & 0xFFu, re = (uint32_t)(rw >> (8 * r)) & 0xFFu, ro = (uint32_t)(rw >> (8 * r + 8)) & 0xFFu;
                    eq |= (q == re ? 1u : 0u) << (2 * r) | (q == ro ? 1u : 0u) << (2 * r + 1);
                }
            }
            const int cell_at = 2 * ((T - t_lo) & 3) + (rc & 1);
            const uint32_t nib = ((uint32_t)__builtin_amdgcn_readlane((int)d, rc >> 1) >> (4 * cell_at)) & 15u;
            uint32_t emit = 0;
            if (state == 0) {
                const uint32_t from = nib & 3u;
                if (from == DIR_E) state = 1;
                else if (from == DIR_F) state = 2;
                else {
                    emit = ((uint32_t)__builtin_amdgcn_readlane((int)eq, rc >> 1) >> cell_at) & 1u ? OP_EQ : OP_X;
                    if (from == DIR_START) done = true;
                    else i -= 1;
                }
            } else if (state == 1) {
                emit = OP_D;
                c -= 1;
                state = nib & DIR_E_OPENS ? 0 : 1;
            } else {
                emit = OP_I;
                i -= 1;
                c += 1;
                state = nib & DIR_F_OPENS ? 0 : 2;
            }
            if (emit != 0 && emit != op) {
                if (len) {
                    if (WRITE && lane == 0 && k < want) runs[at + want - 1 - k] = (len << 4) | op;
                    k++;
                }
                op = emit;
                len = 0;
            }
            if (emit != 0) len++;
        }
        if (len) {
            if (WRITE && lane == 0 && k < want) runs[at + want - 1 - k] = (len << 4) | op;
            k++;
        }
        if (!WRITE && lane == 0) nruns[task] = k;
    }
}

// ---- the exclusive prefix sums of the chunk's counts, 64 bits, on top of *carry: three launches, no workgroup waits for another ----

// the exclusive prefix sum of v over the workgroup's SCAN_TPB threads and, in *total, the sum; every thread of the workgroup calls it
__device__ __forceinline__ u64 block_exclusive(u64 v, u64 *wave_sums, u64 *total)
{
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    u64 inc = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const u64 t = __shfl_up(inc, off);
        if (lane >= (uint32_t)off) inc += t;
    }
    if (lane == 63) wave_sums[wave] = inc;
    __syncthreads();
    u64 base = 0, tot = 0;
#pragma unroll
    for (uint32_t w = 0; w < SCAN_TPB / 64; w++) {
        const u64 x = wave_sums[w];
        base += w < wave ? x : 0u;
        tot += x;
    }
    __syncthreads();                                                          // (wave_sums may be written again)
    *total = tot;
    return base + inc - v;
}

// sums[b] = the sum of counts[b SCAN_BLOCK .. (b + 1) SCAN_BLOCK); grid: one workgroup per block
__global__ void __launch_bounds__(SCAN_TPB)
scan_sums_kernel(const uint32_t *__restrict__ counts, uint32_t n, u64 *__restrict__ sums)
{
    __shared__ u64 wave_sums[SCAN_TPB / 64];
    const uint64_t at = (uint64_t)blockIdx.x * SCAN_BLOCK + threadIdx.x * SCAN_ITEMS;
    u64 v = 0;
#pragma unroll
    for (int j = 0; j < SCAN_ITEMS; j++) v += at + j < n ? counts[at + j] : 0u;
    u64 total;
    (void)block_exclusive(v, wave_sums, &total);
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

// one workgroup: sums[0 .. nblocks) <- *carry + their exclusive prefix sums, *carry <- *carry + the sum of all
__global__ void __launch_bounds__(SCAN_TPB)
scan_top_kernel(u64 *__restrict__ sums, uint32_t nblocks, u64 *carry)
{
    __shared__ u64 wave_sums[SCAN_TPB / 64];
    u64 run = *carry;                                                         // (read by every thread before the barriers thread 0's write lies behind)
    for (uint32_t i0 = 0; i0 < nblocks; i0 += SCAN_TPB) {                     // (the same trips for every thread)
        const uint32_t i = i0 + threadIdx.x;
        const u64 v = i < nblocks ? sums[i] : 0u;
        u64 total;
        const u64 ex = block_exclusive(v, wave_sums, &total);
        if (i < nblocks) sums[i] = run + ex;
        run += total;
    }
    if (threadIdx.x == 0) *carry = run;
}

// offs[i] = the sum of counts[0 .. i) on top of the block's own sum, counts_out[i] = counts[i] in 64 bits; i < n
__global__ void __launch_bounds__(SCAN_TPB)
scan_apply_kernel(const uint32_t *__restrict__ counts, uint32_t n, const u64 *__restrict__ sums, u64 *__restrict__ offs, u64 *__restrict__ counts_out)
{
    __shared__ u64 wave_sums[SCAN_TPB / 64];
    const uint64_t at = (uint64_t)blockIdx.x * SCAN_BLOCK + threadIdx.x * SCAN_ITEMS;
    uint32_t c[SCAN_ITEMS];
    u64 v = 0;
#pragma unroll
    for (int j = 0; j < SCAN_ITEMS; j++) { c[j] = at + j < n ? counts[at + j] : 0u; v += c[j]; }
    u64 total;
    u64 run = block_exclusive(v, wave_sums, &total) + sums[blockIdx.x];
#pragma unroll
    for (int j = 0; j < SCAN_ITEMS; j++) {
        if (at + j < n) { offs[at + j] = run; counts_out[at + j] = c[j]; }
        run += c[j];
    }
}

}  // namespace kdbalign
