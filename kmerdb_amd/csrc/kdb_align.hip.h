// kdb_align.hip.h -- a batch of banded local alignments with affine gaps (kdb_align_banded of include/kdbhip.h):
// per task the best score and where that alignment begins and ends in the oriented query and in the reference record.  The traceback
// (kdb_align_traceback) is kdb_align_trace.hip.h: its forward pass is this one, with the direction stores switched on.
//
// One wave owns one task from its first row to its last; the waves stride through the tasks.  With jb = d - band a cell (i, j) lies on the
// band's diagonal c = j - i - jb, 0 <= c <= 2 band <= 126, and lane l owns the diagonals 2l and 2l + 1.  The wave sweeps anti-diagonals:
// step T has an EVEN half, in which lane l computes the cell (T - l, c = 2l), and an ODD half for (T - l, c = 2l + 1).  What a cell needs:
//   the diagonal term   H(i - 1, c)                    the lane's own register, two halves back
//   E, from the left    H, E(i, c - 1)                 even half: lane l - 1's odd cell of step T - 1;  odd half: the own even cell of step T
//   F, from above       H, F(i - 1, c + 1)             even half: the own odd cell of step T - 1;       odd half: lane l + 1's even cell of step T
// so no cell waits for a lane in the same half, and every half every lane of the band works.  A cell leaves behind what its right and its
// lower neighbour will take from it, Ec = max(H + gap_open, E + gap_extend) and Fc likewise, each with its origin: one value and one origin
// cross a lane boundary per half (__shfl_up in the even half, __shfl_down in the odd one).  H, Ec, Fc and their origins stay in registers
// for the whole task.  An origin is packed as (i0 << 7) | c0 -- 20 + 7 bits: its column is i0 + c0 + jb.
//
// What is not a cell: a row below 0 or a column below 0 is staged as a residue code that matches nothing, and the recurrence then gives
// H = 0 and E, F <= 0 there by itself (mismatch, gap_open, gap_extend <= 0), which no positive score can come from -- and only positive
// scores and their origins are ever reported.  Rows from m and columns from n on have no successor inside the record; they are only kept
// from becoming the best cell.  A diagonal outside the band (c > 2 band) is forced to H = 0, Ec = Fc = -infinity in every half.
//
// Within a lane the halves visit the lane's cells by ascending (i, j), so a lane keeps its best cell with a plain `>`; the wave's best is
// one max-reduction of (score, -i, -c) packed into 64 bits, which is the tie rule of the definition stated outright.
//
// LDS: per wave, and per stage of STAGE steps, the oriented query rows and the reference residues the stage's cells read
// (kdbplan::align_lds_wave: 2 STAGE + 208 bytes, 1232 at STAGE = 512), as one code per byte: A 0, C 1, G 2, T 3, and 4 (query) or 5
// (reference) for an N and for everything outside the record -- two codes that equal nothing, so s(i, j) is one compare.  The residues are
// read from global memory as aligned 4-byte words (strand 1: turned round and complemented on the way) and read from LDS as the two aligned
// words around the 4 rows a lane takes next: 4 LDS reads per 8 cells and lane.
// No scalar memory writes, no atomics, no spinning, no workgroup barrier.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/kdbhip.h"
#include "kdb_sweep_plan.cpp.h"

namespace kdbalign {

typedef unsigned long long u64;

constexpr int TPB = 256;
constexpr uint32_t WAVES = TPB / 64;                       // tasks under way per workgroup
constexpr uint32_t STAGE = KDB_ALIGN_STAGE;
constexpr uint32_t GRID_MAX = KDB_ALIGN_GRID_MAX;
constexpr int MAX_BAND = KDB_ALIGN_MAX_BAND;
constexpr uint64_t MAX_QUERY = KDB_ALIGN_MAX_QUERY;
constexpr int NEG = -(1 << 29);                             // -infinity: a score stays below 2^27
constexpr uint32_t Q_NONE = 4, R_NONE = 5;
static_assert(2 * MAX_BAND + 1 < 2 * (int)kdbplan::ALIGN_LANES, "a lane owns two diagonals of the band");
static_assert(STAGE % 8 == 0 && STAGE >= kdbplan::ALIGN_GROUP, "a stage is whole groups of steps, its LDS whole words");
static_assert(MAX_QUERY <= (1u << 20), "an origin packs its row into 20 bits, and 127 x 2^20 < 2^27");
static_assert((size_t)WAVES * kdbplan::align_lds_wave(STAGE) <= 64u * 1024u, "a workgroup's LDS stays below 64 KiB");

// the bytes g .. g + 3 of a buffer of nwords aligned words (g may lie outside it: those bytes read as 0)
__device__ __forceinline__ uint32_t bytes4(const uint32_t *__restrict__ words, int64_t nwords, int64_t g)
{
    const int64_t a = g >> 2;
    const uint32_t w0 = a >= 0 && a < nwords ? words[a] : 0u;
    const uint32_t w1 = a + 1 >= 0 && a + 1 < nwords ? words[a + 1] : 0u;
    return __builtin_amdgcn_alignbyte(w1, w0, (uint32_t)g & 3u);
}

// four residues (ACGTN, checked on the host) -> four codes, an N -> none; comp: the complement's codes
__device__ __forceinline__ uint32_t codes4(uint32_t w, bool comp, uint32_t none)
{
    const uint32_t is_n = (w >> 3) & 0x01010101u;                             // (bit 3 is set in 'N' alone)
    uint32_t t = ((w >> 1) ^ (w >> 2)) & 0x03030303u;                         // A 0 C 1 G 2 T 3, N 0
    if (comp) t ^= 0x03030303u;
    return (t & ~(is_n * 0xFFu)) | is_n * none;
}

// the codes of the positions p .. p + 3 of a record of len residues; a position outside it -> none
__device__ __forceinline__ uint32_t inside4(uint32_t codes, int64_t p, int64_t len, uint32_t none)
{
    uint32_t out = 0;
#pragma unroll
    for (int b = 0; b < 4; b++) out |= (p + b >= 0 && p + b < len ? (codes >> (8 * b)) & 0xFFu : none) << (8 * b);
    return out;
}

// One cell.  In: H, oH = H(i - 1, c) and its origin; (e, oe) and (f, of) = E(i, c) and F(i, c) as the neighbours left them; s = s(i, j);
// here = this cell as an origin.  Out: H, oH = H(i, c); (Ec, oEc), (Fc, oFc) = what the right and the lower neighbour take.
// The origin of a value that is not positive is never used and may be anything.  dir: the cell's four direction bits for the traceback
// (kdb_align_trace.hip.h) -- bits 0-1 where H comes from (DIR_START: the diagonal from H = 0, DIR_DIAG, DIR_E, DIR_F), DIR_E_OPENS and
// DIR_F_OPENS where the Ec and the Fc it hands on take the H + gap_open term; a caller that does not keep them pays nothing for them.
constexpr uint32_t DIR_START = 0, DIR_DIAG = 1, DIR_E = 2, DIR_F = 3, DIR_E_OPENS = 4, DIR_F_OPENS = 8;
__device__ __forceinline__ void cell(int &H, uint32_t &oH, int e, uint32_t oe, int f, uint32_t of, int s, uint32_t here, int gap_open, int gap_extend, bool in_band,
                                     int &Ec, uint32_t &oEc, int &Fc, uint32_t &oFc, uint32_t &dir)
{
    const uint32_t od = H == 0 ? here : oH;                                   // a diagonal step from H = 0, or from nothing, starts here
    const int dg = H + s;
    const int h = max(max(dg, e), max(f, 0));
    const uint32_t o = dg == h ? od : (e == h ? oe : of);                      // the first of [diagonal, E, F] that reaches h
    const int ho = h + gap_open, ee = e + gap_extend, ff = f + gap_extend;
    dir = (dg == h ? (H == 0 ? DIR_START : DIR_DIAG) : (e == h ? DIR_E : DIR_F)) | (ho >= ee ? DIR_E_OPENS : 0u) | (ho >= ff ? DIR_F_OPENS : 0u);
    H = in_band ? h : 0;
    oH = o;
    Ec = in_band ? max(ho, ee) : NEG;
    oEc = ho >= ee ? o : oe;                                                  // on a tie the H + gap_open term wins
    Fc = in_band ? max(ho, ff) : NEG;
    oFc = ho >= ff ? o : of;
}

// The forward pass of the tasks [task_lo, task_hi), the waves striding through them.  q_words / r_words: the two residue buffers as aligned
// words (the call's own allocations), q_nwords / r_nwords of them.  TRACE: every lane also stores the direction bits of its eight cells
// of a group as one dword -- nibble 2 r + (c & 1) for the group's row r -- at kdbplan::align_trace_dword(group, lane) of the task's bytes,
// which begin dir_offs[task] bytes into dirs (kdbplan::align_trace_chunks).
template <bool TRACE>
__device__ __forceinline__ void
align_tasks(const uint32_t *__restrict__ q_words, int64_t q_nwords, const uint64_t *__restrict__ q_offs, const uint32_t *__restrict__ r_words, int64_t r_nwords,
            const uint64_t *__restrict__ r_offs, const uint32_t *__restrict__ task_q, const uint32_t *__restrict__ task_r, const int64_t *__restrict__ task_diag,
            const uint8_t *__restrict__ task_strand, uint32_t task_lo, uint32_t task_hi, int band, int match, int mismatch, int gap_open, int gap_extend,
            int32_t *__restrict__ score_out, uint32_t *__restrict__ qstart_out, uint32_t *__restrict__ qend_out, uint32_t *__restrict__ rstart_out,
            uint32_t *__restrict__ rend_out, uint32_t *__restrict__ dirs, const uint64_t *__restrict__ dir_offs)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    const int lane = (int)(threadIdx.x & 63u);
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    constexpr uint32_t LDS_Q = kdbplan::align_lds_q(STAGE), LDS_R = kdbplan::align_lds_r(STAGE), BACK = kdbplan::ALIGN_LANES;
    uint32_t *const q_lds = reinterpret_cast<uint32_t *>(lds + (size_t)wave * kdbplan::align_lds_wave(STAGE));
    uint32_t *const r_lds = q_lds + LDS_Q / 4;
    const bool even_in = 2 * lane <= 2 * band, odd_in = 2 * lane + 1 <= 2 * band;

    for (uint32_t task = __builtin_amdgcn_readfirstlane(task_lo + blockIdx.x * WAVES + wave); task < task_hi; task += gridDim.x * WAVES) {   // (wave-uniform)
        const uint32_t tq = task_q[task], tr = task_r[task];
        const bool minus = task_strand[task] != 0;
        const int64_t q0 = (int64_t)q_offs[tq], r0 = (int64_t)r_offs[tr];
        const int64_t m = (int64_t)q_offs[tq + 1] - q0, n = (int64_t)r_offs[tr + 1] - r0;
        const kdbplan::AlignWindow win = kdbplan::align_window((uint64_t)m, (uint64_t)n, task_diag[task], (uint32_t)band);
        if (win.empty()) {                                                    // (wave-uniform)
            if (lane == 0) { score_out[task] = 0; qstart_out[task] = 0; qend_out[task] = 0; rstart_out[task] = 0; rend_out[task] = 0; }
            continue;
        }
        const int jb = win.jb;
        const int t_lo = (int)kdbplan::align_t_lo(win), t_hi = (int)kdbplan::align_t_hi(win, (uint32_t)band);
        // a cell (i, c) of this lane may be the best one iff it lies in the record and in the band: i < lim
        const int64_t right_even = n - jb - 2 * lane, right_odd = right_even - 1;
        const int lim_even = even_in ? (int)(m < right_even ? m : right_even) : 0, lim_odd = odd_in ? (int)(m < right_odd ? m : right_odd) : 0;

        int He = 0, Ho = 0, EcE = NEG, FcE = NEG, EcO = NEG, FcO = NEG;
        uint32_t oHe = 0, oHo = 0, oEcE = 0, oFcE = 0, oEcO = 0, oFcO = 0;
        int best = 0;
        uint32_t best_at = 0, best_from = 0;
        uint32_t *const task_dirs = TRACE ? dirs + dir_offs[task] / 4 : nullptr;

        for (int ts = t_lo; ts < t_hi; ts += (int)STAGE) {
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");            // the last stage's reads before this one's writes
            __builtin_amdgcn_wave_barrier();
            // rows [ts - BACK, ts - BACK + LDS_Q) of the oriented query, as whole words
            for (uint32_t w = (uint32_t)lane; w < LDS_Q / 4; w += 64) {
                const int64_t i = (int64_t)ts - BACK + 4 * (int64_t)w;
                uint32_t v;
                if (!minus) v = bytes4(q_words, q_nwords, q0 + i);
                else v = __builtin_bswap32(bytes4(q_words, q_nwords, q0 + m - 4 - i));         // rows i .. i + 3 are the residues m - 1 - i down to m - 4 - i
                q_lds[w] = inside4(codes4(v, minus, Q_NONE), i, m, Q_NONE);
            }
            // the reference residues [ts - BACK + jb, + LDS_R)
            for (uint32_t w = (uint32_t)lane; w < LDS_R / 4; w += 64) {
                const int64_t j = (int64_t)ts - BACK + jb + 4 * (int64_t)w;
                r_lds[w] = inside4(codes4(bytes4(r_words, r_nwords, r0 + j), false, R_NONE), j, n, R_NONE);
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");            // the stage before the lanes read each other's words
            __builtin_amdgcn_wave_barrier();

            const int t_end = min(ts + (int)STAGE, t_hi);
            for (int t0 = ts; t0 < t_end; t0 += (int)kdbplan::ALIGN_GROUP) {
                // the lane's rows t0 - lane .. + 3 and the columns of its two diagonals there: LDS bytes x .. x + 3 and y .. y + 4
                const uint32_t x = (uint32_t)(t0 - ts) + BACK - (uint32_t)lane, y = x + 2u * (uint32_t)lane;
                const uint32_t qw = __builtin_amdgcn_alignbyte(q_lds[x / 4 + 1], q_lds[x / 4], x & 3u);
                const u64 rw = (((u64)r_lds[y / 4 + 1] << 32) | r_lds[y / 4]) >> (8u * (y & 3u));
                uint32_t group_dirs = 0, dir;
#pragma unroll
                for (int r = 0; r < (int)kdbplan::ALIGN_GROUP; r++) {
                    const int i = t0 + r - lane;
                    const uint32_t q = (qw >> (8 * r)) & 0xFFu, re = (uint32_t)(rw >> (8 * r)) & 0xFFu, ro = (uint32_t)(rw >> (8 * r + 8)) & 0xFFu;
                    const uint32_t here = ((uint32_t)i << 7) | (uint32_t)(2 * lane);
                    // even half: E from lane - 1's odd cell, F from the own odd cell
                    int e = __shfl_up(EcO, 1);
                    const uint32_t oe = __shfl_up(oEcO, 1);
                    if (lane == 0) e = NEG;                                   // (the diagonal c = -1 is outside the band)
                    cell(He, oHe, e, oe, FcO, oFcO, q == re ? match : mismatch, here, gap_open, gap_extend, even_in, EcE, oEcE, FcE, oFcE, dir);
                    if (TRACE) group_dirs |= dir << (8 * r);
                    if (He > best && i < lim_even) { best = He; best_at = here; best_from = oHe; }
                    // odd half: E from the own even cell, F from lane + 1's even cell (lane 63's odd diagonal is never in the band)
                    const int f = __shfl_down(FcE, 1);
                    const uint32_t of = __shfl_down(oFcE, 1);
                    cell(Ho, oHo, EcE, oEcE, f, of, q == ro ? match : mismatch, here | 1u, gap_open, gap_extend, odd_in, EcO, oEcO, FcO, oFcO, dir);
                    if (TRACE) group_dirs |= dir << (8 * r + 4);
                    if (Ho > best && i < lim_odd) { best = Ho; best_at = here | 1u; best_from = oHo; }
                }
                if (TRACE) task_dirs[kdbplan::align_trace_dword((uint32_t)(t0 - t_lo) / kdbplan::ALIGN_GROUP, (uint32_t)lane)] = group_dirs;   // (256 bytes per wave)
            }
        }

        // the wave's best cell: the largest score, then the smallest i, then the smallest j (the smallest c of that row)
        const u64 key = ((u64)(uint32_t)best << 27) | (u64)(0x7FFFFFFu - best_at);
        u64 top = key;
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            const u64 other = __shfl_xor(top, off);
            top = other > top ? other : top;
        }
        const u64 winners = __ballot(key == top);                             // (one lane: a cell has one owner -- or all of them, at score 0)
        const int src = __builtin_ctzll(winners);
        const uint32_t at = (uint32_t)__shfl((int)best_at, src), from = (uint32_t)__shfl((int)best_from, src);
        const int score = __shfl(best, src);
        if (lane == 0) {
            const bool found = score > 0;
            const int i = (int)(at >> 7), c = (int)(at & 127u), i0 = (int)(from >> 7), c0 = (int)(from & 127u);
            score_out[task] = found ? score : 0;
            qstart_out[task] = found ? (uint32_t)i0 : 0u;
            qend_out[task] = found ? (uint32_t)(i + 1) : 0u;
            rstart_out[task] = found ? (uint32_t)(i0 + c0 + jb) : 0u;
            rend_out[task] = found ? (uint32_t)(i + c + jb + 1) : 0u;
        }
    }
}

// grid: at most GRID_MAX workgroups of WAVES waves, WAVES * align_lds_wave(STAGE) bytes of dynamic LDS.  kdb_align_banded: no direction stores.
__global__ void __launch_bounds__(TPB)
align_kernel(const uint32_t *__restrict__ q_words, int64_t q_nwords, const uint64_t *__restrict__ q_offs, const uint32_t *__restrict__ r_words, int64_t r_nwords,
             const uint64_t *__restrict__ r_offs, const uint32_t *__restrict__ task_q, const uint32_t *__restrict__ task_r, const int64_t *__restrict__ task_diag,
             const uint8_t *__restrict__ task_strand, uint32_t ntasks, int band, int match, int mismatch, int gap_open, int gap_extend,
             int32_t *__restrict__ score_out, uint32_t *__restrict__ qstart_out, uint32_t *__restrict__ qend_out, uint32_t *__restrict__ rstart_out,
             uint32_t *__restrict__ rend_out)
{
    align_tasks<false>(q_words, q_nwords, q_offs, r_words, r_nwords, r_offs, task_q, task_r, task_diag, task_strand, 0u, ntasks, band, match, mismatch, gap_open, gap_extend,
                       score_out, qstart_out, qend_out, rstart_out, rend_out, nullptr, nullptr);
}

}  // namespace kdbalign
