// kdb_pairstats.hip.h -- what the distances that are NOT moments are functions of, in one pairwise sweep of the bins.
//   kdb_pairstats, exact integers:   per vector  S[i] = Sum_b x_i[b] (128 bits),  nnz[i] = #{b : x_i[b] > 0}
//                                    per pair    L1 = Sum_b |x - y| (128 bits),  Linf = max_b |x - y|,  ne = #{b : x != y},  both = #{b : x > 0 and y > 0}
//   kdb_pairfloat, float64:          per pair    C = Sum_b |x - y| / (x + y) over bins with x + y > 0                       (canberra)
//                                                D = Sum_b [ p ln(p/m) + q ln(q/m) ],  p = x/S[i], q = y/S[j], m = (p + q)/2  (jensenshannon^2 * 2)
// cityblock, chebyshev, braycurtis, hamming and the presence/absence family come from the integers on the host (kmerdb_amd/distance.py).
//
// Overflow of the integer sweep.  |x - y| <= max(x, y) <= x + y, so L1 <= S[i] + S[j] < 2^65 once both sums are below 2^64 -- one word is
// not enough, two are.  The host refuses (KDB_ERR_ARG) a vector whose exact S reaches 2^64, as kdb_gram does; S itself is a sum of at most
// 2^36 terms below 2^64 and fits 128 bits always.  A lane meets at most LANE_BINS_MAX = 2^30 bins (nbins <= 2^36, 128 bins per chunk, two
// bins per lane and chunk, even if one wave swept it all), so its counters ne, both, nnz fit 32 bits and its sums a 64-bit word with a 32-bit
// carry count: 7 dwords per pair and lane, 4 per vector.  Waves, workgroups and the combine add in 64 / 128 bits.
//
// Shape of the integer sweep, after kdb_gram's.  Vectors in blocks of B = 4.  A row (blockIdx.y) is a set A of NA vectors against a set Bs of
// NB: on the diagonal A = Bs = one block (its NA (NA - 1) / 2 pairs, and the block's S and nnz); off it a full block against HALF = 2 (or 1)
// vectors of a later block -- 8 pairs x 7 dwords = 56 VGPRs of accumulators beside 24 of loaded bins.  A wave steps through chunks of 128
// bins, a 16-byte load per lane and vector from a scalar base.  |x - y| is formed as x > y ? x - y : y - x per lane: neither order wraps.
// Waves reduce with shuffles (sums with carries, Linf with max), workgroups through LDS, each workgroup writes one partial record per row;
// pair_tail_kernel (one wave per row, plain code) takes the last nbins % 128 bins as one more partial; pair_combine_kernel folds a row's
// partials.  Integer adds and max only, no atomics, no floating point: the same integers for any grid and from run to run.
//
// The float sweep (pairfloat_kernel) takes one pair per row: two divisions and two logarithms in float64 per bin bound it, not the loads.
// A wave whose 128 bins are zero in both vectors adds nothing and skips the arithmetic (wave-uniform).  Each lane forms the per-bin term --
// non-negative, by the log-sum inequality -- and adds it to its own sum; lanes, waves, workgroups and the tail are then added in one fixed
// order, and the grid depends on nbins alone: bit-identical from run to run on one build.  No atomics.  Built without fast-math: the
// division is IEEE's.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/kdbhip.h"

namespace kdbpair {

constexpr int B = KDB_PAIRSTATS_BLOCK;             // vectors per block
constexpr int HALF = KDB_PAIRSTATS_HALF;           // off the diagonal: vectors of the second block per row
constexpr int TPB = 256;                           // four waves
constexpr int CHUNK_BINS = 128;                    // a wave's step: 64 lanes x 16 bytes
constexpr int WG_BINS = (TPB / 64) * CHUNK_BINS;   // bins one workgroup covers per grid stride
constexpr int NPAIR = B * B;                       // a row's pair slots: (i of A, j of Bs) in slot i * B + j
constexpr int PAIR_WORDS = 5, VEC_WORDS = 3;       // a pair's record: L1 lo, L1 hi, Linf, ne, both; a vector's: S lo, S hi, nnz
constexpr int NSLOT = NPAIR + B;                   // pair slots, then the vectors of A (diagonal rows)
constexpr int ROW_WORDS = NPAIR * PAIR_WORDS + B * VEC_WORDS;
constexpr int COMBINE_SLICES = 12;                 // pair_combine_kernel: 12 x NSLOT = 240 of its 256 threads fold
constexpr int FLOAT_WORDS = 2;                     // the float sweep's record: C, D
constexpr uint64_t NBINS_MAX = 1ull << 36;
constexpr uint64_t LANE_BINS_MAX = NBINS_MAX / CHUNK_BINS * 2;      // bins one lane can meet, if a single wave swept the longest vector
static_assert(B == 4 && HALF == 2 && WG_BINS == KDB_PAIRSTATS_WG_BINS, "include/kdbhip.h states the kernel's constants");
static_assert(COMBINE_SLICES * NSLOT <= 256, "pair_combine_kernel's workgroup");
static_assert(LANE_BINS_MAX < (1ull << 32), "a lane's 32-bit counters (ne, both, nnz) and the 32-bit carry counts of its 64-bit sums cannot wrap");

typedef unsigned __int128 u128;
typedef unsigned long long u64;
typedef unsigned long long u64x2 __attribute__((ext_vector_type(2)));
typedef const __attribute__((address_space(1))) u64x2 *gvec_t;          // the vectors are in global memory: global_load, not flat_load

struct Row { uint8_t a0, na, b0, nb; };            // vectors a0 .. a0 + na against b0 .. b0 + nb; a0 == b0: a diagonal row (then na == nb)

struct Sum96 { u64 lo; uint32_t hi; };             // a lane's sum of at most LANE_BINS_MAX 64-bit terms
struct PairAcc { Sum96 l1; u64 linf; uint32_t ne, both; };
struct VecAcc { Sum96 s; uint32_t nnz; };

__device__ __forceinline__ void add96(Sum96 &a, u64 v) { a.lo += v; a.hi += a.lo < v ? 1u : 0u; }
__device__ __forceinline__ u64 absdiff(u64 x, u64 y) { return x > y ? x - y : y - x; }

__device__ __forceinline__ void pair_bin(PairAcc &p, u64 x, u64 y)
{
    const u64 d = absdiff(x, y);
    add96(p.l1, d);
    p.linf = d > p.linf ? d : p.linf;
    p.ne += d != 0 ? 1u : 0u;
    p.both += (x != 0 && y != 0) ? 1u : 0u;
}

__device__ __forceinline__ u128 wave_sum(u128 a)   // lane 0 gets the wave's sum
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const u64 lo = __shfl_down((u64)a, off), hi = __shfl_down((u64)(a >> 64), off);
        a += ((u128)hi << 64) | lo;
    }
    return a;
}

__device__ __forceinline__ u64 wave_sum(u64 a)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) a += __shfl_down(a, off);
    return a;
}

__device__ __forceinline__ u64 wave_max(u64 a)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { const u64 o = __shfl_down(a, off); a = o > a ? o : a; }
    return a;
}

// record `slot` of a row's ROW_WORDS words
__device__ __forceinline__ int slot_word(int slot) { return slot < NPAIR ? slot * PAIR_WORDS : NPAIR * PAIR_WORDS + (slot - NPAIR) * VEC_WORDS; }

// fold record `slot` of `src` into `acc` (5 words; a vector's record uses 3): sums with the carry from low to high, Linf by max
__device__ __forceinline__ void fold_slot(u64 (&acc)[PAIR_WORDS], const u64 *src, int slot)
{
    const u64 *w = src + slot_word(slot);
    const u128 s = (((u128)acc[1] << 64) | acc[0]) + (((u128)w[1] << 64) | w[0]);
    acc[0] = (u64)s;
    acc[1] = (u64)(s >> 64);
    if (slot < NPAIR) {
        acc[2] = w[2] > acc[2] ? w[2] : acc[2];
        acc[3] += w[3];
        acc[4] += w[4];
    } else {
        acc[2] += w[2];
    }
}

__device__ __forceinline__ void store_slot(u64 *dst, const u64 (&acc)[PAIR_WORDS], int slot)
{
    u64 *w = dst + slot_word(slot);
    w[0] = acc[0]; w[1] = acc[1]; w[2] = acc[2];
    if (slot < NPAIR) { w[3] = acc[3]; w[4] = acc[4]; }
}

// whole chunks of the vectors: chunks 0 .. nchunks of every vector of the row; partials[row][workgroup][ROW_WORDS], `pstride` workgroups per row
template <int NA, int NB, bool DIAG>
__global__ void __launch_bounds__(TPB, 4)
pair_kernel(const u64 *const *__restrict__ vecs, const Row *__restrict__ rows, uint32_t nchunks, uint32_t pstride, u64 *__restrict__ partials)
{
    static_assert(NA >= 1 && NA <= B && NB >= 1 && (DIAG ? NA == NB : NB <= HALF), "row sizes");
    const Row row = rows[blockIdx.y];
    const uint32_t lane = threadIdx.x & 63u, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);         // (scalar: the loop is wave-uniform)
    const u64 *pa[NA], *pb[NB];
#pragma unroll
    for (int i = 0; i < NA; i++) pa[i] = vecs[row.a0 + i];
#pragma unroll
    for (int j = 0; j < NB; j++) pb[j] = DIAG ? pa[j] : vecs[row.b0 + j];

    PairAcc g[NA][NB];
    VecAcc s[NA];
#pragma unroll
    for (int i = 0; i < NA; i++) {
        s[i] = VecAcc{Sum96{0, 0}, 0};
#pragma unroll
        for (int j = 0; j < NB; j++) g[i][j] = PairAcc{Sum96{0, 0}, 0, 0, 0};
    }

    for (uint32_t chunk = blockIdx.x * (TPB / 64) + wave; chunk < nchunks; chunk += gridDim.x * (TPB / 64)) {
        u64x2 xa[NA], xb[NB];                                                          // (one block of unconditional loads)
#pragma unroll
        for (int i = 0; i < NA; i++) xa[i] = ((gvec_t)(pa[i] + (uint64_t)chunk * CHUNK_BINS))[lane];
#pragma unroll
        for (int j = 0; j < NB; j++) {
            if constexpr (DIAG) xb[j] = xa[j];
            else xb[j] = ((gvec_t)(pb[j] + (uint64_t)chunk * CHUNK_BINS))[lane];
        }
#pragma unroll
        for (int i = 0; i < NA; i++) {
            if constexpr (DIAG) {
                add96(s[i].s, xa[i].x);
                add96(s[i].s, xa[i].y);
                s[i].nnz += (xa[i].x != 0 ? 1u : 0u) + (xa[i].y != 0 ? 1u : 0u);
            }
#pragma unroll
            for (int j = DIAG ? i + 1 : 0; j < NB; j++) {
                pair_bin(g[i][j], xa[i].x, xb[j].x);
                pair_bin(g[i][j], xa[i].y, xb[j].y);
            }
        }
    }

    __shared__ u64 red[TPB / 64][ROW_WORDS];
    for (int w = threadIdx.x; w < (TPB / 64) * ROW_WORDS; w += TPB) (&red[0][0])[w] = 0;      // (the slots this row does not use stay zero)
    __syncthreads();
#pragma unroll
    for (int i = 0; i < NA; i++) {
#pragma unroll
        for (int j = DIAG ? i + 1 : 0; j < NB; j++) {
            const u128 l1 = wave_sum(((u128)g[i][j].l1.hi << 64) | g[i][j].l1.lo);
            const u64 linf = wave_max(g[i][j].linf), ne = wave_sum((u64)g[i][j].ne), both = wave_sum((u64)g[i][j].both);
            if (lane == 0) {
                u64 *w = &red[wave][slot_word(i * B + j)];
                w[0] = (u64)l1; w[1] = (u64)(l1 >> 64); w[2] = linf; w[3] = ne; w[4] = both;
            }
        }
        if (DIAG) {
            const u128 sum = wave_sum(((u128)s[i].s.hi << 64) | s[i].s.lo);
            const u64 nnz = wave_sum((u64)s[i].nnz);
            if (lane == 0) {
                u64 *w = &red[wave][slot_word(NPAIR + i)];
                w[0] = (u64)sum; w[1] = (u64)(sum >> 64); w[2] = nnz;
            }
        }
    }
    __syncthreads();
    if (threadIdx.x < NSLOT) {
        u64 acc[PAIR_WORDS] = {0, 0, 0, 0, 0};
#pragma unroll
        for (int w = 0; w < TPB / 64; w++) fold_slot(acc, red[w], threadIdx.x);
        store_slot(partials + ((uint64_t)blockIdx.y * pstride + blockIdx.x) * ROW_WORDS, acc, threadIdx.x);
    }
}

// bins tail0 .. nbins (fewer than CHUNK_BINS) of the row's vectors: one wave per row, plain code, slot by slot; its result is the row's
// partial number `pslot`.  The slots the row does not use are written as zero.
__global__ void __launch_bounds__(64)
pair_tail_kernel(const u64 *const *__restrict__ vecs, const Row *__restrict__ rows, uint64_t tail0, uint64_t nbins, uint32_t pstride, uint32_t pslot,
                 u64 *__restrict__ partials)
{
    const Row row = rows[blockIdx.x];
    const bool diag = row.a0 == row.b0;
    u64 *out = partials + ((uint64_t)blockIdx.x * pstride + pslot) * ROW_WORDS;
    for (int slot = 0; slot < NSLOT; slot++) {
        const bool is_vec = slot >= NPAIR;
        const int i = is_vec ? slot - NPAIR : slot / B, j = is_vec ? 0 : slot % B;
        const bool used = is_vec ? (diag && i < row.na) : (i < row.na && j < row.nb && (!diag || i < j));         // (uniform)
        u64 acc[PAIR_WORDS] = {0, 0, 0, 0, 0};
        if (used) {
            const u64 *x = vecs[row.a0 + i], *y = vecs[row.b0 + j];
            u128 sum = 0;
            u64 mx = 0, c0 = 0, c1 = 0;
            for (uint64_t b = tail0 + threadIdx.x; b < nbins; b += 64) {
                if (is_vec) {
                    sum += x[b];
                    c0 += x[b] != 0;
                } else {
                    const u64 d = absdiff(x[b], y[b]);
                    sum += d;
                    mx = d > mx ? d : mx;
                    c0 += d != 0;
                    c1 += x[b] != 0 && y[b] != 0;
                }
            }
            sum = wave_sum(sum);
            acc[0] = (u64)sum;
            acc[1] = (u64)(sum >> 64);
            if (is_vec) {
                acc[2] = wave_sum(c0);
            } else {
                acc[2] = wave_max(mx);
                acc[3] = wave_sum(c0);
                acc[4] = wave_sum(c1);
            }
        }
        if (threadIdx.x == 0) store_slot(out, acc, slot);
    }
}

// out[row] = a row's `nparts` partial records folded; one workgroup of 256 threads per row
__global__ void __launch_bounds__(256)
pair_combine_kernel(const u64 *__restrict__ partials, uint32_t nparts, u64 *__restrict__ out)
{
    __shared__ u64 red[COMBINE_SLICES][ROW_WORDS];
    const uint32_t slice = threadIdx.x / NSLOT, slot = threadIdx.x % NSLOT;
    if (slice < COMBINE_SLICES) {
        u64 acc[PAIR_WORDS] = {0, 0, 0, 0, 0};
        for (uint32_t w = slice; w < nparts; w += COMBINE_SLICES) fold_slot(acc, partials + ((uint64_t)blockIdx.x * nparts + w) * ROW_WORDS, slot);
        store_slot(red[slice], acc, slot);
    }
    __syncthreads();
    if (threadIdx.x < NSLOT) {
        u64 acc[PAIR_WORDS] = {0, 0, 0, 0, 0};
        for (int sl = 0; sl < COMBINE_SLICES; sl++) fold_slot(acc, red[sl], threadIdx.x);
        store_slot(out + (uint64_t)blockIdx.x * ROW_WORDS, acc, threadIdx.x);
    }
}

// ---- the float sweep ----

struct FloatRow { uint8_t i, j; };                 // one pair per row

// one bin's terms of C and D; sx, sy: the exact sums converted once
__device__ __forceinline__ void float_bin(double &c, double &d, u64 x, u64 y, double sx, double sy)
{
    if ((x | y) == 0) return;
    const double xd = (double)x, yd = (double)y;
    c += (double)absdiff(x, y) / (xd + yd);
    const double p = xd / sx, q = yd / sy, m = 0.5 * (p + q);
    const double tp = x != 0 ? p * log(p / m) : 0.0, tq = y != 0 ? q * log(q / m) : 0.0;
    d += tp + tq;
}

__device__ __forceinline__ double wave_sum_fixed(double a)      // lane 0 gets the wave's sum, the same tree every time
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) a += __shfl_down(a, off);
    return a;
}

// whole chunks: partials[row][workgroup][C, D]
__global__ void __launch_bounds__(TPB, 4)
pairfloat_kernel(const u64 *const *__restrict__ vecs, const FloatRow *__restrict__ rows, const double *__restrict__ sums, uint32_t nchunks, uint32_t pstride,
                 double *__restrict__ partials)
{
    const FloatRow row = rows[blockIdx.y];
    const uint32_t lane = threadIdx.x & 63u, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const u64 *px = vecs[row.i], *py = vecs[row.j];
    const double sx = sums[row.i], sy = sums[row.j];
    double c = 0.0, d = 0.0;
    for (uint32_t chunk = blockIdx.x * (TPB / 64) + wave; chunk < nchunks; chunk += gridDim.x * (TPB / 64)) {
        const u64x2 x = ((gvec_t)(px + (uint64_t)chunk * CHUNK_BINS))[lane], y = ((gvec_t)(py + (uint64_t)chunk * CHUNK_BINS))[lane];
        if (!__any((x.x | x.y | y.x | y.y) != 0)) continue;                           // (a wave of empty bins adds nothing)
        float_bin(c, d, x.x, y.x, sx, sy);
        float_bin(c, d, x.y, y.y, sx, sy);
    }
    __shared__ double red[TPB / 64][FLOAT_WORDS];
    c = wave_sum_fixed(c);
    d = wave_sum_fixed(d);
    if (lane == 0) { red[wave][0] = c; red[wave][1] = d; }
    __syncthreads();
    if (threadIdx.x < FLOAT_WORDS) {
        double r = 0.0;
#pragma unroll
        for (int w = 0; w < TPB / 64; w++) r += red[w][threadIdx.x];
        partials[((uint64_t)blockIdx.y * pstride + blockIdx.x) * FLOAT_WORDS + threadIdx.x] = r;
    }
}

// bins tail0 .. nbins: one wave per row; the row's partial number `pslot`
__global__ void __launch_bounds__(64)
pairfloat_tail_kernel(const u64 *const *__restrict__ vecs, const FloatRow *__restrict__ rows, const double *__restrict__ sums, uint64_t tail0, uint64_t nbins,
                      uint32_t pstride, uint32_t pslot, double *__restrict__ partials)
{
    const FloatRow row = rows[blockIdx.x];
    const u64 *px = vecs[row.i], *py = vecs[row.j];
    const double sx = sums[row.i], sy = sums[row.j];
    double c = 0.0, d = 0.0;
    for (uint64_t b = tail0 + threadIdx.x; b < nbins; b += 64) float_bin(c, d, px[b], py[b], sx, sy);
    c = wave_sum_fixed(c);
    d = wave_sum_fixed(d);
    if (threadIdx.x == 0) {
        double *out = partials + ((uint64_t)blockIdx.x * pstride + pslot) * FLOAT_WORDS;
        out[0] = c;
        out[1] = d;
    }
}

// out[row][C, D] = the row's partials added in a fixed order: 64 lanes take every 64th partial, then the wave's tree
__global__ void __launch_bounds__(64)
pairfloat_combine_kernel(const double *__restrict__ partials, uint32_t nparts, double *__restrict__ out)
{
    double c = 0.0, d = 0.0;
    for (uint32_t w = threadIdx.x; w < nparts; w += 64) {
        const double *p = partials + ((uint64_t)blockIdx.x * nparts + w) * FLOAT_WORDS;
        c += p[0];
        d += p[1];
    }
    c = wave_sum_fixed(c);
    d = wave_sum_fixed(d);
    if (threadIdx.x == 0) {
        out[(uint64_t)blockIdx.x * FLOAT_WORDS] = c;
        out[(uint64_t)blockIdx.x * FLOAT_WORDS + 1] = d;
    }
}

}  // namespace kdbpair
