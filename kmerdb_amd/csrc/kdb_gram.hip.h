// kdb_gram.hip.h -- exact integer moments of finished count vectors, in one sweep at memory speed (kdb_gram):
//     S[i]    = Sum_b x_i[b]              for each of n vectors of nbins uint64
//     G[i][j] = Sum_b x_i[b] * x_j[b]     for every pair i <= j
// as 128-bit integers.  Every distance kmerdb offers on count profiles (kmerdb/__init__.py:577-813: correlation, pearson, cosine,
// euclidean) is a function of these and of nbins; kmerdb_amd/distance.py takes it from there on the host, in exact arithmetic.
//
// Overflow -- the whole argument: if every S[i] < 2^64 then G[i][j] <= S[i] * S[j] < 2^128, and so is every partial sum of it (all terms
// are non-negative).  128-bit accumulation with carries therefore cannot wrap, per lane, per wave, per workgroup or in the final sum.
// S itself is a sum of at most 2^64 terms below 2^64: it fits 128 bits always, so the host can TEST S[i] < 2^64 on the exact value and
// refuse the call (KDB_ERR_ARG) when it does not hold.
//
// Shape.  The vectors are taken in blocks of B = 4.  A workgroup row (blockIdx.y) owns one pair of blocks (bi <= bj).  gram_kernel sweeps the
// whole chunks of the vectors (a chunk = 128 bins = one 16-byte load per lane of a wave): a lane loads two bins of each vector of the row's
// blocks and keeps the row's accumulators in registers -- NA x NB pairs off the diagonal (the second block's vectors come in passes of two, or of one where all four are there), the
// NA (NA + 1) / 2 pairs i <= j and the NA sums on it: 64 VGPRs of accumulators at most, 128 in all, no scratch -- four waves per SIMD like the
// other streaming kernels.  Block sizes are template arguments: the last block of n vectors may hold 1..3.
// A wave whose loaded values are all below 2^32 (nearly every wave of a count profile) takes one 32 x 32 -> 64 multiply and a carry chain per
// pair and bin; otherwise the full 64 x 64 -> 128 product.  Both are exact; which one ran does not show in the result.
// Waves reduce with shuffles that carry, workgroups through LDS; each workgroup writes its (lo, hi) per slot to `partials`.  The vectors' last
// nbins % 128 bins are gram_tail_kernel's (one wave per row, plain code); its result is one more partial.  gram_combine_kernel adds a row's
// partials.  Integer adds only, no atomics, no floating point: the result is the same for any grid and from run to run.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/kdbhip.h"

namespace kdbgram {

constexpr int B = KDB_GRAM_BLOCK;                  // vectors per block
constexpr int TPB = 256;                           // four waves
constexpr int CHUNK_BINS = 128;                    // a wave's step: 64 lanes x 16 bytes
constexpr int WG_BINS = (TPB / 64) * CHUNK_BINS;   // bins one workgroup covers per grid stride
constexpr int NSLOT = B * B + B;                   // a row's results: pair (i, j) of its blocks in slot i * B + j, sum of vector i (diagonal rows) in B * B + i
constexpr int COMBINE_SLICES = 12;                 // gram_combine_kernel: 12 x NSLOT = 240 of its 256 threads add
static_assert(B == 4 && WG_BINS == KDB_GRAM_WG_BINS, "include/kdbhip.h states the kernel's constants");
static_assert(COMBINE_SLICES * NSLOT <= 256, "gram_combine_kernel's workgroup");

typedef unsigned __int128 u128;                    // (the compiler turns its adds into one carry chain: v_add_co, then v_addc per further dword)
typedef unsigned long long u64x2 __attribute__((ext_vector_type(2)));
typedef const __attribute__((address_space(1))) u64x2 *gvec_t;          // the vectors are in global memory: global_load, not flat_load

struct Row { uint8_t bi, bj; };                    // the row's blocks: vectors bi * B ... and bj * B ...

__device__ __forceinline__ u128 from_words(ulonglong2 x) { return ((u128)x.y << 64) | x.x; }
__device__ __forceinline__ ulonglong2 to_words(u128 v) { return make_ulonglong2((unsigned long long)v, (unsigned long long)(v >> 64)); }

__device__ __forceinline__ void add_mul32(u128 &a, uint32_t x, uint32_t y) { a += (unsigned long long)x * y; }

__device__ __forceinline__ void add_mul64(u128 &a, unsigned long long x, unsigned long long y) { a += (u128)x * y; }

__device__ __forceinline__ u128 wave_sum(u128 a)   // lane 0 gets the wave's sum
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long lo = __shfl_down((unsigned long long)a, off), hi = __shfl_down((unsigned long long)(a >> 64), off);
        a += ((u128)hi << 64) | lo;
    }
    return a;
}

// the wave's chunk of N vectors: scalar base + lane offset, one block of unconditional loads
template <int N>
__device__ __forceinline__ void load_chunk(u64x2 (&x)[N], const unsigned long long *(&p)[N], uint32_t chunk, uint32_t lane)
{
#pragma unroll
    for (int i = 0; i < N; i++) x[i] = ((gvec_t)(p[i] + (uint64_t)chunk * CHUNK_BINS))[lane];
}

// g[i][J0 + j] += xa[i] . xb[j] for both bins of the element; wave-uniform choice of the multiply
template <int NA, int NB, int J0, int NJ, bool DIAG>
__device__ __forceinline__ void accumulate(u128 (&g)[NA][NB], const u64x2 (&xa)[NA], const u64x2 (&xb)[NJ], unsigned long long any_hi)
{
    if (!__any((int)(any_hi >> 32))) {
#pragma unroll
        for (int i = 0; i < NA; i++) {
#pragma unroll
            for (int j = DIAG ? i : 0; j < NJ; j++) {
                add_mul32(g[i][J0 + j], (uint32_t)xa[i].x, (uint32_t)xb[j].x);
                add_mul32(g[i][J0 + j], (uint32_t)xa[i].y, (uint32_t)xb[j].y);
            }
            __builtin_amdgcn_sched_barrier(0);                                        // (a row of pairs at a time: see below)
        }
    } else {
#pragma unroll
        for (int i = 0; i < NA; i++) {
#pragma unroll
            for (int j = DIAG ? i : 0; j < NJ; j++) {
                add_mul64(g[i][J0 + j], xa[i].x, xb[j].x);
                __builtin_amdgcn_sched_barrier(0);                                    // (one product's temporaries at a time: registers are short here, not time)
                add_mul64(g[i][J0 + j], xa[i].y, xb[j].y);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
    }
}

// gram_kernel off the diagonal: vectors J0 .. J0 + NJ of the second block against the NA loaded ones of the first
template <int NA, int NB, int J0, int NJ>
__device__ __forceinline__ void cross_pass(u128 (&g)[NA][NB], const u64x2 (&xa)[NA], unsigned long long a_hi, const unsigned long long *(&pb)[NB],
                                           uint32_t chunk, uint32_t lane)
{
    const unsigned long long *pj[NJ];
    u64x2 xb[NJ];
#pragma unroll
    for (int j = 0; j < NJ; j++) pj[j] = pb[J0 + j];
    load_chunk(xb, pj, chunk, lane);
    unsigned long long any_hi = a_hi;
#pragma unroll
    for (int j = 0; j < NJ; j++) any_hi |= xb[j].x | xb[j].y;
    accumulate<NA, NB, J0, NJ, false>(g, xa, xb, any_hi);
    __builtin_amdgcn_sched_barrier(0);                                                // (the next pass loads after this one is done with its registers)
}

// whole chunks of the vectors: chunks 0 .. nchunks of every vector of the row's blocks; partials[row][workgroup][slot], `pstride` workgroups per row
template <int NA, int NB, bool DIAG>
__global__ void __launch_bounds__(TPB, 4)
gram_kernel(const unsigned long long *const *__restrict__ vecs, const Row *__restrict__ rows, uint32_t nchunks, uint32_t pstride, ulonglong2 *__restrict__ partials)
{
    static_assert(NA >= 1 && NA <= B && NB >= 1 && NB <= B && (!DIAG || NA == NB), "block sizes");
    const Row row = rows[blockIdx.y];
    const uint32_t lane = threadIdx.x & 63u, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);         // (scalar: the loop is wave-uniform)
    const unsigned long long *pa[NA], *pb[NB];
#pragma unroll
    for (int i = 0; i < NA; i++) pa[i] = vecs[row.bi * B + i];
#pragma unroll
    for (int j = 0; j < NB; j++) pb[j] = DIAG ? pa[j] : vecs[row.bj * B + j];

    u128 g[NA][NB], s[NA];
#pragma unroll
    for (int i = 0; i < NA; i++) {
        s[i] = 0;
#pragma unroll
        for (int j = 0; j < NB; j++) g[i][j] = 0;
    }

    for (uint32_t chunk = blockIdx.x * (TPB / 64) + wave; chunk < nchunks; chunk += gridDim.x * (TPB / 64)) {
        u64x2 xa[NA];
        load_chunk(xa, pa, chunk, lane);
        unsigned long long a_hi = 0;
#pragma unroll
        for (int i = 0; i < NA; i++) a_hi |= xa[i].x | xa[i].y;
        if (DIAG) {
#pragma unroll
            for (int i = 0; i < NA; i++) { s[i] += xa[i].x; s[i] += xa[i].y; }
            accumulate<NA, NB, 0, NA, true>(g, xa, xa, a_hi);
        } else {
            // the second block in two passes (one vector at a time where all four are there): 16 + 8 registers of loaded bins at most beside the accumulators
            if constexpr (NB < B) {
                cross_pass<NA, NB, 0, (NB < 2 ? NB : 2)>(g, xa, a_hi, pb, chunk, lane);
                if constexpr (NB > 2) cross_pass<NA, NB, 2, NB - 2>(g, xa, a_hi, pb, chunk, lane);
            } else {
                cross_pass<NA, NB, 0, 1>(g, xa, a_hi, pb, chunk, lane);
                cross_pass<NA, NB, 1, 1>(g, xa, a_hi, pb, chunk, lane);
                cross_pass<NA, NB, 2, 1>(g, xa, a_hi, pb, chunk, lane);
                cross_pass<NA, NB, 3, 1>(g, xa, a_hi, pb, chunk, lane);
            }
        }
    }

    __shared__ ulonglong2 red[TPB / 64][NSLOT];
#pragma unroll
    for (int slot = 0; slot < NSLOT; slot++) {
        const int i = slot < B * B ? slot / B : slot - B * B, j = slot < B * B ? slot % B : 0;
        const bool used = slot < B * B ? (i < NA && j < NB && (!DIAG || i <= j)) : (DIAG && i < NA);
        u128 r = 0;
        if (used) r = wave_sum(slot < B * B ? g[i < NA ? i : 0][j < NB ? j : 0] : s[i < NA ? i : 0]);
        if (lane == 0) red[wave][slot] = to_words(r);
    }
    __syncthreads();
    if (threadIdx.x < NSLOT) {
        u128 r = 0;
#pragma unroll
        for (int w = 0; w < TPB / 64; w++) r += from_words(red[w][threadIdx.x]);
        partials[((uint64_t)blockIdx.y * pstride + blockIdx.x) * NSLOT + threadIdx.x] = to_words(r);
    }
}

// bins tail0 .. nbins (fewer than CHUNK_BINS) of the vectors: one wave per row, two bins per lane at most, the full product, slot by slot;
// its result is the row's partial number `pslot`.  n = number of vectors: the slots of vectors past it, and below the diagonal, stay zero.
__global__ void __launch_bounds__(64)
gram_tail_kernel(const unsigned long long *const *__restrict__ vecs, const Row *__restrict__ rows, int n, uint64_t tail0, uint64_t nbins,
                 uint32_t pstride, uint32_t pslot, ulonglong2 *__restrict__ partials)
{
    const Row row = rows[blockIdx.x];
    const bool diag = row.bi == row.bj;
    for (int slot = 0; slot < NSLOT; slot++) {
        const bool is_sum = slot >= B * B;
        const int vi = row.bi * B + (is_sum ? slot - B * B : slot / B), vj = is_sum ? vi : row.bj * B + slot % B;
        const bool used = vi < n && vj < n && (is_sum ? diag : vi <= vj);              // (uniform)
        u128 r = 0;
        if (used) {
            const unsigned long long *x = vecs[vi], *y = vecs[vj];
            for (uint64_t b = tail0 + threadIdx.x; b < nbins; b += 64) r += is_sum ? (u128)x[b] : (u128)x[b] * y[b];
            r = wave_sum(r);
        }
        if (threadIdx.x == 0) partials[((uint64_t)blockIdx.x * pstride + pslot) * NSLOT + slot] = to_words(r);
    }
}

// out[row][slot] = Sum over the row's `nparts` partials of partials[row][part][slot]; one workgroup of 256 threads per row
__global__ void __launch_bounds__(256)
gram_combine_kernel(const ulonglong2 *__restrict__ partials, uint32_t nparts, ulonglong2 *__restrict__ out)
{
    __shared__ ulonglong2 red[COMBINE_SLICES][NSLOT];
    const uint32_t slice = threadIdx.x / NSLOT, slot = threadIdx.x % NSLOT;
    if (slice < COMBINE_SLICES) {
        u128 r = 0;
        for (uint32_t w = slice; w < nparts; w += COMBINE_SLICES) r += from_words(partials[((uint64_t)blockIdx.x * nparts + w) * NSLOT + slot]);
        red[slice][slot] = to_words(r);
    }
    __syncthreads();
    if (threadIdx.x < NSLOT) {
        u128 r = 0;
        for (int sl = 0; sl < COMBINE_SLICES; sl++) r += from_words(red[sl][threadIdx.x]);
        out[(uint64_t)blockIdx.x * NSLOT + threadIdx.x] = to_words(r);
    }
}

}  // namespace kdbgram
