// kdb_strands.hip.h -- the two strands of a canonical profile, merged once per sync:
//     canonical[c] = forward[c] + forward[rc(c)]   for c <  rc(c)
//     canonical[c] = forward[c]                    for c == rc(c)   (palindromes: even k only)
// A canonical engine counts the FORWARD id of every window into a staging vector F of its own (no reverse-complement word, no min()
// per window in the counting kernels) and strand_merge adds F to the caller-visible vector at the canonical bins, clearing F in the
// same sweep.  rc reverses the k two-bit digits of an id and complements each (A=0 C=1 G=2 T=3: the complement of d is 3 - d = d ^ 3).
//
// Direct form (k <= STRAND_DIRECT_MAX_K, a vector of 512 KiB at most): one thread per id.  The thread of the smaller id of a pair
// reads, adds and clears both strands; the thread of the larger one does nothing, so no two threads touch the same word.
//
// Blocked form (from k = 9): a thread per id reading F[rc(i)] would be 4^k / 2 random 8-byte accesses.  Write
//     id = (A : 3 digits)(M : k - 6 digits)(B : 3 digits).
// For a fixed M the 64 x 64 counters [A][B] are 64 runs of 512 contiguous bytes ("the tile of M").  rc(A, M, B) = (rc B, rc M, rc A): the
// partner of an element lies in the tile of rc(M), transposed and with both indices reverse-complemented.  One workgroup takes the
// unordered pair of tiles {M, rc(M)} (one tile where M == rc(M)): both go to LDS, 2 x 32 KiB, and zeros go over them in F.  Which of i and
// rc(i) is the smaller is decided per element -- A is the leading field, so it does not follow from M < rc(M):
//     (A, M, B) < (rc B, rc M, rc A)   <=>   A < rc B,  or  A == rc B (then B == rc A) and M < rc M.
// The workgroup adds into the vector at the canonical elements of both tiles; where both strands are zero the vector is not touched.
// Every global access of a wave is one run of 512 bytes.
// LDS layout: element (A, B) of a tile sits in row A at column B ^ A.  A wave reads its partners down a column of the other tile
// (row rc B, B = lane): with the xor the 64 lanes fall into 64 different columns, as they do for the row-wise writes.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace kdbstrands {

constexpr int STRAND_DIRECT_MAX_K = 8;
constexpr int TPB = 256;                           // four waves; a wave takes whole rows (lane = B)
constexpr int TILE = 64;                           // 3 digits
constexpr int ROWS = TILE / (TPB / 64);            // rows of a tile per wave

// reverse-complement of an id of k digits (k <= 32)
__host__ __device__ __forceinline__ uint64_t rc_id(uint64_t x, int k)
{
    uint64_t v = ~x;
    v = ((v >> 2) & 0x3333333333333333ull) | ((v & 0x3333333333333333ull) << 2);
    v = ((v >> 4) & 0x0F0F0F0F0F0F0F0Full) | ((v & 0x0F0F0F0F0F0F0F0Full) << 4);
    v = ((v >> 8) & 0x00FF00FF00FF00FFull) | ((v & 0x00FF00FF00FF00FFull) << 8);
    v = ((v >> 16) & 0x0000FFFF0000FFFFull) | ((v & 0x0000FFFF0000FFFFull) << 16);
    v = (v >> 32) | (v << 32);
    return v >> (64 - 2 * k);
}

__global__ __launch_bounds__(TPB) void
strand_merge_direct_kernel(unsigned long long *__restrict__ F, unsigned long long *__restrict__ table, int k)
{
    const uint64_t nbins = 1ull << (2 * k);
    for (uint64_t i = (uint64_t)blockIdx.x * TPB + threadIdx.x; i < nbins; i += (uint64_t)gridDim.x * TPB) {
        const uint64_t r = rc_id(i, k);
        if (i > r) continue;                        // the pair belongs to the thread of r
        unsigned long long s = F[i];
        if (i < r) { s += F[r]; F[r] = 0; }
        F[i] = 0;
        if (s) table[i] += s;
    }
}

// grid: one workgroup per M in [0, 4^(k-6)); those with rc(M) < M leave at once (the workgroup of rc(M) takes the pair)
__global__ __launch_bounds__(TPB) void
strand_merge_kernel(unsigned long long *__restrict__ F, unsigned long long *__restrict__ table, int k)
{
    __shared__ unsigned long long T[2][TILE * TILE];
    const int km = k - 6;
    const uint32_t M0 = blockIdx.x, M1 = (uint32_t)rc_id(M0, km);
    if (M1 < M0) return;
    const bool self = M1 == M0;
    const int ntiles = self ? 1 : 2;
    const uint64_t a_stride = 1ull << (2 * (k - 3));                 // bins between (A, M, B) and (A + 1, M, B)
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint64_t base[2] = {(uint64_t)M0 * TILE + lane, (uint64_t)M1 * TILE + lane};

    // a wave's rows: A = wave, wave + 4, ...  All loads of a tile are issued before the first of them is used
    const uint64_t row_step = (uint64_t)(TPB / 64) * a_stride;
    for (int t = 0; t < ntiles; t++) {
        unsigned long long *p = F + (uint64_t)wave * a_stride + base[t];
        unsigned long long v[ROWS];
#pragma unroll
        for (int j = 0; j < ROWS; j++) v[j] = p[(uint64_t)j * row_step];
#pragma unroll
        for (int j = 0; j < ROWS; j++) {
            const uint32_t A = wave + (uint32_t)j * (TPB / 64);
            T[t][A * TILE + (lane ^ A)] = v[j];
            p[(uint64_t)j * row_step] = 0;
        }
    }
    __syncthreads();

    const uint32_t rcB = (uint32_t)rc_id(lane, 3);                    // the lane's B, reverse-complemented: the partner's A
    for (int t = 0; t < ntiles; t++) {
        const int o = self ? 0 : 1 - t;                               // the tile the partners are in
        const bool m_less = t == 0 && !self;                          // M of this tile < M of the other
        unsigned long long s[ROWS], old[ROWS];
#pragma unroll
        for (int j = 0; j < ROWS; j++) {
            // (A, M, B) against its partner (rc B, rc M, rc A)
            const uint32_t A = wave + (uint32_t)j * (TPB / 64);
            const bool less = A < rcB || (A == rcB && m_less);
            const bool same = A == rcB && self;
            s[j] = 0;
            if (less || same) s[j] = T[t][A * TILE + (lane ^ A)];
            if (less) { const uint32_t rcA = (uint32_t)rc_id(A, 3); s[j] += T[o][rcB * TILE + (rcA ^ rcB)]; }
        }
        unsigned long long *q = table + (uint64_t)wave * a_stride + base[t];
#pragma unroll
        for (int j = 0; j < ROWS; j++) if (s[j]) old[j] = q[(uint64_t)j * row_step];
#pragma unroll
        for (int j = 0; j < ROWS; j++) if (s[j]) q[(uint64_t)j * row_step] = old[j] + s[j];
    }
}

// F and table: 4^k uint64 each, on the current device; stream-ordered, returns after the launch
inline void strand_merge_launch(hipStream_t st, unsigned long long *F, unsigned long long *table, int k)
{
    if (k <= STRAND_DIRECT_MAX_K) {
        const uint64_t nbins = 1ull << (2 * k);
        hipLaunchKernelGGL(strand_merge_direct_kernel, dim3((unsigned)((nbins + TPB - 1) / TPB)), dim3(TPB), 0, st, F, table, k);
    } else {
        hipLaunchKernelGGL(strand_merge_kernel, dim3(1u << (2 * (k - 6))), dim3(TPB), 0, st, F, table, k);
    }
}

}  // namespace kdbstrands
