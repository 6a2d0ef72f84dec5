// kdb_spectrum.hip.h -- the abundance spectrum of a finished count vector (how many bins hold each count value) and the vector's doubled
// mid-ranks, each in one sweep of the vector where it lies in HBM (kdb_spectrum, kdb_rank_transform).
//     dense[v]  = #{b : x[b] == v}                  for v < DENSE = 65536, as uint64
//     over[]    = every x[b] >= DENSE, once per occurrence, in no particular order
//     ranks[b]  = 2 #{c : x[c] < x[b]} + #{c : x[c] == x[b]} + 1      (twice the mid-rank scipy.stats.rankdata gives; an integer)
// The reference walks the 4^k bins in Python for the first (kmerdb/util.py:92-116 get_histo, after every profile: __init__.py:2000); the
// second is what turns Pearson's r into Spearman's rho (python_distances.py:95-114).  Integer adds only, no floating point: the same
// numbers for any grid and from run to run (the order of over[] aside, which nobody relies on: the host sorts it).
//
// spectrum_kernel.  A count profile is the worst case of a shared histogram: most bins hold 0 and the rest a handful of small values, so
// every lane of every wave wants the same few counters.  Three tiers, by value:
//   v < NPRIV      a column of LDS counters per lane (priv[v][thread]): no two lanes ever share a counter, bank = thread % 64, so one
//                  ds_add per bin and no conflict whatever the data -- all-zero, all-equal or mixed.  A wave whose loaded values are all
//                  below NPRIV (nearly every wave of a profile) runs nothing else.
//   v < LDS_BINS   one LDS histogram per workgroup; the lanes of a wave that hold the first lane's value add once, together (an all-equal
//                  vector is one LDS add per wave and load, not 64 serialised ones).
//   v < DENSE      global 64-bit adds to the dense table, merged in the same way.
//   v >= DENSE     compacted: the wave's lanes that hold such a value reserve their slots with ONE add to the list's counter and store behind
//                  one another.  The counter always counts; values are stored while they fit (`cap`): a call that finds the list too short
//                  knows exactly how long it has to be.
// At the end a workgroup adds its non-zero LDS counters to the global table: contiguous 64-bit adds, one per workgroup and value.
// Width of the partial counters: uint32 in LDS.  A workgroup tallies fewer than 2^32 bins -- MAX_GRID workgroups share at most 2^36 bins,
// see the static_assert and spectrum_grid -- so none of them wraps; everything global is uint64.
//
// rank_map_kernel.  Elementwise: out[b] = table(x[b]).  The host made the tables from the spectrum (kdb_spectrum_host.cpp.h): rank_dense[v]
// for v < DENSE, whose first RANK_LDS entries -- the ones nearly every bin hits -- are copied to LDS; larger values are looked up by
// binary search in the sorted distinct overflow values.  A lane loads its bins before it stores them: out may be x itself.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/kdbhip.h"

namespace kdbspectrum {

constexpr uint32_t DENSE = KDB_SPECTRUM_DENSE;     // values below it are tallied, the others listed
constexpr int TPB = 256;                           // four waves
constexpr int CHUNK_BINS = 256;                    // a wave's step: 64 lanes x two 16-byte loads
constexpr int WG_BINS = (TPB / 64) * CHUNK_BINS;   // bins one workgroup covers per grid stride
constexpr uint32_t NPRIV = 16;                     // values with a counter per lane: 16 x 256 x 4 bytes = 16 KiB of LDS
constexpr uint32_t LDS_BINS = 4096;                // values with a counter per workgroup: another 16 KiB
constexpr uint32_t RANK_LDS = 2048;                // rank_map_kernel: entries of the dense rank table kept in LDS (16 KiB)
constexpr uint32_t MAX_GRID = KDB_SPECTRUM_GRID_MAX;   // workgroups of either kernel: four per CU
constexpr uint64_t MAX_BINS = 1ull << 36;          // what the entry points accept
static_assert(DENSE == 65536 && WG_BINS == KDB_SPECTRUM_WG_BINS, "include/kdbhip.h states the kernel's constants");
static_assert(NPRIV <= LDS_BINS && LDS_BINS <= DENSE && RANK_LDS <= DENSE, "the tiers nest");
static_assert((NPRIV & (NPRIV - 1)) == 0, "spectrum_kernel tests a wave's values against NPRIV on their bitwise OR");
static_assert(MAX_BINS / MAX_GRID + 2 * WG_BINS < (1ull << 32), "a workgroup's uint32 LDS counters cannot wrap: it tallies fewer than 2^32 bins");

typedef unsigned long long u64;
typedef unsigned long long u64x2 __attribute__((ext_vector_type(2)));
typedef const __attribute__((address_space(1))) u64x2 *gvec_t;          // the vector is in global memory: global_load, not flat_load

// workgroups for nchunks whole chunks: every workgroup then makes at most ceil(nchunks / (grid * 4)) strides of WG_BINS bins
inline uint32_t spectrum_grid(uint64_t nchunks)
{
    const uint64_t wgs = (nchunks + TPB / 64 - 1) / (TPB / 64);
    return (uint32_t)(wgs < 1 ? 1 : (wgs > MAX_GRID ? MAX_GRID : wgs));
}

__device__ __forceinline__ uint32_t lane_rank_in(uint64_t mask)         // number of set bits below this lane
{
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
}

// one bin.  Any subset of a wave's lanes may call it together: the ballots see the lanes that took the same branch.
__device__ __forceinline__ void tally(uint32_t *priv, uint32_t *hist, u64 *dense, u64 *over, u64 cap, u64 *n_over, u64 v)
{
    if (v < NPRIV) {
        atomicAdd(&priv[(uint32_t)v * TPB + threadIdx.x], 1u);                        // (this lane's own counter)
    } else if (v < DENSE) {
        const uint32_t bin = (uint32_t)v, bin0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)bin);
        const uint64_t same = __ballot(bin == bin0);
        const bool merged = bin == bin0;
        if (merged && lane_rank_in(same) != 0) return;                                // (the first of them adds for all)
        const uint32_t n = merged ? (uint32_t)__popcll(same) : 1u;
        if (bin < LDS_BINS) atomicAdd(&hist[bin], n);
        else __hip_atomic_fetch_add(&dense[bin], (u64)n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    } else {
        const uint64_t active = __ballot(1);
        const uint32_t rank = lane_rank_in(active);
        u64 base = 0;
        if (rank == 0) base = __hip_atomic_fetch_add(n_over, (u64)__popcll(active), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        base = __shfl(base, __ffsll((unsigned long long)active) - 1);
        if (base + rank < cap) over[base + rank] = v;
    }
}

// dense: DENSE words, n_over: one word, both zero before the launch; over: room for `cap` values (not touched when cap == 0)
__global__ void __launch_bounds__(TPB, 4)
spectrum_kernel(const u64 *x, uint64_t nbins, uint64_t nchunks, u64 *__restrict__ dense, u64 *__restrict__ over, u64 cap, u64 *__restrict__ n_over)
{
    __shared__ uint32_t priv[NPRIV * TPB];
    __shared__ uint32_t hist[LDS_BINS];
    const uint32_t lane = threadIdx.x & 63u, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    for (uint32_t i = threadIdx.x; i < NPRIV * TPB; i += TPB) priv[i] = 0;
    for (uint32_t i = threadIdx.x; i < LDS_BINS; i += TPB) hist[i] = 0;
    __syncthreads();

    for (uint64_t chunk = (uint64_t)blockIdx.x * (TPB / 64) + wave; chunk < nchunks; chunk += (uint64_t)gridDim.x * (TPB / 64)) {
        const gvec_t p = (gvec_t)(x + chunk * CHUNK_BINS);
        const u64x2 a = p[lane], b = p[lane + 64];
        if (!__any((a.x | a.y | b.x | b.y) >= NPRIV)) {                               // (wave-uniform: four adds, no branch)
            atomicAdd(&priv[(uint32_t)a.x * TPB + threadIdx.x], 1u);
            atomicAdd(&priv[(uint32_t)a.y * TPB + threadIdx.x], 1u);
            atomicAdd(&priv[(uint32_t)b.x * TPB + threadIdx.x], 1u);
            atomicAdd(&priv[(uint32_t)b.y * TPB + threadIdx.x], 1u);
        } else {
            tally(priv, hist, dense, over, cap, n_over, a.x);
            tally(priv, hist, dense, over, cap, n_over, a.y);
            tally(priv, hist, dense, over, cap, n_over, b.x);
            tally(priv, hist, dense, over, cap, n_over, b.y);
        }
    }
    // the bins behind the whole chunks (fewer than CHUNK_BINS): workgroup 0, one each
    if (blockIdx.x == 0) {
        const uint64_t b = nchunks * CHUNK_BINS + threadIdx.x;
        if (b < nbins) tally(priv, hist, dense, over, cap, n_over, x[b]);
    }
    __syncthreads();

    // a wave sums the 256 per-lane counters of a value; then the workgroup's histogram, 256 neighbouring entries at a time
    for (uint32_t v = wave; v < NPRIV; v += TPB / 64) {
        u64 s = 0;
#pragma unroll
        for (int q = 0; q < TPB / 64; q++) s += priv[v * TPB + q * 64 + lane];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off);
        if (lane == 0 && s) __hip_atomic_fetch_add(&dense[v], s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    for (uint32_t i = NPRIV + threadIdx.x; i < LDS_BINS; i += TPB) {
        const uint32_t c = hist[i];
        if (c) __hip_atomic_fetch_add(&dense[i], (u64)c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

struct RankTables {
    const u64 *rank_dense;     // DENSE entries: the doubled mid-rank of every value below DENSE (whatever, where the value does not occur)
    const u64 *over_values;    // the distinct values >= DENSE, ascending
    const u64 *over_ranks;     // their doubled mid-ranks
    uint32_t n_over;           // how many
};

__device__ __forceinline__ u64 rank_of(const u64 *lds_rank, const RankTables &t, u64 v)
{
    if (v < RANK_LDS) return lds_rank[(uint32_t)v];
    if (v < DENSE) return t.rank_dense[(uint32_t)v];
    uint32_t lo = 0, hi = t.n_over;                                                   // the first entry >= v: it IS v, the spectrum listed it
    while (lo < hi) { const uint32_t mid = lo + ((hi - lo) >> 1); if (t.over_values[mid] < v) lo = mid + 1; else hi = mid; }
    return lo < t.n_over ? t.over_ranks[lo] : 0;
}

// out[b] = doubled mid-rank of x[b]; out == x is allowed (no __restrict__ on either)
__global__ void __launch_bounds__(TPB, 4)
rank_map_kernel(const u64 *x, uint64_t nbins, uint64_t nchunks, RankTables t, u64 *out)
{
    __shared__ u64 lds_rank[RANK_LDS];
    const uint32_t lane = threadIdx.x & 63u, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    for (uint32_t i = threadIdx.x; i < RANK_LDS; i += TPB) lds_rank[i] = t.rank_dense[i];
    __syncthreads();
    for (uint64_t chunk = (uint64_t)blockIdx.x * (TPB / 64) + wave; chunk < nchunks; chunk += (uint64_t)gridDim.x * (TPB / 64)) {
        const gvec_t p = (gvec_t)(x + chunk * CHUNK_BINS);
        u64x2 a = p[lane], b = p[lane + 64];
        a.x = rank_of(lds_rank, t, a.x); a.y = rank_of(lds_rank, t, a.y);
        b.x = rank_of(lds_rank, t, b.x); b.y = rank_of(lds_rank, t, b.y);
        u64x2 *q = (u64x2 *)(out + chunk * CHUNK_BINS);
        q[lane] = a; q[lane + 64] = b;
    }
    if (blockIdx.x == 0) {
        const uint64_t b = nchunks * CHUNK_BINS + threadIdx.x;
        if (b < nbins) out[b] = rank_of(lds_rank, t, x[b]);
    }
}

}  // namespace kdbspectrum
